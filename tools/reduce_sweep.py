#!/usr/bin/env python3
"""Reduction geometry sweep: level-0 run length (ARK_HIP_MSM_L0, powers of two and not) x second stage (ARK_HIP_MSM_STAGE2:
one kernel with its chunk ARK_HIP_MSM_CHUNK, or two digits) against the library's own choice, device-resident plain MSM, every result checked against k*G.
    python tools/reduce_sweep.py CURVE LOG_N [LOG_N ...]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import algebra_amd as A
import synth as S
from algebra_amd import curves as cv
from algebra_amd._lib import check, lib

curve = sys.argv[1]
cid = cv.curve_id(curve)
r = S.R[cv.scalar_field(cid)]
L = lib()
for logn in [int(x) for x in sys.argv[2:]]:
    n = 1 << logn
    bases = S.grow_bases(cid, n, S.A0, S.B0, r)
    sc = S.gen_scalars(n, 5, r)
    d = torch.from_numpy(sc.view(np.int64)).cuda()
    kg = S.mul_gen(cid, S.dlog_of_msm(sc, S.A0, S.B0, r), r)

    def run(steps=6):
        A.msm_bigint(cid, bases, d)
        check(L.ark_hip_msm_set_timing(1), "t")
        t0 = time.perf_counter()
        for _ in range(steps):
            res = A.msm_bigint(cid, bases, d)
        dt = (time.perf_counter() - t0) / steps
        tm = (C.c_double * 8)()
        L.ark_hip_msm_last_timing(tm)
        check(L.ark_hip_msm_set_timing(0), "t")
        ok = bool(np.array_equal(A.into_affine(cid, res), kg))
        return dt * 1e3, tm[4], ok

    KNOBS = ("ARK_HIP_MSM_L0", "ARK_HIP_MSM_CHUNK", "ARK_HIP_MSM_STAGE2")
    for k in KNOBS:
        os.environ.pop(k, None)
    ms, red, ok = run()
    print("%s 2^%d plan %s: library choice %.3f ms (reduce %.3f)%s" % (curve, logn, A.msm_plan(cid, n), ms, red, "" if ok else " WRONG"), flush=True)
    # level-0 chunk length (any integer: the last chunk of a window is ragged) x second stage: the one-kernel bit-sliced form
    # with its chunk sizes, then the two-digit form (row and column sums; no chunk knob)
    l0s = (1, 2, 3, 4, 6, 8, 12, 16) if logn < 16 else (4, 6, 8, 11, 12, 16, 21, 24, 32) if logn < 22 else (8, 11, 13, 16, 21, 22, 24, 26, 32, 43, 64)
    for l0 in l0s:
        line = "  L0=%-2d" % l0
        os.environ["ARK_HIP_MSM_L0"] = str(l0)
        os.environ["ARK_HIP_MSM_STAGE2"] = "0"
        for ch in ((256, 1024, 4096) if logn < 16 else (512, 1024, 2048) if logn < 22 else (2048, 4096, 8192)):
            os.environ["ARK_HIP_MSM_CHUNK"] = str(ch)
            ms, red, ok = run()
            line += "  chunk %4d: %.3f (%.3f)%s" % (ch, ms, red, "" if ok else "!")
        os.environ.pop("ARK_HIP_MSM_CHUNK")
        os.environ["ARK_HIP_MSM_STAGE2"] = "1"
        ms, red, ok = run()
        line += "  two-digit: %.3f (%.3f)%s" % (ms, red, "" if ok else "!")
        print(line, flush=True)
    for k in KNOBS:
        os.environ.pop(k, None)
    del bases, d
    torch.cuda.empty_cache()
