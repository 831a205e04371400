"""Child process of tests/test_gpu_reduce_s30.py: BLS12-381 G1 MSMs of 2^10 and 2^12 pairs against the oracle with the plan forced
so that every kernel of the bucket reduction, the heavy-run kernels and the first entries of a bucket each run once.
ARK_HIP_MSM_SPLIT_LEVEL is read once per process (the environment this process was started with picks the one-lane or the
two-wave level-0 kernel); the other knobs are read per call and set here.
    python tests/reduce_s30_child.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import algebra_amd as A
import oracle_lib as O

CID = O.CID["BLS12_381_G1"]
FW = O.fe_words(CID)
BITS = 255
A4 = np.array([0xA11CE, 1, 2, 0], dtype=np.uint64)
B4 = np.array([0xB0B, 3, 0, 0], dtype=np.uint64)
KNOBS = ("ARK_HIP_MSM_C", "ARK_HIP_MSM_STAGE2", "ARK_HIP_MSM_HEAVY", "ARK_HIP_MSM_L0", "ARK_HIP_MSM_RUN_PARTS")


def narrow_windows(c):
    """top windows one bit narrower (msm_window_layout)"""
    w = (BITS + c - 1) // c
    deficit = w * c - BITS
    return 0 if deficit > w or c < 3 else deficit


def run(name, bases, scalars, **knobs):
    for k in KNOBS:
        os.environ.pop(k, None)
    for k, v in knobs.items():
        os.environ["ARK_HIP_MSM_" + k] = str(v)
    got = A.msm_bigint(CID, torch.from_numpy(bases.view(np.int64)).cuda(), torch.from_numpy(scalars.view(np.int64)).cuda())
    exp = O.msm(CID, bases, scalars, O.SIGNED, 4)
    assert np.array_equal(A.into_affine(CID, got), O.to_affine(CID, exp)), name
    print("ok", name, knobs, flush=True)


def bucket_loads(scalars, c, window):
    """entries per bucket of one window, as the oracle's signed digits fill them"""
    loads = {}
    for s in scalars:
        d = O.make_digits(s, c, BITS)[window]
        if d:
            loads[abs(int(d))] = loads.get(abs(int(d)), 0) + 1
    return loads


def main():
    n12 = 1 << 12
    bases = O.gen_bases(CID, A4, B4, n12).reshape(n12, 2 * FW)
    scalars = O.gen_scalars(O.curve_info(CID)[1], 7, n12).reshape(n12, 4)
    b10, s10 = np.ascontiguousarray(bases[:1 << 10]), np.ascontiguousarray(scalars[:1 << 10])
    # the one-kernel second stage and the two-digit one, a plan with narrow top windows (c = 8: one, c = 10: five) and one without
    assert narrow_windows(8) == 1 and narrow_windows(10) == 5 and narrow_windows(5) == 0
    run("2^10 one-kernel stage", b10, s10, C=8, STAGE2=0)
    run("2^10 two-digit stage", b10, s10, C=8, STAGE2=1)
    run("2^12 one-kernel stage", bases, scalars, C=10, STAGE2=0)
    run("2^12 two-digit stage", bases, scalars, C=10, STAGE2=1)
    run("2^10 no narrow window, ragged chunks", b10, s10, C=5, STAGE2=0, L0=3)
    run("2^12 the plan's own", bases, scalars)
    # heavy runs: all scalars equal, one bucket per window holds every pair, the threshold forced below its load
    eq = np.ascontiguousarray(np.repeat(scalars[5:6], 1 << 10, axis=0))
    run("2^10 heavy runs", b10, eq, C=8, HEAVY=64)
    eq12 = np.ascontiguousarray(np.repeat(scalars[9:10], n12, axis=0))
    run("2^12 heavy runs", bases, eq12, C=10, HEAVY=64, STAGE2=1)
    # buckets of exactly one, two and three entries (c = 12 at 2^10: 2048 buckets per window for 1024 pairs); duplicate bases and a
    # base with its negative under one scalar -- the lowest indices, so a doubling and an infinity inside a bucket's first two entries
    d10, ds10 = b10.copy(), s10.copy()
    d10[1], ds10[1] = d10[0], ds10[0]
    d10[3, :FW] = d10[2, :FW]
    d10[3, FW:] = O.basefield_op(CID, "neg", d10[2, FW:])
    ds10[3] = ds10[2]
    d10[6], ds10[6] = d10[4], ds10[4]              # P, Q, P in one bucket: the third entry meets a sum
    ds10[5] = ds10[4]
    loads = bucket_loads(ds10, 12, 0)
    assert {1, 2, 3} <= set(loads.values()), sorted(set(loads.values()))
    # (at these sizes the default plan splits runs over lanes: msm_accumulate_parts_kernel and msm_sum_parts_kernel; RUN_PARTS=1 gives
    # every run to one lane of msm_accumulate_lazy_kernel, whose buckets the reduction then reads)
    run("2^10 one, two and three entries; P P, P -P, P Q P", d10, ds10, C=12, STAGE2=0, RUN_PARTS=1)
    run("2^10 the same, runs split over lanes", d10, ds10, C=12, STAGE2=0)
    run("2^10 the same at c = 8", d10, ds10, C=8, STAGE2=1, RUN_PARTS=1)
    d12, ds12 = bases.copy(), scalars.copy()
    d12[:8], ds12[:8] = d10[:8], ds10[:8]
    run("2^12 duplicates and opposite bases", d12, ds12, C=13, STAGE2=1, RUN_PARTS=1)
    run("2^12 one lane per run", bases, scalars, C=10, STAGE2=0, RUN_PARTS=1)
    print("reduce-s30 ok", flush=True)


if __name__ == "__main__":
    main()
