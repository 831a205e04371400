"""The MSM's host tail with a level-0 chunk length that is not a power of two (msm_host_fold):
    out = sum_w 2^(off_w) (A_w + L0 sum_b 2^b U_(w,b)),   L0 = 1 .. 128,
on caller-supplied part sums, against one naive MSM of the oracle's over the same points with those weights.  Host only."""
import ctypes as C

import numpy as np
import pytest

import algebra_amd as A
import oracle_lib as O
from algebra_amd import _lib

A4 = np.array([0xA11CE, 1, 2, 0], dtype=np.uint64)
B4 = np.array([0xB0B, 3, 0, 0], dtype=np.uint64)


def make_parts(cid, windows, nbits):
    """windows x (nbits + 1) bucket-form points (x t^2, y t^3, t^2, t^3), a different t each, some the identity"""
    fw = O.fe_words(cid)
    npts = windows * (nbits + 1)
    aff = O.gen_bases(cid, A4, B4, npts + 1)
    t_src = O.gen_bases(cid, B4, A4, npts)
    parts = np.zeros((windows, nbits + 1, 4 * fw), dtype=np.uint64)
    live = []
    for w in range(windows):
        for q in range(nbits + 1):
            k = w * (nbits + 1) + q
            if k % 7 == 4:
                continue                                            # identity part: all-zero cell
            x, y = aff[k][:fw], aff[k][fw:]
            t = t_src[k][:fw]
            t2 = O.basefield_op(cid, "mul", t, t)
            t3 = O.basefield_op(cid, "mul", t2, t)
            parts[w, q, :fw] = O.basefield_op(cid, "mul", x, t2)
            parts[w, q, fw:2 * fw] = O.basefield_op(cid, "mul", y, t3)
            parts[w, q, 2 * fw:3 * fw] = t2
            parts[w, q, 3 * fw:] = t3
            live.append((w, q, aff[k]))
    return np.ascontiguousarray(parts), live


@pytest.mark.parametrize("cname", O.CURVES)
def test_host_tail_with_any_chunk_length(cname):
    cid = O.CID[cname]
    fw = O.fe_words(cid)
    # (>= 4 windows over Fp2: the helper pool's tail; fewer: the single thread's; one window: a prepared set)
    for windows, nbits, widths, l0s in ((5, 4, [9, 9, 9, 8, 8], range(1, 129)), (2, 6, [11, 10], (1, 2, 3, 5, 21, 53, 64, 96, 127, 128)),
                                        (1, 3, [13], (1, 6, 7, 100))):
        parts, live = make_parts(cid, windows, nbits)
        off = [sum(widths[:w]) for w in range(windows)]
        wid = (C.c_int * windows)(*widths)
        pts = np.stack([p for _, _, p in live])
        for l0 in l0s:
            weights = [(1 << off[w]) if q == nbits else (l0 << (off[w] + q)) for w, q, _ in live]
            out = np.zeros(3 * fw, dtype=np.uint64)
            rc = _lib.test_lib().ark_hip_test_msm_host_fold_l0(cid, parts.ctypes.data_as(C.c_void_p), windows, nbits, l0, wid,
                                                               out.ctypes.data_as(C.c_void_p))
            assert rc == 0
            sc = np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in weights], dtype=np.uint64)
            want = O.to_affine(cid, O.msm(cid, pts, sc, O.NAIVE))
            assert np.array_equal(A.into_affine(cid, out), want), (cname, windows, nbits, l0)
    none = C.c_void_p(None)
    assert _lib.test_lib().ark_hip_test_msm_host_fold_l0(cid, none, 1, 1, 3, none, none) != 0          # argument checks
    out = np.zeros(3 * fw, dtype=np.uint64)
    for bad in (0, -1, 65537):
        assert _lib.test_lib().ark_hip_test_msm_host_fold_l0(cid, parts.ctypes.data_as(C.c_void_p), 1, 3, bad, wid,
                                                             out.ctypes.data_as(C.c_void_p)) != 0


def test_powers_of_two_agree_with_the_log2_hook():
    cid = O.CID["BLS12_381_G1"]
    fw = O.fe_words(cid)
    parts, _ = make_parts(cid, 6, 5)
    wid = (C.c_int * 6)(10, 10, 10, 10, 9, 9)
    for k in range(0, 8):
        a, b = np.zeros(3 * fw, dtype=np.uint64), np.zeros(3 * fw, dtype=np.uint64)
        assert _lib.test_lib().ark_hip_test_msm_host_fold(cid, parts.ctypes.data_as(C.c_void_p), 6, 5, k, wid, a.ctypes.data_as(C.c_void_p)) == 0
        assert _lib.test_lib().ark_hip_test_msm_host_fold_l0(cid, parts.ctypes.data_as(C.c_void_p), 6, 5, 1 << k, wid,
                                                             b.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(a, b), k
