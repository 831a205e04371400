"""The MSM's host-side planning (csrc/msm_plan.hpp) without a GPU:
  * the bucket reduction's geometry (msm_reduce_geometry through its test hook) at the cells the code's comments and
    DESIGN.md document, derived by hand from the rules, and its identities over every window size on every curve;
  * the window plan (ark_hip_msm_plan) against the cells recorded before the planner moved into that header
    (tests/golden/msm_plan_cells.json)."""
import ctypes as C
import json
import os

import pytest

import algebra_amd as A
from algebra_amd import _lib

CURVES = ["BN254_G1", "BLS12_381_G1", "BLS12_377_G1", "BLS12_377_G2", "BLS12_381_G2"]
SCALAR_BITS = {"BN254_G1": 254, "BLS12_381_G1": 255, "BLS12_377_G1": 253, "BLS12_377_G2": 253, "BLS12_381_G2": 255}
FIELDS = ("L0", "m", "mn", "nbits", "Q", "two_digit", "d2", "rows2", "nsum2", "chunk", "nchunks", "npairs")
RESIDENT = 131072   # 2 workgroups of 128 x 2 x 256 CUs: what the level-0 kernel keeps resident on the chip


def geometry(curve, c, W, narrow, shared=False, resident=RESIDENT):
    out = (C.c_uint32 * 12)()
    rc = _lib.test_lib().ark_hip_test_msm_reduce_geometry(CURVES.index(curve), c, W, narrow, int(shared), resident, out)
    assert rc == 0, rc
    return dict(zip(FIELDS, out))


def layout(c, bits):
    """msm_window_layout: W windows of c bits, the top `narrow` one bit narrower"""
    w = (bits + c - 1) // c
    deficit = w * c - bits
    if deficit > w or c < 3:
        return (bits + c) // c, 0
    return w, deficit


def test_large_plain_job_fills_whole_rounds():
    """BLS12-381 G1 at 2^24 (c = 20): 172 032 level-0 chunks at L0 = 32 are 1.31 rounds of 131 072 resident lanes; L0 = 22 is
    the smallest whose chunks fit two (8 x 23 832 + 5 x 11 916 = 250 236; L0 = 21: 262 156 > 262 144)."""
    assert layout(20, 255) == (13, 5)
    g32 = geometry("BLS12_381_G1", 20, 13, 5, resident=0)   # occupancy unknown: the power of two stays
    assert (g32["L0"], g32["m"], g32["nbits"], g32["Q"]) == (32, 16384, 14, 15)
    assert 8 * g32["m"] + 5 * g32["mn"] == 172032
    g = geometry("BLS12_381_G1", 20, 13, 5)
    assert (g["L0"], g["m"], g["mn"], g["nbits"], g["Q"]) == (22, 23832, 11916, 15, 16)
    assert (g["two_digit"], g["d2"], g["rows2"], g["nsum2"], g["nchunks"]) == (1, 7, 187, 502, 1)
    assert 8 * -(-(1 << 19) // 21) + 5 * -(-(1 << 18) // 21) == 262156


def test_prepared_set_reduces_one_window():
    g = geometry("BLS12_381_G1", 22, 12, 9, shared=True)   # 2^21 buckets
    assert (g["L0"], g["m"], g["nbits"], g["Q"], g["two_digit"], g["d2"], g["rows2"]) == (16, 1 << 17, 17, 18, 1, 8, 512)
    assert g["npairs"] == 18


def test_small_job_takes_short_chunks_and_one_kernel():
    g = geometry("BLS12_381_G1", 12, 22, 9)   # 45 056 buckets
    assert (g["L0"], g["m"], g["mn"], g["nbits"], g["Q"]) == (4, 512, 256, 9, 10)
    assert (g["two_digit"], g["chunk"], g["nchunks"]) == (0, 512, 1)


def test_lane_pair_curves_cap_the_chunk_by_scalar_width():
    assert layout(19, 253) == (14, 13) and layout(19, 255) == (14, 11)
    assert geometry("BLS12_377_G2", 19, 14, 13)["L0"] == 64
    assert geometry("BLS12_381_G2", 19, 14, 11)["L0"] == 32


@pytest.mark.parametrize("curve", CURVES)
def test_identities_over_every_window_size(curve):
    for shared in (False, True):
        for c in range(3, 24):
            W, narrow = layout(c, SCALAR_BITS[curve])
            for resident in (0, RESIDENT):
                g = geometry(curve, c, W, narrow, shared, resident)
                where = (curve, shared, c, resident, g)
                mwin = 1 << (c - 1)
                assert 1 <= g["L0"] <= mwin, where
                assert g["m"] == -(-mwin // g["L0"]), where
                assert g["Q"] == g["nbits"] + 1, where
                if g["m"] > 1:
                    assert (1 << g["nbits"]) >= g["m"] > (1 << (g["nbits"] - 1)), where
                assert g["rows2"] == -(-g["m"] // (1 << g["d2"])), where
                assert g["npairs"] == (1 if shared else W) * g["Q"], where


def test_hook_rejects_bad_arguments():
    out = (C.c_uint32 * 12)()
    T = _lib.test_lib()
    assert T.ark_hip_test_msm_reduce_geometry(5, 12, 22, 9, 0, 0, out) != 0
    assert T.ark_hip_test_msm_reduce_geometry(1, 12, 22, 23, 0, 0, out) != 0
    assert T.ark_hip_test_msm_reduce_geometry(1, 12, 22, 9, 0, 0, None) != 0


def test_window_plan_is_the_recorded_one():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msm_plan_cells.json")) as f:
        cells = json.load(f)
    for key, prepared in (("plain", False), ("prepared", True)):
        for curve in CURVES:
            got = [list(A.msm_plan(curve, 1 << lg, prepared)) for lg in cells["log_n"]]
            assert got == cells[key][curve], (key, curve)
