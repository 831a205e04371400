"""CPU-side pieces of the FFT plan tests (tests/test_gpu_fft_plans.py), pinned without a GPU:
  * the closed form of the transform of a geometric input (pyref.geometric_fft) -- the reference that scales past the
    oracle, up to each field's two-adicity -- against the oracle's transform and its direct evaluation, in Montgomery
    limbs and the reference's index order: forward, inverse, coset both ways, degree-aware lengths;
  * the Python restatement of the pass planner (pyref.fft_plan) on the table of default stage counts, the knobs and the
    rules the device planner follows (csrc/fft.cuh, fft_run_device)."""
import numpy as np
import pytest

import oracle_lib as O
import pyref as P

FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]


def geometric(field, n, a, b, count=None):
    """x_i = a b^i for i < count, zero beyond: Montgomery limbs [n, 4]"""
    p = P.MODULI[field][0]
    x = np.zeros((n, 4), dtype=np.uint64)
    v = a
    for i in range(n if count is None else count):
        x[i] = P.to_mont(v, p)
        v = v * b % p
    return x


def enc(field, vals):
    p = P.MODULI[field][0]
    return np.stack([P.to_mont(v, p) for v in vals])


def ratio(field, seed):
    p = P.MODULI[field][0]
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % p for _ in range(3)]   # a, b, coset offset h


@pytest.mark.parametrize("field", FR)
def test_closed_form_matches_oracle_transform(field):
    fid = O.FID[field]
    p = P.MODULI[field][0]
    for log_n in range(1, 13):
        n = 1 << log_n
        a, b, h = ratio(field, 10 * log_n + fid)
        x = geometric(field, n, a, b)
        hm = P.to_mont(h, p)
        js = range(n)
        for off, om in ((1, None), (h, hm)):
            for inverse in (False, True):
                exp = O.fft(fid, x, log_n, om, inverse, 2).reshape(n, 4)
                got = enc(field, P.geometric_fft(field, log_n, a, b, js, off, inverse))
                assert np.array_equal(got, exp), (field, log_n, off != 1, inverse)
        # sampled indices of a larger input: the same values as the full transform at those positions
        js = P.sample_indices(log_n, extra=8, seed=log_n)
        exp = O.fft(fid, x, log_n, None, False, 2).reshape(n, 4)[js]
        assert np.array_equal(enc(field, P.geometric_fft(field, log_n, a, b, js)), exp)


@pytest.mark.parametrize("field", FR)
def test_closed_form_degree_aware_matches_direct_evaluation(field):
    fid = O.FID[field]
    p = P.MODULI[field][0]
    for log_n, count in [(1, 1), (2, 1), (4, 3), (6, 16), (8, 33), (9, 2), (10, 200), (12, 1024), (12, 700)]:
        n = 1 << log_n
        a, b, h = ratio(field, 1000 + 7 * log_n + count)
        x = geometric(field, count, a, b)
        for off in (1, h):
            om = None if off == 1 else P.to_mont(off, p)
            exp = O.dft_naive(fid, x, log_n, om).reshape(n, 4)
            got = enc(field, P.geometric_fft(field, log_n, a, b, range(n), off, num_coeffs=count))
            assert np.array_equal(got, exp), (field, log_n, count, off != 1)
        # and the oracle's FFT of the zero-extended input
        exp = O.fft(fid, np.concatenate([x, np.zeros((n - count, 4), dtype=np.uint64)]), log_n, None, False, 2)
        assert np.array_equal(enc(field, P.geometric_fft(field, log_n, a, b, range(n), num_coeffs=count)),
                              exp.reshape(n, 4))


def test_sample_indices_cover_the_edges():
    for log_n in (1, 2, 12, 28):
        n = 1 << log_n
        s = set(P.sample_indices(log_n, extra=50).tolist())
        assert {0, 1, n - 1, n >> 1} <= s and all(0 <= j < n for j in s)
        assert all((1 << m) in s or (1 << m) == n for m in range(log_n + 1))
        assert all((1 << m) - 1 in s for m in range(log_n + 1))
        if log_n >= 2:
            assert {(n >> 1) - 1, (n >> 1) + 1} <= s


# the default plans for k = 11 .. 28, as the device planner builds them: P = ceil(k / 8) passes, odd pairs trade a stage,
# up to three passes sorted short-first, four passes left longest-first
DEFAULT_PLANS = {
    11: [5, 6], 12: [6, 6], 13: [6, 7], 14: [6, 8], 15: [7, 8], 16: [8, 8],
    17: [5, 6, 6], 18: [6, 6, 6], 19: [6, 6, 7], 20: [6, 6, 8], 21: [6, 7, 8], 22: [6, 8, 8], 23: [7, 8, 8], 24: [8, 8, 8],
    25: [7, 6, 6, 6], 26: [8, 6, 6, 6], 27: [8, 7, 6, 6], 28: [8, 8, 6, 6],
}


def test_planner_restatement_default_table():
    for k, kps in DEFAULT_PLANS.items():
        assert P.fft_plan(k) == kps, k
        assert sum(kps) == k and max(kps) <= 8
    for k in range(0, 11):
        assert P.fft_plan(k) == [k] and P.fft_plan(k, zlog=max(k - 1, 0)) == [k]   # one workgroup, zero-filled tail


def test_planner_restatement_degree_aware():
    # only the k - zlog executed stages are planned
    assert P.fft_plan(15, 7) == [8]            # one executed pass with k > 10: into the ping buffer, copied back
    assert P.fft_plan(18, 10) == [8]
    assert P.fft_plan(24, 3) == P.fft_plan(21)
    assert P.fft_plan(26, 2) == [8, 8, 8]
    assert P.fft_plan(26, 1) == [7, 6, 6, 6]
    assert P.fft_plan(28, 20) == [8] and P.fft_plan(28, 19) == [4, 5]


def test_planner_restatement_knobs():
    # ARK_HIP_FFT_KP: at most kp stages per pass
    assert P.fft_plan(16, kp=5) == [4, 4, 4, 4] and P.fft_plan(16, kp=6) == [4, 6, 6] == P.fft_plan(16, kp=7)
    assert P.fft_plan(20, kp=5) == [5, 5, 5, 5] and P.fft_plan(20, kp=7) == [6, 7, 7]
    assert P.fft_plan(16, kp=4) == P.fft_plan(16) == P.fft_plan(16, kp=9)   # out of range: ignored
    # ARK_HIP_FFT_TILE_LOG: tile_log - 1 stages per pass; the carry-free kernel keeps 1024-element tiles
    assert P.fft_plan(22, tile_log=11) == [6, 8, 8] and P.fft_plan(22, tile_log=12) == [11, 11]
    assert P.fft_plan(16, tile_log=11) == [8, 8] and P.fft_plan(17, tile_log=12) == [8, 9]
    assert P.fft_plan(25, tile_log=11) == [8, 8, 9] == P.fft_plan(25, tile_log=12)
    assert P.fft_plan(12, tile_log=11) == [6, 6] and P.fft_plan(11, tile_log=12) == [11]
    assert P.fft_plan(22, tile_log=12, carry_free=True) == P.fft_plan(22)
    assert P.fft_plan(22, tile_log=9) == P.fft_plan(22) == P.fft_plan(22, tile_log=13)
    # ARK_HIP_FFT_BALANCED: no odd-pair trade
    assert P.fft_plan(21, balanced=True) == [7, 7, 7] and P.fft_plan(20, balanced=True) == [6, 7, 7]
    # ARK_HIP_FFT_ASCENDING=0: longest first
    assert P.fft_plan(20, ascending=False) == [8, 6, 6] and P.fft_plan(21, ascending=False) == [8, 7, 6]
    # ARK_HIP_FFT_PLAN: taken only when it adds up to the executed stages and fits the tile; otherwise dropped
    assert P.fft_plan(14, plan=[1, 3, 10]) == [1, 3, 10]
    assert P.fft_plan(14, plan=[1, 3, 9]) == P.fft_plan(14)
    assert P.fft_plan(14, plan=[11, 3]) == P.fft_plan(14)
    assert P.fft_plan(14, plan=[0, 4, 10]) == P.fft_plan(14)
    assert P.fft_plan(16, plan=[2] * 8) == [2] * 8 and P.fft_plan(18, plan=[2] * 9) == P.fft_plan(18)
    assert P.fft_plan(16, 3, plan=[5, 8]) == [5, 8] and P.fft_plan(16, 3, plan=[8, 8]) == P.fft_plan(13)
