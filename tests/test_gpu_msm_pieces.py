"""Streamed MSM pieces, bucket by bucket: ark_hip_test_msm_pieces (csrc/msm_piece_dump.cuh) runs one MSM as explicit pieces
through the msm_enqueue / msm_finish the host-pointer entry runs, and copies out the whole bucket array and the counter words
behind every piece.  tests/msm_bucket_ref.py checks every cell against [sum of +-k_i] G (no tolerance anywhere) and names the
piece, window and bucket that is wrong; tests/msm_piece_cases.py builds inputs that put a doubling, a cancellation, an identity,
an empty piece and a heavy / light switch on a piece boundary -- the `accum` branches of the accumulate and heavy-combine kernels.
tests/test_msm_bucket_host.py shows without a GPU that each case reaches its regime and that the checker rejects a wrong bucket.
The saturated kernels run through lazy = 0 in the hook's knob record (MsmKnobs::lazy reaches every kernel choice of a piece).
The API-level cases at the end go through ark_hip_msm_sw on host arrays, where pieces alternate lanes and ring slots."""
import numpy as np
import pytest

import algebra_amd as A
import msm_bucket_ref as BR
import msm_piece_cases as PC
import msm_sort_ref as R
import oracle_lib as O
from algebra_amd._lib import ArkHipError

pytestmark = pytest.mark.gpu

CASES = PC.bucket_cases()
CURVE = "BLS12_381_G1"


def oracle_affine(inp, n=None):
    cid = inp.cr.cid
    return O.to_affine(cid, O.msm(cid, inp.bases[:n], inp.scalars[:n], O.SIGNED, 4, montgomery_scalars=bool(inp.mont))).reshape(-1)


def run_case(case, **over):
    """one hook call, every piece checked in full; returns (dump, model, regimes)"""
    d = BR.gpu_pieces(case.inp, **dict(case.knobs(), **over))
    assert d["rc"] == 0, d["rc"]
    h = d["header"]
    ref = BR.plan_header(case.inp.curve, case.c, case.inp.sizes)
    assert (h["c"], h["W"], h["narrow"], h["nbuckets"], h["npieces"]) == (ref["c"], ref["W"], ref["narrow"], ref["nbuckets"], ref["npieces"])
    assert h["pieces_run"] == h["npieces"] and h["bad_piece"] == BR.NO_PIECE and h["lazy"] == case.lazy
    assert [p["ngroups"] for p in h["pieces"]] == [1] * h["npieces"] and h["nbuckets"] < 32768
    m = case.model(h)
    regimes = BR.check_dump(d, m)
    assert np.array_equal(O.to_affine(case.inp.cr.cid, d["result"]).reshape(-1), oracle_affine(case.inp)), "the final point"
    return d, m, regimes


# ---- bucket-level cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_buckets_after_every_piece(case):
    d, m, regimes = run_case(case)
    for k, (items, runs, thr, flag) in enumerate(regimes):
        assert thr == (case.heavy or 64) and flag == 0
        if case.heavy_cells is not None:
            assert runs == len(case.heavy_cells[k]) and m.regime(k)[1] == case.heavy_cells[k]
        if case.runs is not None:
            assert (items, runs, thr) == case.runs[k]
        if k in case.empty:
            assert (items, runs) == (0, 0)
            if k:      # the lanes returned early and nothing re-encoded a bucket
                assert np.array_equal(d["buckets"][k], d["buckets"][k - 1]), "an empty piece changed the bucket array"
        if k in case.all_identity:
            assert (d["buckets"][k] == BR.identity_limbs(case.inp.cr)).all()
    if case.all_identity and case.all_identity[-1] == len(regimes) - 1:
        cr = case.inp.cr
        assert not np.any(O.to_affine(cr.cid, d["result"]))        # the result is the identity


def test_upper_half_of_narrow_windows_is_identity_from_the_first_piece_on():
    case = next(c for c in CASES if c.name == "baseline-BN254_G1-mont0")
    d = BR.gpu_pieces(case.inp, **case.knobs())
    m = case.model(d["header"])
    up = m.upper_half()
    assert d["header"]["narrow"] == 2 and up.sum() == 2 * 64
    for k in range(3):
        assert (d["buckets"][k][up] == BR.identity_limbs(case.inp.cr)).all(), k


def test_one_piece_equals_a_plain_call():
    import torch
    case = PC.alternating(CURVE, pieces=1)
    d, m, regimes = run_case(case)
    assert regimes[0][1] == 2
    bases = torch.from_numpy(case.inp.bases.view(np.int64)).cuda()
    scalars = torch.from_numpy(case.inp.scalars.view(np.int64)).cuda()
    plain = A.msm_bigint(case.inp.cr.cid, bases, scalars)
    assert np.array_equal(O.to_affine(case.inp.cr.cid, plain), O.to_affine(case.inp.cr.cid, d["result"]))
    # the same from device memory: the same points (not the same bytes -- the order inside a run is free, and with it ZZ)
    dd = BR.gpu_pieces(case.inp, bases=bases, scalars=scalars, **case.knobs())
    assert dd["rc"] == 0
    BR.check_dump(dd, m)
    assert np.array_equal(O.to_affine(case.inp.cr.cid, dd["result"]), O.to_affine(case.inp.cr.cid, d["result"]))


@pytest.mark.parametrize("piece", [0, 2])
def test_range_flag_names_the_piece(piece):
    case = PC.out_of_range(CURVE, piece)
    m0 = case.model()
    assert m0.out_of_range == [k == piece for k in range(3)]
    d = BR.gpu_pieces(case.inp, **case.knobs())
    h = d["header"]
    assert d["rc"] == BR.ERR_SCALAR_RANGE and h["bad_piece"] == piece and h["pieces_run"] == piece + 1
    m = case.model(h)
    assert len(d["buckets"]) == piece
    for k in range(piece):                        # the pieces in front of it ran and are right
        BR.check_hctr(d, m, k)
        BR.check_buckets(d, m, k)
    hctr, buckets = d["raw"]
    assert (hctr[16 * piece:] == 0xDEADBEEF).all() and (buckets[piece:] == 0xDEADBEEFDEADBEEF).all()   # nothing later was written
    good = PC.alternating(CURVE)                  # the same context, right away: no slot taken, nothing in flight
    run_case(good)


def test_a_piece_refuses_a_prepared_set_and_short_buffers():
    case = PC.lane_boundary(CURVE)
    d = BR.gpu_pieces(case.inp, prepared=1, **case.knobs())
    assert d["rc"] == BR.ERR_ARG
    for short in ((1, 0), (0, 8)):
        d = BR.gpu_pieces(case.inp, short_caps=short, **case.knobs())
        hctr, buckets = d["raw"]
        assert d["rc"] == BR.ERR_SIZE and (hctr == 0xDEADBEEF).all() and (buckets == 0xDEADBEEFDEADBEEF).all()
    run_case(case)


# ---- API-level cases: ark_hip_msm_sw on host arrays ------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def default_state():
    """Every test starts from the library's defaults (verified cache on with its default budget, nothing pinned)."""
    A.base_cache_config(-2, 0)
    A.base_cache_clear()
    yield
    A.base_cache_config(-2, 0)
    A.base_cache_clear()
    assert A.base_cache_stats()["pinned"] == 0, "a test leaked a pin"


_api_inputs = {}


def api_input(kind, pieces):
    """(Input, oracle's affine point), made once per (kind, pieces)"""
    key = (kind, pieces)
    if key not in _api_inputs:
        per = -(-720 // pieces)      # 720 points and more: a set below 64 KiB never enters the verified cache
        if kind == "two-valued":
            case = PC.two_valued(CURVE, max(720, 40 * pieces) + 3, pieces)
        elif kind == "alternating":
            case = PC.alternating(CURVE, pieces=pieces, background=max(11, per - 149), equal=True)
        elif kind == "cancelling":
            case = PC.cancelling(CURVE, True, n=max(100, per), pieces=pieces)
        else:
            case = PC.self_cancelling_pieces(CURVE, pieces, m=44)
        assert case.inp.bases.nbytes >= 64 << 10
        _api_inputs[key] = (case.inp, oracle_affine(case.inp))
    return _api_inputs[key]


def api_point(inp):
    return O.to_affine(inp.cr.cid, A.msm_bigint(inp.cr.cid, inp.bases, inp.scalars)).reshape(-1)


@pytest.mark.parametrize("pieces", [2, 3, 5, 16])
@pytest.mark.parametrize("kind", ["two-valued", "alternating", "cancelling"])
def test_api_pieces_under_every_cache_state(kind, pieces, monkeypatch):
    inp, want = api_input(kind, pieces)
    if kind != "two-valued":
        assert len(set(inp.sizes)) == 1 and len(inp.sizes) == pieces       # the entry's equal steps cut where the case does
    monkeypatch.setenv("ARK_HIP_STREAM_PIECES", str(pieces))
    monkeypatch.setenv("ARK_HIP_MSM_C", "6")
    A.base_cache_config(0, 0)                                   # cache off: the bases ring through with the scalars
    assert np.array_equal(api_point(inp), want), "cache off"
    A.base_cache_config(8 << 30, 0)                             # transparent cache: miss (fill), then the resident copy
    A.base_cache_clear()
    s0 = A.base_cache_stats()
    assert np.array_equal(api_point(inp), want), "miss"
    assert np.array_equal(api_point(inp), want), "hit"
    s1 = A.base_cache_stats()
    assert (s1["misses"] - s0["misses"], s1["hits"] - s0["hits"]) == (1, 1)
    with A.pin_bases(inp.cr.cid, inp.bases):
        assert np.array_equal(api_point(inp), want), "pinned"
    monkeypatch.setenv("ARK_HIP_MSM_HEAVY", "1024")             # no run is heavy any more: the lanes alone
    assert np.array_equal(api_point(inp), want), "heavy = 1024"


@pytest.mark.parametrize("kind", ["two-valued", "alternating", "cancelling", "self-cancelling"])
def test_api_seventeen_pieces_are_independent_msms(kind, monkeypatch):
    inp, want = api_input(kind, 17)
    monkeypatch.setenv("ARK_HIP_STREAM_PIECES", "17")
    monkeypatch.setenv("ARK_HIP_MSM_C", "6")
    for budget in (0, 8 << 30):
        A.base_cache_config(budget, 0)
        assert np.array_equal(api_point(inp), want), budget


@pytest.mark.parametrize("n", [1, 3])
def test_api_fewer_pairs_than_pieces(n, monkeypatch):
    inp, _ = api_input("two-valued", 5)
    monkeypatch.setenv("ARK_HIP_STREAM_PIECES", "5")
    cid = inp.cr.cid
    for budget in (0, 8 << 30):
        A.base_cache_config(budget, 0)
        got = O.to_affine(cid, A.msm_bigint(cid, inp.bases[:n].copy(), inp.scalars[:n].copy())).reshape(-1)
        assert np.array_equal(got, oracle_affine(inp, n)), (n, budget)


@pytest.mark.parametrize("where", ["first", "last"])
def test_api_out_of_range_scalar_in_a_piece(where, monkeypatch):
    inp, want = api_input("alternating", 4)
    monkeypatch.setenv("ARK_HIP_STREAM_PIECES", "4")
    monkeypatch.setenv("ARK_HIP_MSM_C", "6")
    cid, bits = inp.cr.cid, inp.cr.bits
    i = 5 if where == "first" else len(inp.logs) - 5
    bad = inp.scalars.copy()
    bad[i] = R.ints_to_limbs([1 << bits])[0]
    for pinned in (False, True):
        A.base_cache_config(0 if pinned else 8 << 30, 0)
        pin = A.pin_bases(cid, inp.bases) if pinned else None
        try:
            with pytest.raises(ArkHipError) as e:
                A.msm_bigint(cid, inp.bases, bad)
            assert e.value.code == BR.ERR_SCALAR_RANGE
            assert np.array_equal(api_point(inp), want), "the call after the refused one"
        finally:
            if pin is not None:
                pin.unpin()
        assert A.base_cache_stats()["pinned"] == 0
