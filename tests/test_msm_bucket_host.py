"""The reference and the checker of the streamed-piece bucket dumps (tests/msm_bucket_ref.py), without a GPU: the model folds to
the oracle's MSM for every input family of tests/test_gpu_msm_pieces.py on every curve; the checker rejects every single wrong
bucket a dump can hold and names piece, window and bucket; and every GPU case reaches the regime it is named for from the model
alone -- the heavy runs of every piece, their chunk items, the threshold, the pieces without a digit."""
import numpy as np
import pytest

import msm_bucket_ref as BR
import msm_piece_cases as PC
import msm_sort_ref as R
import oracle_lib as O
from msm_sort_ref import StageMismatch

CASES = PC.bucket_cases()
API_CASES = [PC.two_valued("BLS12_381_G1", 600, 3), PC.alternating("BLS12_381_G1", pieces=5, background=0),
             PC.cancelling("BLS12_381_G1", True, n=100, pieces=16, c=6)]


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = case.model()
        return cache[case.name]
    return get


def oracle_affine(inp):
    return O.to_affine(inp.cr.cid, O.msm(inp.cr.cid, inp.bases, inp.scalars, O.SIGNED, 4, montgomery_scalars=bool(inp.mont)))


# ---- the model folds to the oracle's MSM -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + API_CASES, ids=repr)
def test_fold_matches_oracle(case, models):
    m = models(case)
    assert not any(m.out_of_range)
    got = case.inp.cr.mul_gen([m.fold()])[0]
    assert np.array_equal(got, oracle_affine(case.inp).reshape(-1)), case.name


def test_fold_of_every_prefix():
    """behind piece k the model holds the MSM of pieces 0 .. k"""
    case = PC.heavy_boundary("BLS12_381_G1")
    m = case.model()
    for k, (lo, hi) in enumerate(case.inp.bounds()):
        part = BR.Input(case.inp.curve, case.inp.logs[:hi], R.scalars_to_ints(case.inp.scalars[:hi]), case.inp.sizes[:k + 1])
        assert np.array_equal(part.cr.mul_gen([m.fold(k)])[0], oracle_affine(part).reshape(-1)), k


# ---- every GPU case reaches its regime --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_regime_follows_from_the_model(case, models):
    m = models(case)
    h = m.h
    assert 5 <= h["c"] <= 8 and 1 <= len(case.inp.logs) <= 6000 and h["nbuckets"] < 32768
    for k in range(h["npieces"]):
        (items, runs, thr, flag), cells = m.regime(k)
        assert flag == 0
        assert thr == (case.heavy or 64)                      # few slots, few entries: the floor, unless forced
        if case.heavy_cells is not None:
            assert cells == case.heavy_cells[k], (k, cells)   # (window 0's cells are the bucket numbers themselves)
        if case.runs is not None:
            assert (items, runs, thr) == case.runs[k]
        if k in case.empty:
            assert m.counts[k].sum() == 0 and runs == 0
            if k:
                assert m.sums[k] == m.sums[k - 1]
        else:
            assert m.counts[k].sum() > 0
        assert (not any(m.sums[k])) == (k in case.all_identity), k
    if "baseline" in case.name:
        assert h["narrow"] >= 1 and case.inp.sizes == [1000, 1, 1501]


def test_named_regimes(models):
    by_name = {c.name: c for c in CASES}
    # runs of exactly 64 and 1024 stay with a lane / in one chunk, 65 and 1025 do not
    m = models(by_name["threshold-edges"])
    assert [int(m.counts[0][b]) for b in range(4)] == [64, 65, 1024, 1025]
    d = m.sort_dump(0)
    assert sorted(d["hlist"][0][:, 2].tolist()) == [1, 1, 2] and m.regime(0)[0][:3] == (4, 3, 64)
    assert models(by_name["threshold-edges-heavy1024"]).regime(0)[0][:3] == (2, 1, 1024)
    # the alternating cells: light -> heavy -> light, heavy -> light -> heavy, heavy throughout
    m = models(by_name["alternating-BLS12_381_G1-3"])
    over = [[bool(m.counts[k][b] > 64) for k in range(3)] for b in range(3)]
    assert over == [[False, True, False], [True, False, True], [True, True, True]]
    assert all(m.counts[k][b] > 0 for k in range(3) for b in range(3))
    # the boundaries: doubled and cancelled buckets behind piece 1
    m = models(by_name["lane-boundary-BLS12_381_G1"])
    r = m.inp.cr.r
    s0, s1 = m.sums[0], m.sums[1]
    assert s1[0] == 2 * s0[0] % r and s1[2] == 2 * s0[2] % r and s1[1] == 0 and s1[3] == 0 and s0[1] and s0[3]
    assert all(m.counts[1][b] == 1 for b in range(4)) and all(m.counts[1][b] == 2 for b in (4, 5, 6))
    assert all(m.sums[2][b] for b in range(7))
    m = models(by_name["heavy-boundary-BLS12_381_G1"])
    s0, s1 = m.sums[0], m.sums[1]
    assert s1[0] == 2 * s0[0] % r and s0[1] and s1[1] == 0 and s0[2] == 0 and s0[3] == 0 and s1[2] and s1[3]
    assert m.counts[0][2] == 0 and m.counts[0][3] == 2 and s1[4] == 9 * s0[4] % r
    # identity bases: a heavy run that sums to the identity, and a piece that changes nothing although it has digits
    m = models(by_name["identity-bases"])
    assert 0 in m.regime(0)[1] and m.counts[1].sum() > 0 and m.sums[1] == m.sums[0]
    # the cancelling inputs: lanes only / heavy runs
    assert models(by_name["cancelling-BLS12_381_G1-uniform-2"]).regime(1)[0][1] == 0
    m = models(by_name["cancelling-BLS12_381_G1-two-2"])
    assert m.regime(0)[0][1] >= m.h["W"] // 2 and m.regime(1)[0][1] == m.regime(0)[0][1]


def test_out_of_range_case_sets_the_model_flag():
    for piece in (0, 2):
        m = PC.out_of_range("BLS12_381_G1", piece).model()
        assert m.out_of_range == [k == piece for k in range(3)]


# ---- the checker rejects every single wrong bucket -------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["BLS12_381_G1", "BN254_G1", "BLS12_381_G2"])
def good(request):
    case = PC.lane_boundary(request.param)
    m = case.model()
    d = BR.encode_dump(m, seed=5)
    BR.check_dump(d, m)                                         # the CPU-made dump passes, decoded through a ZZ of its own
    return m, d


def mutated(d, k, cell, row):
    out = dict(d, buckets=[b.copy() for b in d["buckets"]])
    out["buckets"][k][cell] = row
    return out


def rejects(m, d, k, cell, text=None):
    w, b = m.where(cell)
    with pytest.raises(StageMismatch) as e:
        BR.check_dump(d, m)
    assert e.value.array == "buckets" and ("piece %d, window %d, bucket %d:" % (k, w, b)) in str(e.value), str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def test_checker_rejects_each_mutation(good):
    m, d = good
    cr = m.inp.cr
    fw = cr.fw
    k = 1
    filled = [c for c in range(m.h["nbuckets"]) if m.sums[k][c]]
    empty = [c for c in range(m.h["nbuckets"]) if not m.sums[k][c] and not m.upper_half()[c]]
    cell = filled[len(filled) // 2]
    row = d["buckets"][k][cell]
    for word in (0, fw + 1, 2 * fw, 4 * fw - 1):               # one limb flipped, in each coordinate
        bad = row.copy()
        bad[word] ^= np.uint64(1 << 7)
        rejects(m, mutated(d, k, cell, bad), k, cell)
    nb = next(c for c in filled if c + 1 in filled and m.sums[k][c] != m.sums[k][c + 1])   # swapped with its neighbour
    sw = mutated(d, k, nb, d["buckets"][k][nb + 1])
    sw["buckets"][k][nb + 1] = d["buckets"][k][nb]
    rejects(m, sw, k, nb, "not the model's point")
    rejects(m, mutated(d, k, empty[3], row), k, empty[3], "the model has the identity")         # identity -> point
    rejects(m, mutated(d, k, cell, BR.identity_limbs(cr)), k, cell, "holds the identity")      # point -> identity
    neg = row.copy()                                                                          # -S
    y = cr.F.dec(row[fw:2 * fw])
    neg[fw:2 * fw] = cr.F.enc(cr.F.neg(y))
    rejects(m, mutated(d, k, cell, neg), k, cell, "the negative of the model's point")
    for j in range(4):                                                                        # x + p: the same residue, not canonical
        big = row.copy()
        v = pyref_int(row[j * fw:j * fw + cr.nl]) + cr.p
        big[j * fw:j * fw + cr.nl] = int_limbs(v, cr.nl)
        rejects(m, mutated(d, k, cell, big), k, cell, "not canonical")
    weird = BR.identity_limbs(cr)                                                             # an identity that is not (1, 1, 0, 0)
    weird[0] ^= np.uint64(1)
    rejects(m, mutated(d, k, empty[0], weird), k, empty[0], "(1, 1, 0, 0)")
    changed = next(c for c in range(m.h["nbuckets"]) if m.sums[1][c] != m.sums[0][c] and m.sums[0][c] and m.sums[1][c])
    rejects(m, mutated(d, 1, changed, d["buckets"][0][changed]), 1, changed, "unchanged since piece 0")   # stale
    if m.h["narrow"]:
        up = int(np.flatnonzero(m.upper_half())[0])
        rejects(m, mutated(d, k, up, row), k, up, "upper half of a narrow window")


def test_checker_rejects_wrong_counters(good):
    m, d = good
    for word in range(4):
        bad = dict(d, hctr=[h.copy() for h in d["hctr"]])
        bad["hctr"][2][word] += 1
        with pytest.raises(StageMismatch) as e:
            BR.check_dump(bad, m)
        assert e.value.array == "hctr" and "piece 2" in str(e.value)


def pyref_int(limbs):
    return int.from_bytes(np.ascontiguousarray(limbs, dtype="<u8").tobytes(), "little")


def int_limbs(v, n):
    return np.frombuffer(v.to_bytes(8 * n, "little"), dtype="<u8")
