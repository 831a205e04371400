"""The sumcheck round on the device (ark_hip_sumcheck_round_device) through the Python mirror, limb for limb against the
big-integer model of tests/sumcheck_ref.py -- never against the code under test.  Outputs are canonical Montgomery residues:
no tolerance anywhere.  The model works on canonical values (a product is not linear in R): tables are decoded from their
Montgomery limbs, results encoded."""
import ctypes as C
import functools

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd._lib import lib
import mle_ref
import oracle_lib as O
import pyref
import sumcheck_ref as S

pytestmark = pytest.mark.gpu

FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
MLE = A.DenseMultilinearExtension
NT = 8                                # tables of a set: the most one call takes


def modulus(fname):
    return pyref.MODULI[fname][0]


@functools.lru_cache(maxsize=None)
def tables(fname, m):
    """eight tables of 2^m random elements with zeros, the residue p - 1 and the value -1 planted; uploaded once, cached with
    their canonical integers and never written to.  -> (device extensions, Montgomery limbs, canonical integers)"""
    fid, p = O.FID[fname], modulus(fname)
    n = 1 << m
    out = []
    for k in range(NT):
        a = O.gen_scalars(fid, 1700 + 16 * m + k, n, montgomery=True).copy()
        a[(k + 1) % n] = 0
        if n >= 4:
            a[(2 * k + 2) % n] = pyref.to_limbs(p - 1, 4)         # the largest residue
            a[(n - 1 - k) % n] = pyref.to_mont(p - 1, p)          # the value -1
        if n >= 1024:
            a[510 + k:514 + k:2] = 0                              # around the seam of the first two workgroups
        a.setflags(write=False)
        out.append(a)
    return tuple(MLE.from_evaluations(fname, m, a) for a in out), tuple(out), tuple(tuple(S.decode(a, p)) for a in out)


def coefficient(kind, fname, seed):
    """a canonical value: 0, 1, p - 1 or a seeded random one"""
    p = modulus(fname)
    if kind == "random":
        return pyref.from_mont(O.gen_scalars(O.FID[fname], 4000 + seed, 1, montgomery=True)[0], p)
    return {"0": 0, "1": 1, "p-1": p - 1}[kind]


# name -> (tables used, [(coefficient kind, table indices)])
SHAPES = {
    "lone": (1, [("random", [0])]),
    "ab": (2, [("1", [0, 1])]),
    "aab": (2, [("random", [0, 0, 1])]),
    "four": (4, [("p-1", [0, 1, 2, 3])]),
    "two_terms": (4, [("1", [0, 1, 2]), ("random", [0, 3])]),
    "eight_terms": (4, [("0", [0, 1]), ("1", [1, 2, 3]), ("p-1", [0]), ("random", [3, 3]), ("random", [0, 1, 2, 3]), ("1", [2]),
                        ("p-1", [1, 0, 1]), ("random", [2, 0])]),
    "eight_tables": (8, [("1", [0, 1, 2, 3]), ("random", [4, 5, 6, 7]), ("p-1", [7, 0]), ("random", [5])]),
}
CHALLENGES = ["0", "1", "p-1", "random"]


def terms_of(shape, fname):
    nt, kinds = SHAPES[shape]
    return nt, [(coefficient(kind, fname, 10 * len(ix) + j), ix) for j, (kind, ix) in enumerate(kinds)]


def make_list(fname, m, mles, terms):
    p = modulus(fname)
    lp = A.ListOfProducts(fname, m)
    for c, ix in terms:
        lp.add_product([mles[k] for k in ix], pyref.to_mont(c, p))
    return lp


def test_the_mirror_refuses_what_does_not_fit():
    fname = "BLS12_381_FR"
    mles, _, _ = tables(fname, 3)
    one = pyref.to_mont(1, modulus(fname))
    lp = A.ListOfProducts(fname, 3)
    with pytest.raises(ValueError):
        lp.round()                                                # no products
    with pytest.raises(ValueError):
        lp.add_product([], one)
    with pytest.raises(ValueError):
        lp.add_product([mles[0]] * 5, one)
    with pytest.raises(ValueError):
        lp.add_product([tables(fname, 2)[0][0]], one)             # a wrong num_vars
    with pytest.raises(ValueError):
        lp.add_product([tables("BN254_FR", 3)[0][0]], one)        # a wrong field
    lp.add_product([mles[0], mles[1], mles[0]], one)
    assert len(lp.tables) == 2 and lp.degree == 3                 # shared by identity
    full = A.ListOfProducts(fname, 3)
    full.add_product(list(mles[:4]), one)
    full.add_product(list(mles[4:]), one)
    extra = mles[0].clone()                                       # equal content, another object: a ninth table
    with pytest.raises(ValueError):
        full.add_product([extra], one)
    assert len(full.tables) == 8 and len(full.products) == 2
    for _ in range(6):
        full.add_product([mles[0]], one)
    with pytest.raises(ValueError):
        full.add_product([mles[0]], one)                          # a ninth product
    extra.free()


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("m", [1, 2, 3, 6, 7, 8, 9, 10, 12])
def test_plain_and_fused_rounds(fname, m):
    """m variables are summed over: one pair is m = 1, a wave 64 pairs (m = 7), a workgroup 256 pairs (m = 9), two workgroups
    and the second reduction stage from m = 10.  Plain rounds read the 2^m tables; fused rounds read the 2^(m+1) tables, bind
    a challenge, write 2^m tables and sum over those."""
    p = modulus(fname)
    mles, limbs, ints = tables(fname, m)
    big_mles, big_limbs, big_ints = tables(fname, m + 1)
    rnd = coefficient("random", fname, 77 + m)
    folded = {}                                                   # challenge kind -> (the model's bound tables, their limbs)
    for si, shape in enumerate(SHAPES):
        nt, terms = terms_of(shape, fname)
        want = S.encode(S.round_sums([list(t) for t in ints[:nt]], terms, p), p)
        lp = make_list(fname, m, mles, terms)
        got = lp.round()
        assert got.shape == (S.degree_of(terms) + 1, 4) and np.array_equal(got, want), (shape, "plain")
        assert np.array_equal(lp.round(), want), (shape, "plain, again")
        # fused: every challenge at the small sizes, one per shape (all four over the shapes) at the larger ones
        for kind in CHALLENGES if m <= 8 else [CHALLENGES[si % 4]]:
            r = rnd if kind == "random" else coefficient(kind, fname, 0)
            r_limbs = pyref.to_mont(r, p)
            if kind not in folded:
                model = [mle_ref.fix_variables(list(t), [r], p) for t in big_ints]
                model_limbs = [S.encode(t, p) for t in model]
                for k in range(NT):                               # the existing entry agrees with the model
                    fixed = big_mles[k].fix_variables(r_limbs.reshape(1, 4))
                    assert np.array_equal(fixed.to_evaluations(), model_limbs[k]), (kind, k, "fix_variables")
                    fixed.free()
                folded[kind] = (model, model_limbs)
            bound, bound_limbs = folded[kind][0][:nt], folded[kind][1][:nt]
            want = S.encode(S.round_sums(bound, terms, p), p)
            lp = make_list(fname, m + 1, big_mles, terms)
            got = lp.round(r_limbs)
            assert np.array_equal(got, want), (shape, kind, "fused: evaluations")
            out = lp.bound_tables()
            assert out.shape == (nt, 1 << m, 4)
            for k in range(nt):                                   # the model's fold, which fix_variables equals element for element
                assert np.array_equal(out[k], bound_limbs[k]), (shape, kind, k, "fused: the bound table")
            # the unfused chain gives the same
            lp2 = make_list(fname, m + 1, big_mles, terms)
            assert np.array_equal(lp2.round(r_limbs, fused=False), want), (shape, kind, "fix_variables, then a plain round")
            assert np.array_equal(lp2.bound_tables(), out)
            # the round after it reads the list's own tables
            if 2 <= m <= 8:
                r2 = (r * r + 5) % p
                twice = [mle_ref.fix_variables(t, [r2], p) for t in bound]
                assert np.array_equal(lp.round(pyref.to_mont(r2, p)), S.encode(S.round_sums(twice, terms, p), p)), (shape, kind, "second bind")
                assert np.array_equal(lp.bound_tables(), np.stack([S.encode(t, p) for t in twice]))
            lp.free()
            lp2.free()
    for k in range(NT):
        assert np.array_equal(mles[k].to_evaluations(), limbs[k]) and np.array_equal(big_mles[k].to_evaluations(), big_limbs[k]), "input changed"


@pytest.mark.parametrize("fname", FR)
def test_the_end_case(fname):
    """m = 0: the fused call on two-element tables writes the one-element tables f_k(r), reports sum_j c_j prod_k f_k(r) as
    evals[0] and zeros behind it; the plain call has nothing to sum and is refused"""
    p = modulus(fname)
    mles, limbs, ints = tables(fname, 1)
    for shape in SHAPES:
        nt, terms = terms_of(shape, fname)
        for kind in CHALLENGES:
            r = coefficient(kind, fname, 5)
            bound = [mle_ref.fix_variables(list(t), [r], p) for t in ints[:nt]]
            lp = make_list(fname, 1, mles, terms)
            got = lp.round(pyref.to_mont(r, p))
            want = S.final_round(bound, terms, p)
            assert want[1:] == [0] * S.degree_of(terms) and np.array_equal(got, S.encode(want, p)), (shape, kind)
            assert np.array_equal(lp.bound_tables()[:, 0, :], S.encode([t[0] for t in bound], p)), (shape, kind)
            with pytest.raises(ValueError):
                lp.round()
            lp.free()
    ptrs = (C.c_void_p * 1)(mles[0].evaluations.ptr.value)
    one = pyref.to_mont(1, p)
    ev = np.zeros((2, 4), dtype=np.uint64)
    args = ((C.c_uint * 1)(1), (C.c_uint * 1)(0), one.ctypes.data_as(C.c_void_p), 1)
    assert lib().ark_hip_sumcheck_round_device(mles[0].field, ptrs, 1, 0, *args, None, None, ev.ctypes.data_as(C.c_void_p)) == -1
    assert lib().ark_hip_sumcheck_round_device(mles[0].field, ptrs, 1, 0, *args, one.ctypes.data_as(C.c_void_p), ptrs,
                                               ev.ctypes.data_as(C.c_void_p)) == -1


# ---- every launch geometry: one and two reduction stages, one and several pairs per lane ---------------------------
PERIOD_LOG = 8
TWO = {f: min(nv for nv in range(1, 40) if A.sumcheck_plan(nv, fused=f)[2] == 2) for f in (False, True)}
MANY = {f: min(nv for nv in range(1, 40) if A.sumcheck_plan(nv, fused=f)[1] > 1) for f in (False, True)}
GEOMETRY_CASES = sorted({(f, nv + d) for f in (False, True) for nv in (TWO[f], MANY[f]) for d in (-1, 0, 1)})


def periodic_tables(fname, nv, count, seed):
    """count tables of 2^nv elements: a base block of 2^8 repeated, with cells planted in the first pair and the last, on both
    sides of a workgroup seam (of the plain round and of the fused one), in the middle, and in pairs only the grid-stride
    tail reaches.  -> (numpy limbs per table, Periodic models)"""
    fid, p = O.FID[fname], modulus(fname)
    n = 1 << nv
    s = min(PERIOD_LOG, nv)
    spots = [0, 1, 2, 3, n - 1, n - 2, n - 4, 510, 511, 512, 513, 1022, 1023, 1024, 1025, n // 2 - 1, n // 2, n // 2 + 1]
    for blocks_log in (18, 19):                                   # pair 2^18 of a plain round, row 2^18 of a fused one, and neighbours
        spots += [(1 << blocks_log) * 2 - 1, (1 << blocks_log) * 2, (1 << blocks_log) * 2 + 5, (1 << blocks_log) * 3 + 2]
    spots = sorted({i for i in spots if 0 <= i < n})
    arrays, models = [], []
    for k in range(count):
        base = O.gen_scalars(fid, seed + k, 1 << s, montgomery=True)
        a = np.tile(base, (n >> s, 1))
        cells = {}
        for q, i in enumerate(spots[k % 2::2] if k else spots):  # table 0 has every spot, the others every second one
            v = (0, p - 1, (q * 0x9E3779B97F4A7C15 + k) % p)[q % 3]
            cells[i] = v
            a[i] = pyref.to_mont(v, p)
        arrays.append(a)
        models.append(S.Periodic(nv, S.decode(base, p), cells))
    return arrays, models


def periodic_limbs(t, p):
    """the numpy table of a Periodic model"""
    a = np.tile(S.encode(t.base, p), ((1 << t.m) // len(t.base), 1))
    for i, v in t.cells.items():
        a[i] = pyref.to_mont(v, p)
    return a


def test_the_geometry_cases_cover_every_variant():
    seen = {(f, A.sumcheck_plan(nv, fused=f)[2], A.sumcheck_plan(nv, fused=f)[1] > 1) for f, nv in GEOMETRY_CASES}
    for f in (False, True):
        assert {(f, 1, False), (f, 2, False), (f, 2, True)} <= seen, seen
        assert TWO[f] < MANY[f] <= 24
        blocks, ppl, _ = A.sumcheck_plan(MANY[f] + 1, fused=f)
        assert ppl >= 2 and blocks * 256 == 1 << 18, "the planted cells behind row 2^18 sit in the grid-stride tail"


@pytest.mark.parametrize("fused,nv", GEOMETRY_CASES)
def test_every_geometry(fused, nv):
    fname = "BLS12_381_FR"
    p = modulus(fname)
    # three tables run the four-table kernel; five tables, at the sizes where a lane walks several pairs, the eight-table one
    cases = [(3, [("1", [0, 1, 2]), ("random", [1, 1])])]
    if nv in (TWO[fused], MANY[fused]):
        cases.append((5, [("random", [0, 1, 2, 3]), ("p-1", [4, 0]), ("1", [3])]))
    arrays, models = periodic_tables(fname, nv, max(nt for nt, _ in cases), 300 + nv)
    mles = [MLE.from_evaluations(fname, nv, a) for a in arrays]
    r = coefficient("random", fname, nv)
    for nt, kinds in cases:
        terms = [(coefficient(kind, fname, 3 + j), ix) for j, (kind, ix) in enumerate(kinds)]
        lp = make_list(fname, nv, mles, terms)
        if not fused:
            assert np.array_equal(lp.round(), S.encode(S.round_sums(models[:nt], terms, p), p)), (nt, "plain")
        else:
            bound = S.bind(models[:nt], r, p)
            got = lp.round(pyref.to_mont(r, p))
            assert np.array_equal(got, S.encode(S.round_sums(bound, terms, p), p)), (nt, "fused: evaluations")
            out = lp.bound_tables()
            for k in range(nt):
                want = periodic_limbs(bound[k], p)
                assert np.array_equal(out[k], want), (nt, k, np.nonzero((out[k] != want).any(axis=1))[0][:5])
            fixed = mles[0].fix_variables(pyref.to_mont(r, p).reshape(1, 4))
            assert np.array_equal(fixed.to_evaluations(), out[0]), "the bound table against fix_variables"
            fixed.free()
        lp.free()
    for m, a in zip(mles, arrays):
        assert np.array_equal(m.to_evaluations(), a), "input changed"
        m.free()


# ---- the whole protocol ----------------------------------------------------------------------------------------------
def check_proof(fname, nv, mles, models, terms, proof, claim, walked):
    p = modulus(fname)
    _, model_challenge = S.hash_challenge(p)
    rounds, point, finals, final_value = S.prove(models, terms, model_challenge, p)
    assert len(proof.rounds) == nv and proof.point.shape == (nv, 4)
    for i in range(nv):
        assert np.array_equal(proof.rounds[i], S.encode(rounds[i], p)), ("round", i)
        assert np.array_equal(proof.point[i], pyref.to_mont(point[i], p)), ("challenge", i)
    assert np.array_equal(proof.final_evaluations, S.encode(finals, p)), "per-table final values"
    assert np.array_equal(proof.final_value, pyref.to_mont(final_value, p)), "final value"
    got_rounds = [S.decode(g, p) for g in proof.rounds]
    got_point = S.decode(proof.point, p)
    got_finals = S.decode(proof.final_evaluations, p)
    if walked:
        assert S.verify_tables(claim, got_rounds, got_point, models, terms, p), "the verifier, f_k(point) from mle_ref.evaluate"
    assert S.verify(claim, got_rounds, got_point, got_finals, terms, p), "the verifier on the device's transcript"
    assert S.interpolate(got_rounds[-1], got_point[-1], p) == S.decode(proof.final_value.reshape(1, 4), p)[0]
    for k, m in enumerate(mles):
        assert np.array_equal(m.evaluate(proof.point), proof.final_evaluations[k]), (k, "final value against evaluate at the point")


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("nv", [10, 12])
def test_prove(fname, nv):
    p = modulus(fname)
    mles, limbs, ints = tables(fname, nv)
    device_challenge, _ = S.hash_challenge(p)
    for shape in ("two_terms", "eight_tables") if nv == 10 else ("aab",):
        nt, terms = terms_of(shape, fname)
        models = [list(t) for t in ints[:nt]]
        claim = 0                                                 # the sum over the whole cube, from the definition
        for c, ix in terms:
            for i in range(1 << nv):
                pr = c
                for k in ix:
                    pr = pr * models[k][i] % p
                claim += pr
        claim %= p
        lp = make_list(fname, nv, mles, terms)
        proof = lp.prove(device_challenge)
        check_proof(fname, nv, mles[:nt], models, terms, proof, claim, True)
        lp.free()
        if nv == 10:                                              # binding with the fold kernel gives the same transcript
            lp = make_list(fname, nv, mles, terms)
            other = lp.prove(device_challenge, fused=False)
            assert all(np.array_equal(a, b) for a, b in zip(other.rounds, proof.rounds)) and np.array_equal(other.final_value, proof.final_value)
            assert np.array_equal(other.final_evaluations, proof.final_evaluations)
            with pytest.raises(ValueError):
                lp.prove(device_challenge)                        # a list is proved once
            lp.free()
    for k in range(NT):
        assert np.array_equal(mles[k].to_evaluations(), limbs[k]), "the caller's tables changed"


@pytest.mark.parametrize("nv", [TWO[True], MANY[True]])
def test_prove_on_periodic_tables(nv):
    """the sizes where the second reduction stage and the grid-stride loop begin, on tables no model could walk"""
    fname = "BLS12_381_FR"
    p = modulus(fname)
    arrays, models = periodic_tables(fname, nv, 3, 900 + nv)
    mles = [MLE.from_evaluations(fname, nv, a) for a in arrays]
    terms = [(1, [0, 1, 2]), (coefficient("random", fname, 9), [2, 0])]
    g = S.round_sums(models, terms, p)
    lp = make_list(fname, nv, mles, terms)
    proof = lp.prove(S.hash_challenge(p)[0])
    check_proof(fname, nv, mles, models, terms, proof, (g[0] + g[1]) % p, False)
    lp.free()
    for m, a in zip(mles, arrays):
        assert np.array_equal(m.to_evaluations(), a), "the caller's tables changed"
        m.free()


def test_a_small_round_after_a_large_one():
    """the partial sums of a two-stage round stay in the library's scratch: a one-stage round after it must not read them"""
    fname = "BLS12_381_FR"
    p = modulus(fname)
    nt, terms = terms_of("two_terms", fname)
    big, small = 14, 3
    assert A.sumcheck_plan(big)[2] == 2 and A.sumcheck_plan(small)[2] == 1 and A.sumcheck_plan(11)[0] < A.sumcheck_plan(big)[0]
    want = {m: S.encode(S.round_sums([list(t) for t in tables(fname, m)[2][:nt]], terms, p), p) for m in (small, 11)}
    for m in (big, 11, small, big, small):
        lp = make_list(fname, m, tables(fname, m)[0], terms)
        got = lp.round()
        if m in want:
            assert np.array_equal(got, want[m]), m
        r = pyref.to_mont(coefficient("random", fname, m), p)
        lp.round(r)
        lp.free()
    # ... nor a round of lower degree the higher evaluations of the one before
    lp = make_list(fname, small, tables(fname, small)[0], terms_of("lone", fname)[1])
    assert np.array_equal(lp.round(), S.encode(S.round_sums([list(tables(fname, small)[2][0])], terms_of("lone", fname)[1], p), p))
