"""DenseMultilinearExtension on the device (ark_hip_mle_fix_variables_device, _evaluate_device, _relabel_device,
ark_hip_fr_axpy_device) through the Python mirror, limb for limb against the big-integer model of tests/mle_ref.py -- never
against the code under test.  Outputs are canonical Montgomery residues: no tolerance anywhere.

The tables stay Montgomery residues a R, used as the plain integers they are, and the POINT is converted to its canonical
value: the fold is linear in the table, so R rides along (tests/mle_ref.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd._lib import lib
import mle_ref
import oracle_lib as O
import pyref

pytestmark = pytest.mark.gpu

FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
MLE = A.DenseMultilinearExtension
W = A.mle_fold_plan(0, 0)[0]          # variables one launch binds: every seam below follows it
ints, limbs = mle_ref.ints, mle_ref.limbs


def enc(x, p):
    return pyref.to_mont(x % p, p)


def mont_ints(xs, p):
    r = pyref.R_of(p)
    return limbs([x % p * r % p for x in xs])


@functools.lru_cache(maxsize=None)
def table(fname, nv):
    """2^nv random elements with 0, the residue p - 1, the value -1 and zeros on both sides of a tile seam planted; cached
    together with its integers and never written to"""
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    n = 1 << nv
    a = O.gen_scalars(fid, 900 + nv, n, montgomery=True).copy()
    if n >= 8:
        a[1] = 0
        a[n // 2] = 0
        a[2] = pyref.to_limbs(p - 1, 4)               # the largest residue
        a[3] = enc(p - 1, p)                          # the value -1
    T = 1 << W
    if n >= 2 * T:
        a[T - 1] = pyref.to_limbs(p - 1, 4)           # the two sides of a tile seam
        a[T] = 0
        a[T - 3:T - 1] = 0
        a[T + 1:T + 3] = 0
        a[n - T - 2:n - T + 2] = 0
    a.setflags(write=False)
    return a, tuple(ints(a))


def points(fname, count, seed):
    """[(label, Montgomery limbs [count, 4], canonical integers)]: all 0, all 1 (both select table entries), all p - 1,
    random, and random with 0 / 1 mixed in"""
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    rnd = ints(O.gen_scalars(fid, seed, max(count, 1), montgomery=True))[:count]     # canonical residues: random values < p
    mixed = [(0, 1, x)[i % 3] for i, x in enumerate(rnd)]
    out = []
    for label, vals in (("0", [0] * count), ("1", [1] * count), ("p-1", [p - 1] * count), ("random", rnd), ("mixed", mixed)):
        out.append((label, mont_ints(vals, p).reshape(-1, 4), vals))
    return out


def test_documented_answers():
    """dense.rs:49-56, :211-221, :448-458 and the concat example :113-132, on the device"""
    fname = "BLS12_381_FR"
    p = pyref.MODULI[fname][0]
    m = MLE.from_evaluations(fname, 2, mont_ints([0, 0, 1, 0], p))
    assert np.array_equal(m.evaluate(mont_ints([-2, 17], p)), enc(51, p))
    m = MLE.from_evaluations(fname, 2, mont_ints([0, 1, 2, 6], p))
    bound = m.fix_variables(mont_ints([5], p))
    assert bound.num_vars == 1 and np.array_equal(bound.to_evaluations(), mont_ints([5, 22], p))
    f1 = MLE.from_evaluations(fname, 2, mont_ints([2, 3, 2, 6], p))
    assert np.array_equal(f1.evaluate(mont_ints([1, 17], p)), enc(54, p))
    f2 = MLE.from_evaluations(fname, 2, mont_ints([0, 0, 0, 1], p))
    f3 = MLE.concat([f1, f2])
    assert f3.num_vars == 3 and np.array_equal(f3.to_evaluations(), mont_ints([2, 3, 2, 6, 0, 0, 0, 1], p))
    e1, e2 = mle_ref.evaluate([2, 3, 2, 6], [1, 17], p), mle_ref.evaluate([0, 0, 0, 1], [1, 17], p)
    assert np.array_equal(f3.evaluate(mont_ints([1, 17, 3], p)), enc((1 - 3) * e1 + 3 * e2, p))
    # unequal lengths: zero fill up to the next power of two (dense.rs:628-647)
    one = MLE.from_evaluations(fname, 0, mont_ints([7], p))
    c = MLE.concat([f1, one])
    assert c.num_vars == 3 and np.array_equal(c.to_evaluations(), mont_ints([2, 3, 2, 6, 7, 0, 0, 0], p))
    with pytest.raises(ValueError):
        MLE.from_evaluations(fname, 2, mont_ints([1, 2, 3], p))
    with pytest.raises(ValueError):
        f1.evaluate(mont_ints([1], p))
    with pytest.raises(ValueError):
        f1.fix_variables(mont_ints([1, 2, 3], p))


NVS = sorted({0, 1, 2, 3, 4, W - 1, W, W + 1, W + 2, 16, 20})


def dims(nv):
    return sorted({d for d in (0, 1, 2, 3, W - 1, W, W + 1, nv - 1, nv) if 0 <= d <= nv})


def test_the_cases_sit_on_the_plans_seams():
    assert A.mle_fold_plan(W, W)[1] == [W] and len(A.mle_fold_plan(W + 1, W + 1)[1]) == 2
    assert len(A.mle_fold_plan(2 * W, 2 * W)[1]) == 2 and len(A.mle_fold_plan(2 * W + 1, 2 * W + 1)[1]) == 3
    assert {W - 1, W, W + 1} <= set(dims(20)) and {W, W + 1, W + 2} <= set(NVS)


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("nv", NVS)
def test_fix_variables_and_evaluate(fname, nv):
    p = pyref.MODULI[fname][0]
    a, am = table(fname, nv)
    m = MLE.from_evaluations(fname, nv, a)
    pts = points(fname, nv, 7 + nv)
    if nv >= 18:                                       # the model takes over a second per full fold there: the random point,
        for label, pt, _ in pts[:2]:                   # and the two points that SELECT entries, which need no model
            pick = 0 if label == "0" else -1
            assert np.array_equal(m.evaluate(pt), a[pick]), (label, "evaluate")
            for d in dims(nv):
                out = m.fix_variables(pt[:d])
                got = out.to_evaluations()
                assert np.array_equal(got, a[pick % (1 << d)::1 << d]), (label, d)
                out.free()
        pts = pts[3:4]
    for label, pt, ptc in pts:
        folds = {0: list(am)}                          # the model once per point: every dim is a prefix of the full fold
        for d in range(1, nv + 1):
            folds[d] = mle_ref.fix_variables(folds[d - 1], ptc[d - 1:d], p)
        want_value = pyref.to_limbs(folds[nv][0], 4)
        if label == "0":
            assert folds[nv][0] == am[0]
        if label == "1":
            assert folds[nv][0] == am[-1]
        ev = m.evaluate(pt)
        assert np.array_equal(ev, want_value), (label, "evaluate")
        for d in dims(nv):
            out = m.fix_variables(pt[:d])
            assert out.num_vars == nv - d and len(out) == 1 << (nv - d)
            got, want = out.to_evaluations(), (limbs(folds[d]) if d else a)
            assert np.array_equal(got, want), (label, d, np.nonzero((got != want).any(axis=1))[0][:5])
            if d == nv:
                assert np.array_equal(got[0], ev), (label, "evaluate == fix_variables(point)[0]")
            out.free()
        assert np.array_equal(m.to_evaluations(), a), (label, "input changed")
    m.free()


LO = W + 1                            # low variables of the block construction below


def block_table(nv, seed):
    """A 2^nv table that needs no 2^nv-step model: four random base blocks g_0..g_3 of 2^LO elements, block h of the table
    being g_{c[h]} for a random map c, plus a few planted single elements (0, the residue p - 1, random) at and around the
    block, tile and table boundaries.  -> (table, the base blocks as integers, c, {index: (what the block construction has
    there, what is there now)})"""
    fid, p = O.FID["BLS12_381_FR"], pyref.MODULI["BLS12_381_FR"][0]
    rng = np.random.default_rng(seed)
    g = O.gen_scalars(fid, 77, 4 << LO, montgomery=True).reshape(4, 1 << LO, 4)
    gm = [ints(g[q]) for q in range(4)]
    c = rng.integers(0, 4, size=1 << (nv - LO))
    c[:4] = [0, 1, 2, 3]
    a = g[c].reshape(-1, 4).copy()                      # [2^(nv-LO), 2^LO, 4] -> the table
    planted = {}
    for idx in [0, 1, (1 << LO) - 1, 1 << LO, (1 << W) - 1, 1 << W, (1 << nv) - 1, (1 << (nv - 1)) + 5] + \
            [int(v) for v in rng.integers(0, 1 << nv, size=6)]:
        old = pyref.from_limbs(a[idx])
        new = (0, p - 1, int.from_bytes(rng.bytes(40), "little") % p)[len(planted) % 3]
        a[idx] = pyref.to_limbs(new, 4)
        planted[idx] = (planted.get(idx, (old, None))[0], new)
    return a, gm, c, planted


def block_fold(gm, c, planted, ptc, d, p):
    """fix_variables(ptc[:d]) of a block_table for d <= LO, as numpy limbs: every base block folded over the d variables
    (4 * 2^LO steps of big-integer work), laid out by c, and each planted element's delta * eq(low index, r) added to the one
    output element it reaches"""
    assert d <= LO
    r = ptc[:d]
    fb = np.stack([limbs(mle_ref.fix_variables(gm[q], r, p)) for q in range(4)])     # [4, 2^(LO-d), 4]
    want = fb[c].reshape(-1, 4).copy()
    delta = {}
    for idx, (old, new) in planted.items():
        o = idx >> d
        delta[o] = (delta.get(o, 0) + (new - old) * mle_ref.eq(idx & ((1 << d) - 1), r, p)) % p
    for o, dv in delta.items():
        want[o] = pyref.to_limbs((pyref.from_limbs(want[o]) + dv) % p, 4)
    return want


@pytest.mark.parametrize("nv", [2 * W, 2 * W + 1])
def test_three_launches(nv):
    """nv = 2W (two full launches) and 2W + 1 (three) on a block_table: with LO = W + 1 low variables bound, row h of what is
    left is g_{c[h]}(r_low) plus the planted elements' shares, and the value is the fold of the rows over the high variables."""
    fname = "BLS12_381_FR"
    p = pyref.MODULI[fname][0]
    assert len(A.mle_fold_plan(nv, nv)[1]) == (2 if nv == 2 * W else 3)
    a, gm, c, planted = block_table(nv, 31 + nv)
    m = MLE.from_evaluations(fname, nv, a)
    for label, pt, ptc in points(fname, nv, 3 + nv)[2:]:
        want = block_fold(gm, c, planted, ptc, LO, p)
        part = m.fix_variables(pt[:LO])
        got = part.to_evaluations()
        assert part.num_vars == nv - LO and np.array_equal(got, want), (label, np.nonzero((got != want).any(axis=1))[0][:5])
        value = pyref.to_limbs(mle_ref.evaluate(ints(want), ptc[LO:], p), 4)
        assert np.array_equal(m.evaluate(pt), value), (label, "evaluate")
        assert np.array_equal(part.evaluate(pt[LO:]), value), (label, "evaluate after fix_variables")
        full = m.fix_variables(pt)
        assert full.num_vars == 0 and np.array_equal(full.to_evaluations()[0], value), (label, "fix_variables(point)")
        part.free()
        full.free()
    assert np.array_equal(m.to_evaluations(), a)
    m.free()


# The fold kernel is compiled once per (variables bound w, tiles per wave 2^GL), and GL > 0 -- the rolled loop over a wave's
# tiles with its shifting register window -- is chosen by the size of the table alone, from 2^21 elements on.
MULTI_TILE_NVS = [21, 22, 23]
MULTI_TILE_DIMS = [W - 2, W - 1, W]   # and all nv variables


def variants(nv, d):
    return set(zip(A.mle_fold_plan(nv, d)[1], A.mle_fold_tiles(nv, d)))


def test_the_multi_tile_cases_run_every_kernel_variant():
    """every (w, GL) with GL > 0 that ANY table size and dim can reach is reached by the cases of the test below"""
    reachable = set()
    for nv in range(59):
        for d in range(nv + 1):
            reachable |= variants(nv, d)
    multi = {v for v in reachable if v[1] > 0}
    assert multi and all(1 <= w <= W for w, _ in reachable)
    run = set()
    for nv in MULTI_TILE_NVS:
        for d in MULTI_TILE_DIMS + [nv]:
            run |= variants(nv, d)
    assert multi <= run, sorted(multi - run)
    small = set()
    for nv in NVS + [2 * W, 2 * W + 1]:
        for d in range(nv + 1):
            small |= variants(nv, d)
    assert all(gl == 0 for _, gl in small) and {v for v in reachable if v[1] == 0} <= small


@pytest.mark.parametrize("nv", MULTI_TILE_NVS)
def test_multi_tile_variants(nv):
    """fix_variables with dim in {W-2, W-1, W} and evaluate on block_tables of 2^21, 2^22 and 2^23 elements, every output
    element against the model, at the points 0, 1, p - 1, random and mixed"""
    fname = "BLS12_381_FR"
    p = pyref.MODULI[fname][0]
    a, gm, c, planted = block_table(nv, 57 + nv)
    m = MLE.from_evaluations(fname, nv, a)
    for label, pt, ptc in points(fname, nv, 5 + nv):
        for d in MULTI_TILE_DIMS:
            out = m.fix_variables(pt[:d])
            got, want = out.to_evaluations(), block_fold(gm, c, planted, ptc, d, p)
            assert out.num_vars == nv - d and np.array_equal(got, want), (label, d, np.nonzero((got != want).any(axis=1))[0][:5])
            out.free()
        rows = ints(block_fold(gm, c, planted, ptc, LO, p))
        value = pyref.to_limbs(mle_ref.evaluate(rows, ptc[LO:], p), 4)
        if label == "0":
            assert np.array_equal(value, a[0])
        if label == "1":
            assert np.array_equal(value, a[-1])
        assert np.array_equal(m.evaluate(pt), value), (label, "evaluate")
    assert np.array_equal(m.to_evaluations(), a), "input changed"
    m.free()


@pytest.mark.parametrize("nv", [12, 13])
def test_relabel(nv):
    fname = "BLS12_381_FR"
    p = pyref.MODULI[fname][0]
    a, am = table(fname, nv)
    _, pt, ptc = points(fname, nv, 11)[3]
    m = MLE.from_evaluations(fname, nv, a)
    want_value = pyref.to_limbs(mle_ref.evaluate(am, ptc, p), 4)
    inplace = m.clone()
    cur, cur_pt = list(am), pt.copy()
    for wa, wb, k in ((2, 2, 1), (3, 4, 1), (7, 5, 1), (2, 5, 3), (7, 0, 2), (0, nv - 1, 1), (nv - 4, 1, 4), (nv - 6, nv - 3, 3), (4, 9, 0)):
        # out of place, from the untouched table
        perm = [mle_ref.swap_bits(i, min(wa, wb), max(wa, wb), k) if wa != wb and k else i for i in range(1 << nv)]
        out = m.relabel(wa, wb, k)
        assert np.array_equal(out.to_evaluations(), a[perm]), (wa, wb, k)
        assert np.array_equal(m.to_evaluations(), a), "input changed"
        moved_pt = pt.copy()
        for t in range(k if wa != wb else 0):
            moved_pt[[wa + t, wb + t]] = moved_pt[[wb + t, wa + t]]
        assert np.array_equal(out.evaluate(moved_pt), want_value), (wa, wb, k, "evaluate with the point swapped the same way")
        out.free()
        # in place, one after the other as the reference's own test does (dense.rs:507-542)
        cur = mle_ref.relabel(cur, wa, wb, k)
        assert inplace.relabel_in_place(wa, wb, k) is inplace
        assert np.array_equal(inplace.to_evaluations(), limbs(cur)), (wa, wb, k, "in place")
        for t in range(k if wa != wb else 0):
            cur_pt[[wa + t, wb + t]] = cur_pt[[wb + t, wa + t]]
        assert np.array_equal(inplace.evaluate(cur_pt), want_value), (wa, wb, k, "in place: evaluate")
    for bad in ((1, nv - 1, 2), (nv - 1, 1, 2), (2, 3, 2), (5, 3, 4)):
        with pytest.raises(ValueError):
            m.relabel(*bad)
        assert lib().ark_hip_mle_relabel_device(m.field, m.evaluations.ptr, nv, bad[0], bad[1], bad[2], inplace.evaluations.ptr) == -1
    assert np.array_equal(inplace.to_evaluations(), limbs(cur))
    m.free()
    inplace.free()


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("n", [1, 63, 64, 65, (1 << 16) + 3])
def test_axpy(fname, n):
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    rinv = pow(pyref.R_of(p), -1, p)
    a = O.gen_scalars(fid, 61, n, montgomery=True)
    x = O.gen_scalars(fid, 62, n, montgomery=True)
    a[0], x[n // 2] = 0, pyref.to_limbs(p - 1, 4)
    am, xm = ints(a), ints(x)
    L = lib()
    ks = [("0", 0), ("1", pyref.R_of(p)), ("p-1", p - 1), ("random", pyref.from_limbs(O.gen_scalars(fid, 63, 1, montgomery=True)[0]))]
    for label, km in ks:                                # km: the scalar's Montgomery residue
        want = limbs([(u + km * v * rinv) % p for u, v in zip(am, xm)])   # (k R)(x R) / R = (k x) R
        k = pyref.to_limbs(km, 4)
        kp = k.ctypes.data_as(C.c_void_p)
        da, dx, dr = A.DeviceVec.from_host(fname, a), A.DeviceVec.from_host(fname, x), A.DeviceVec(fname, n)
        assert L.ark_hip_fr_axpy_device(da.field, da.ptr, kp, dx.ptr, dr.ptr, n) == 0
        assert np.array_equal(dr.to_host(), want), (label, "r")
        assert np.array_equal(da.to_host(), a) and np.array_equal(dx.to_host(), x), (label, "inputs changed")
        assert L.ark_hip_fr_axpy_device(da.field, da.ptr, kp, dx.ptr, da.ptr, n) == 0      # r == a
        assert np.array_equal(da.to_host(), want), (label, "r == a")
        da2 = A.DeviceVec.from_host(fname, a)
        assert L.ark_hip_fr_axpy_device(da.field, da2.ptr, kp, dx.ptr, dx.ptr, n) == 0     # r == x
        assert np.array_equal(dx.to_host(), want), (label, "r == x")
        for v in (da, dx, dr, da2):
            v.free()
    assert L.ark_hip_fr_axpy_device(O.FID[fname], None, k.ctypes.data_as(C.c_void_p), None, None, 0) == 0


@pytest.mark.parametrize("fname", FR)
def test_vector_space(fname):
    """+, -, neg, * scalar, += (f, other) with the reference's corner cases (dense.rs:278-432)"""
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    rinv = pow(pyref.R_of(p), -1, p)
    nv = 7
    a, am = table(fname, nv)
    b = O.gen_scalars(fid, 71, 1 << nv, montgomery=True)
    bm = ints(b)
    f = O.gen_scalars(fid, 72, 1, montgomery=True)[0]
    fm = pyref.from_limbs(f)
    A_, B_ = MLE.from_evaluations(fname, nv, a), MLE.from_evaluations(fname, nv, b)
    zero = MLE.zero(fname)
    assert zero.is_zero() and zero.num_vars == 0 and not A_.is_zero()
    assert not MLE.from_evaluations(fname, 1, np.zeros((2, 4), dtype=np.uint64)).is_zero()   # all zero, but num_vars = 1

    def same(m, nvars, want):
        assert m.num_vars == nvars and np.array_equal(m.to_evaluations(), limbs(want))

    same(A_ + B_, nv, [(u + v) % p for u, v in zip(am, bm)])
    same(A_ - B_, nv, [(u - v) % p for u, v in zip(am, bm)])
    same(-A_, nv, [(-u) % p for u in am])
    same(A_ * f, nv, [u * fm * rinv % p for u in am])
    same(A_ * enc(1, p), nv, am)
    # the zero polynomial: a copy of the other operand, whatever its num_vars
    same(A_ + zero, nv, am)
    same(zero + A_, nv, am)
    same(A_ - zero, nv, am)
    same(zero - A_, nv, [(-u) % p for u in am])
    same(zero + zero, 0, [0])
    prod = A_ * np.zeros(4, dtype=np.uint64)
    assert prod.is_zero() and prod.num_vars == 0                                              # * 0 gives zero()
    small = MLE.from_evaluations(fname, nv - 1, a[:1 << (nv - 1)])
    const = MLE.from_evaluations(fname, 0, enc(5, p))
    for l, r in ((A_, small), (small, A_), (A_, const), (const, A_)):
        with pytest.raises(ValueError):
            l + r
        with pytest.raises(ValueError):
            l - r
    # += (f, other): self + f other in one pass
    acc = A_.clone()
    acc += (f, B_)
    same(acc, nv, [(u + fm * v * rinv) % p for u, v in zip(am, bm)])
    acc += (f, zero)
    same(acc, nv, [(u + fm * v * rinv) % p for u, v in zip(am, bm)])
    acc += B_
    same(acc, nv, [(u + fm * v * rinv + v) % p for u, v in zip(am, bm)])
    z = MLE.zero(fname)
    z += (f, B_)                                                                              # zero += f B is f B
    same(z, nv, [fm * v * rinv % p for v in bm])
    z = MLE.zero(fname)
    z += (np.zeros(4, dtype=np.uint64), B_)                                                   # 0 B keeps B's num_vars (dense.rs:321-325)
    same(z, nv, [0] * (1 << nv))
    with pytest.raises(ValueError):
        acc += (f, small)
    assert np.array_equal(A_.to_evaluations(), a) and np.array_equal(B_.to_evaluations(), b)


def test_commit_and_evaluate_without_leaving_the_device(monkeypatch):
    """C = <bases, table> by MSM with Montgomery scalars read where the table lies, then the value at a point and a partial
    binding committed again: after the one upload only 32-byte elements (and MSM results) come back."""
    import torch
    cname, fname = "BLS12_381_G1", "BLS12_381_FR"
    cid, fid, r = O.CID[cname], O.FID[fname], pyref.MODULI[fname][0]
    fw = O.fe_words(cid)
    nv = 12
    n = 1 << nv
    L = lib()
    G = O.generator(cid)
    one = O.field_const(O.curve_info(cid)[0], 1)
    rng = np.random.default_rng(2024)
    ks = [int.from_bytes(rng.bytes(40), "little") % r for _ in range(n)]
    bases = A.batch_mul(cid, np.concatenate([G, one]), torch.from_numpy(mont_ints(ks, r).view(np.int64)).cuda())   # k_i G, affine, on the device
    a = O.gen_scalars(fid, 5, n, montgomery=True)
    m = MLE.from_evaluations(fname, nv, a)
    torch.cuda.synchronize()
    downloads = []
    to_host = A.DeviceVec.to_host
    monkeypatch.setattr(A.DeviceVec, "to_host", lambda v: (downloads.append(len(v)), to_host(v))[1])   # the one way a vector leaves

    def commit(vec, count):
        out = np.zeros(3 * fw, dtype=np.uint64)
        assert L.ark_hip_msm_sw_device(cid, bases.data_ptr(), vec.ptr, count, 1, out.ctypes.data_as(C.c_void_p)) == 0
        return out

    _, pt, ptc = points(fname, nv, 19)[3]
    Cm = commit(m.evaluations, n)
    value = m.evaluate(pt)
    half = m.fix_variables(pt[:nv // 2])
    Ch = commit(half.evaluations, len(half))
    value2 = half.evaluate(pt[nv // 2:])
    assert half.num_vars == nv - nv // 2 and not half.is_zero() and not (half + MLE.zero(fname)).is_zero()
    assert all(k <= 1 for k in downloads), "a table was copied to the host"
    monkeypatch.undo()
    am = ints(a)
    rinv = pow(pyref.R_of(r), -1, r)
    assert np.array_equal(value, pyref.to_limbs(mle_ref.evaluate(am, ptc, r), 4)) and np.array_equal(value2, value)
    # the commitments against the scalars they stand for: sum_i a_i k_i G
    s = sum(x * rinv % r * k for x, k in zip(am, ks)) % r
    assert np.array_equal(O.to_affine(cid, Cm), O.to_affine(cid, O.scalar_mul(cid, G, pyref.to_limbs(s, 4))))
    hm = mle_ref.fix_variables(am, ptc[:nv // 2], r)
    s = sum(x * rinv % r * k for x, k in zip(hm, ks)) % r
    assert np.array_equal(O.to_affine(cid, Ch), O.to_affine(cid, O.scalar_mul(cid, G, pyref.to_limbs(s, 4))))

