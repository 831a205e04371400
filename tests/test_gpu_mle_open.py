"""Multilinear openings on the device (ark_hip_mle_eq_table_device, ark_hip_mle_quotients_device) through the Python mirror,
limb for limb against the big-integer model of tests/mle_open_ref.py -- never against the code under test.  Outputs are
canonical Montgomery residues: no tolerance anywhere.

The quotients are linear in the table, so tables stay Montgomery residues a R used as the integers they are, with the POINT
in canonical form (tests/mle_ref.py).  The eq table is not linear: its model works on canonical values and converts at the
end.  Which sizes run which kernel variant is read from the library's own plans."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd import curves as cv
from algebra_amd._lib import check, lib
import mle_open_ref as R
import mle_ref
import msm_bucket_ref as B
import oracle_lib as O
import pyref
import sumcheck_ref as S
import test_gpu_mle as G                 # table(), points(), block_table(), block_fold(): section 12's constructions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR = G.FR
MLE = A.DenseMultilinearExtension
W = A.mle_eq_plan(0)[0]
ints, limbs = mle_ref.ints, mle_ref.limbs
SMALL = 12                               # up to here every kind of point and scale runs; above, the random ones


def modulus(fname):
    return pyref.MODULI[fname][0]


def plan_changes(plan, top):
    """the sizes up to `top` at which `plan` takes another number of launches or another tile count, each with its neighbours"""
    out = set()
    for nv in range(1, top + 1):
        a, b = plan(nv - 1), plan(nv)
        if len(a[1]) != len(b[1]) or sorted(set(a[2])) != sorted(set(b[2])):
            out |= {nv - 1, nv, nv + 1}
    return {nv for nv in out if nv <= top}


NVS = sorted(set(range(0, SMALL + 1)) | plan_changes(A.mle_eq_plan, 20) | plan_changes(A.mle_quotients_plan, 20) | {17, 20})
# the eq table takes more tiles per wave once the table is large enough: the sizes where that count changes, the smallest first
EQ_LARGE = [nv for nv in range(21, 28) if A.mle_eq_plan(nv)[2][-1] != A.mle_eq_plan(nv - 1)[2][-1]]


def variants(plan, nvs):
    return {(w, g) for nv in nvs for w, g in zip(plan(nv)[1], plan(nv)[2])}


def test_the_cases_run_every_kernel_variant():
    assert A.mle_eq_plan(W)[1] == [W] and len(A.mle_eq_plan(W + 1)[1]) == 2 and len(A.mle_eq_plan(2 * W + 1)[1]) == 3
    assert {W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 20} <= set(NVS)
    assert variants(A.mle_eq_plan, NVS + EQ_LARGE) == variants(A.mle_eq_plan, range(64))
    assert variants(A.mle_quotients_plan, NVS) == variants(A.mle_quotients_plan, range(64))
    assert {w for w, _ in variants(A.mle_quotients_plan, NVS)} == set(range(1, W + 1))
    assert EQ_LARGE and len(EQ_LARGE) <= 3, EQ_LARGE   # beyond the element-for-element grid: sampled, a few sizes only


def scales(fname, seed):
    """[(label, Montgomery limbs or None, canonical integer)]"""
    p = modulus(fname)
    rnd = ints(O.gen_scalars(O.FID[fname], seed, 1, montgomery=True))[0]
    return [("none", None, 1)] + [(label, G.enc(v, p), v) for label, v in (("0", 0), ("1", 1), ("p-1", p - 1), ("random", rnd))]


def peek(vec, index):
    out = np.zeros(4, dtype=np.uint64)
    check(lib().ark_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(vec.ptr.value + 32 * int(index)), 32), "ark_hip_memcpy_d2h")
    return out


# ---- the eq table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("nv", NVS)
def test_eq_table(fname, nv):
    p, Rm = modulus(fname), pyref.R_of(modulus(fname))
    pts, scs = G.points(fname, nv, 40 + nv), scales(fname, 60 + nv)
    if nv > SMALL:
        pts, scs = pts[3:4], scs[4:5] + (scs[:1] if nv == 20 else [])
    for label, pt, ptc in pts:
        for slabel, sc, scv in scs:
            want = limbs(R.eq_table_mont(ptc, scv, p, Rm))
            m = MLE.eq(fname, pt, sc)
            assert m.num_vars == nv and len(m) == 1 << nv
            got = m.to_evaluations()
            assert np.array_equal(got, want), (label, slabel, np.nonzero((got != want).any(axis=1))[0][:5])
            m.free()
        if label in ("0", "1") and nv:                 # a boolean point: the indicator of one index, times the scale
            m = MLE.eq(fname, pt, scs[-1][1])
            got = m.to_evaluations()
            hot = 0 if label == "0" else (1 << nv) - 1
            assert np.array_equal(got[hot], scs[-1][1]) and not np.delete(got, hot, axis=0).any()
            m.free()


def half_point(fname, nv):
    p = modulus(fname)
    return G.mont_ints([pow(2, -1, p)] * nv, p).reshape(-1, 4)


@pytest.mark.parametrize("nv", EQ_LARGE)
def test_eq_table_with_several_tiles_per_wave(nv):
    """the sizes that take 2, 4, 8 tiles per wave: 4096 sampled indices against the product formula, and the table's sum --
    2^nv times its value at (1/2, .., 1/2) -- equal to the scale; at the smallest of them also <eq(r), f> = f(r) on the device"""
    fname = "BLS12_381_FR"
    p, Rm = modulus(fname), pyref.R_of(modulus(fname))
    assert A.mle_eq_plan(nv)[2][-1] == EQ_LARGE.index(nv) + 1
    _, pt, ptc = G.points(fname, nv, 90 + nv)[3]
    _, sc, scv = scales(fname, 91 + nv)[4]
    m = MLE.eq(fname, pt, sc)
    n, T = 1 << nv, 1 << W
    rng = np.random.default_rng(nv)
    tiles = [0, n // T - 1, n // (2 * T) + 3]
    idx = [t * T + o for t in tiles for o in (0, 1, 63, 64, T - 1)] + [int(v) for v in rng.integers(0, n, size=4096 - 15)]
    for i in idx:
        assert np.array_equal(peek(m.evaluations, i), pyref.to_limbs(mle_ref.eq(i, ptc, p) * scv % p * Rm % p, 4)), i
    total = ints(m.evaluate(half_point(fname, nv)).reshape(1, 4))[0] * pow(2, nv, p) % p
    assert total == scv * Rm % p, "sum of the table"
    if nv == EQ_LARGE[0]:
        a = G.block_table(nv, 5)[0]
        f = MLE.from_evaluations(fname, nv, a)
        ip = f.evaluations.inner_product(m.evaluations)
        fr = ints(f.evaluate(pt).reshape(1, 4))[0]                                   # f(r) R
        assert ints(np.asarray(ip).reshape(1, 4))[0] == fr * scv % p, "<eq(r), f> = scale f(r)"
        f.free()
    m.free()


# ---- the quotients ---------------------------------------------------------------------------------------------------
def check_quotients(m, nv, pt, want_value, want_segments, tag):
    value, segs = m.quotients(pt)
    assert len(segs) == nv and np.array_equal(value, want_value), (tag, "value")
    for i, (seg, want) in enumerate(zip(segs, want_segments)):
        assert seg.offset == R.segment_offset(nv, i) and len(seg) == R.segment_len(nv, i)
        got = seg.to_host()
        assert np.array_equal(got, want), (tag, "segment", i, np.nonzero((got != want).any(axis=1))[0][:5])
    if nv:
        assert np.array_equal(value, m.evaluate(pt)), (tag, "the value against evaluate, bit for bit")
        assert all(s.owner is segs[0].owner for s in segs) and len(segs[0].owner) == (1 << nv) - 1, "views into one vector"
    return segs


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("nv", NVS)
def test_quotients(fname, nv):
    p = modulus(fname)
    a, am = G.table(fname, nv)
    m = MLE.from_evaluations(fname, nv, a)
    pts = G.points(fname, nv, 20 + nv)
    if nv > SMALL:
        pts = pts[3:4]
    for label, pt, ptc in pts:
        value, qs = R.quotients(list(am), ptc, p)
        segs = check_quotients(m, nv, pt, pyref.to_limbs(value, 4), [limbs(q) for q in qs], label)
        if label == "0":
            assert value == am[0]
        if label == "1":
            assert value == am[-1]
        if label == "random" and nv:                   # without a value the call is asynchronous: the same segments
            none, other = m.quotients(pt, wait=False)
            check(lib().ark_hip_synchronize(), "ark_hip_synchronize")
            assert none is None and np.array_equal(other[0].owner.to_host(), segs[0].owner.to_host())
        assert np.array_equal(m.to_evaluations(), a), (label, "input changed")
    m.free()


def test_quotients_of_a_constant():
    """num_vars = 0: no quotient, d_quot may be NULL, the value is the one entry"""
    for fname in FR:
        a, _ = G.table(fname, 0)
        m = MLE.from_evaluations(fname, 0, a)
        out = np.zeros(4, dtype=np.uint64)
        check(lib().ark_hip_mle_quotients_device(m.field, m.evaluations.ptr, 0, None, None, out.ctypes.data_as(C.c_void_p)), "quotients")
        assert np.array_equal(out, a[0])
        check(lib().ark_hip_mle_quotients_device(m.field, m.evaluations.ptr, 0, None, None, None), "quotients")
        value, segs = m.quotients(np.zeros((0, 4), dtype=np.uint64))
        assert np.array_equal(value, a[0]) and segs == []
        m.free()


def test_quotients_at_2_21():
    """element for element on section 12's block table: below LO variables every segment is the blocks' own quotients laid out
    by the map, plus each planted element's share; from LO on the model walks the 2^(nv-LO) rows that are left"""
    fname, nv, LO = "BLS12_381_FR", 21, G.LO
    p = modulus(fname)
    assert len(A.mle_quotients_plan(nv)[1]) == 3
    a, gm, c, planted = G.block_table(nv, 21)
    _, pt, ptc = G.points(fname, nv, 77)[3]
    per_block = [R.quotients(gm[q], ptc[:LO], p)[1] for q in range(4)]
    want = []
    for i in range(LO):
        seg = np.stack([limbs(per_block[q][i]) for q in range(4)])[c].reshape(-1, 4).copy()
        delta = {}
        for idx, (old, new) in planted.items():
            share = (new - old) * mle_ref.eq(idx & ((1 << i) - 1), ptc[:i], p)
            o = idx >> (i + 1)
            delta[o] = (delta.get(o, 0) + (share if (idx >> i) & 1 else -share)) % p
        for o, dv in delta.items():
            seg[o] = pyref.to_limbs((pyref.from_limbs(seg[o]) + dv) % p, 4)
        want.append(seg)
    rows = ints(G.block_fold(gm, c, planted, ptc, LO, p))
    value, high = R.quotients(rows, ptc[LO:], p)
    want += [limbs(q) for q in high]
    m = MLE.from_evaluations(fname, nv, a)
    check_quotients(m, nv, pt, pyref.to_limbs(value, 4), want, "2^21")
    assert np.array_equal(m.to_evaluations(), a), "input changed"
    m.free()


# ---- stale scratch ---------------------------------------------------------------------------------------------------
def test_small_calls_on_poisoned_scratch():
    """tests/mle_open_scratch_child.py: a small eq table and small quotients after larger calls on the same context, then again
    with every scratch buffer poisoned (ark_hip_test_scratch_poison): the same results, nothing written past what was asked"""
    env = dict(os.environ, ARK_HIP_LIB=os.path.join(ROOT, "algebra_amd", "libark_hip_test.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mle_open_scratch_child.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mle-open scratch ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ---- end to end ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def known_bases(curve, n):
    """n bases [k_i] G with known k_i (tests/msm_bucket_ref.py), on the device"""
    import torch
    cr = B.CurveRef(curve)
    rng = np.random.default_rng(4242)
    logs = [int.from_bytes(rng.bytes(40), "little") % cr.r for _ in range(n)]
    dev = torch.from_numpy(np.ascontiguousarray(cr.bases(logs)).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return cr, logs, dev


def point_of_log(cr, k):
    return O.to_affine(cr.cid, O.scalar_mul(cr.cid, O.generator(cr.cid), pyref.to_limbs(k % cr.r, 4)))


def test_commit_sumcheck_open():
    """commit -> sumcheck of eq a b with the eq table built on the device -> open a at the sumcheck's point, with level i's
    bases the same slice of one base array that q_i is of the quotient vector; every point against the oracle's scalar
    multiplication of sum_b q_i[b] dlog(B_i[b])"""
    fname, curve, nv = "BLS12_381_FR", "BLS12_381_G1", 10
    p, Rm = modulus(fname), pyref.R_of(modulus(fname))
    n = 1 << nv
    cr, logs, dbases = known_bases(curve, n)
    assert cr.r == p
    inv = pow(Rm, -1, p)
    arrays = [G.table(fname, nv)[0], O.gen_scalars(O.FID[fname], 555, n, montgomery=True)]
    canon = [[v * inv % p for v in ints(x)] for x in arrays]                       # the tables' values
    a, b = (MLE.from_evaluations(fname, nv, x) for x in arrays)                    # the uploads
    # commit to a: an MSM over the table where it lies
    com = np.zeros(cv.projective_words(cr.cid), dtype=np.uint64)
    check(lib().ark_hip_msm_sw_device(cr.cid, dbases.data_ptr(), a.evaluations.ptr, n, 1, com.ctypes.data_as(C.c_void_p)), "commit")
    assert np.array_equal(A.into_affine(cr.cid, com), point_of_log(cr, sum(v * k for v, k in zip(canon[0], logs))))
    # sumcheck of sum_b eq(tau, b) a[b] b[b]
    _, tau, tauc = G.points(fname, nv, 31)[3]
    eqc = R.eq_table(tauc, 1, p)
    e = MLE.eq(fname, tau)
    terms = [(1, [0, 1, 2])]
    claim = sum(x * y * z for x, y, z in zip(eqc, canon[0], canon[1])) % p
    lp = A.ListOfProducts(fname, nv)
    lp.add_product([e, a, b], pyref.to_mont(1, p))
    device_challenge, _ = S.hash_challenge(p)
    proof = lp.prove(device_challenge)
    rounds, point = [S.decode(g, p) for g in proof.rounds], S.decode(proof.point, p)
    finals = S.decode(proof.final_evaluations, p)
    assert S.verify(claim, rounds, point, finals, terms, p), "the verifier rejects"
    assert finals[0] == mle_ref.eq((1 << nv) - 1, [(t * z + (1 - t) * (1 - z)) % p for t, z in zip(tauc, point)], p), "eq(tau, point)"
    # open a at the sumcheck's point
    levels = [dbases.data_ptr() + cv.affine_bytes(cr.cid) * R.segment_offset(nv, i) for i in range(nv)]
    value, pts = a.open(proof.point, levels, curve)
    assert np.array_equal(value, proof.final_evaluations[1]), "the opened value is the proof's final evaluation of that table"
    want_value, qs = R.quotients(canon[0], point, p)
    assert ints(value.reshape(1, 4))[0] == want_value * Rm % p
    for i, q in enumerate(qs):
        at = R.segment_offset(nv, i)
        k = sum(v * logs[at + j] for j, v in enumerate(q))
        assert np.array_equal(A.into_affine(cr.cid, pts[i]), point_of_log(cr, k)), ("level", i)
    with pytest.raises(ValueError):
        a.open(proof.point, levels[:-1], curve)
    with pytest.raises(ValueError):
        a.open(proof.point, levels, "BN254_G1")
    lp.free()
    for m in (a, b, e):
        m.free()
