"""Grand products on the device (ark_hip_mle_product_tree_device, ark_hip_fr_lincomb_device, GrandProduct.prove) limb for limb
against the big-integer model of tests/grand_product_ref.py -- never against the code under test.  Montgomery products of
canonical residues are canonical whatever the association: no tolerance anywhere.

A product is not linear in R, so the model works on canonical values (sumcheck_ref.decode / encode); the linear combination
is linear in the tables, so there the tables stay Montgomery residues used as the integers they are, with canonical
coefficients.  Which sizes run which kernel variant is read from the library's own plan."""
import ctypes as C
import functools

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd._lib import check, lib
import grand_product_ref as R
import mle_ref
import oracle_lib as O
import pyref
import sumcheck_ref as S
import test_gpu_mle as G                 # enc(), mont_ints(): section 12's constructions

pytestmark = pytest.mark.gpu

FR = G.FR
MLE = A.DenseMultilinearExtension
ints, limbs = mle_ref.ints, mle_ref.limbs
ERR_ARG = -1
GUARD = 67                               # elements behind the tree that must stay as they were
NVS = list(range(0, 13))


def modulus(fname):
    return pyref.MODULI[fname][0]


def variants(nvs):
    return {v for nv in nvs for v in A.mle_product_tree_launches(nv)}


def test_the_cases_run_every_kernel_variant():
    """every (levels, chunks per wave) the plan reports for up to 26 variables is run by the sizes of the grid"""
    assert variants(NVS) == variants(range(27)), variants(range(27)) - variants(NVS)
    assert {w for w, _ in variants(NVS)} == set(range(1, A.mle.PRODUCT_TREE_LEVELS + 1))
    for nv in range(27):                 # the mirror's launches are the plan's runs spelled out
        assert sum(w for w, _ in A.mle_product_tree_launches(nv)) == nv == sum(A.mle_product_tree_plan(nv)[0])


@functools.lru_cache(maxsize=None)
def table(fname, nv, kind):
    """2^nv elements, cached and never written to.  "planted": random with the residues 0, 1, p - 1 and R mod p planted;
    "last-zero": random with its ONLY zero in the last cell, so the zero has to travel through every level; "random": as drawn"""
    fid, p = O.FID[fname], modulus(fname)
    n = 1 << nv
    a = O.gen_scalars(fid, 1900 + nv, n, montgomery=True).copy()
    assert a.any(axis=1).all()
    if kind == "planted":
        for at, v in ((1, 0), (2, 1), (3, p - 1), (4, pyref.R_of(p)), (n - 2, 0)):
            if 0 <= at < n and n >= 8:
                a[at] = pyref.to_limbs(v, 4)
    elif kind == "last-zero":
        a[n - 1] = 0
    a.setflags(write=False)
    return a, tuple(S.decode(a, p))


def check_tree(fname, nv, kind):
    p = modulus(fname)
    a, canon = table(fname, nv, kind)
    n = 1 << nv
    product, flat = R.tree(list(canon), p)
    want = S.encode(flat, p) if flat else np.zeros((0, 4), dtype=np.uint64)
    want_product = S.encode([product], p)[0]
    m = MLE.from_evaluations(fname, nv, a)
    # the raw entry into a buffer with a guard region behind the 2^nv - 1 elements
    pattern = O.gen_scalars(O.FID[fname], 77, n - 1 + GUARD, montgomery=True)
    for wait in (True, False):
        buf = A.DeviceVec.from_host(fname, pattern)
        out = np.zeros(4, dtype=np.uint64)
        check(lib().ark_hip_mle_product_tree_device(m.field, m.evaluations.ptr, nv, buf.ptr if nv else None,
                                                    out.ctypes.data_as(C.c_void_p) if wait else None), "ark_hip_mle_product_tree_device")
        if not wait:
            check(lib().ark_hip_synchronize(), "ark_hip_synchronize")
        got = buf.to_host()
        assert np.array_equal(got[:n - 1], want), (kind, wait, np.nonzero((got[:n - 1] != want).any(axis=1))[0][:5])
        assert np.array_equal(got[n - 1:], pattern[n - 1:]), (kind, wait, "the guard region was written")
        if wait:
            assert np.array_equal(out, want_product), (kind, "product")
        buf.free()
    # the mirror: the levels as views of one vector
    got_product, levels = m.product_tree()
    assert np.array_equal(got_product, want_product) and len(levels) == nv
    lv = R.levels(list(canon), p)
    for j, seg in enumerate(levels, 1):
        assert seg.offset == R.level_offset(nv, j) and len(seg) == R.level_len(nv, j)
        assert np.array_equal(seg.to_host(), S.encode(lv[j], p)), (kind, "level", j)
    if nv:
        assert all(s.owner is levels[0].owner for s in levels) and len(levels[0].owner) == n - 1, "views into one vector"
        assert np.array_equal(levels[-1].to_host()[0], want_product)
        levels[0].owner.free()
    if kind == "random":
        assert product != 0
    if kind == "last-zero":
        assert product == 0 and all(level[-1] == 0 and all(level[:-1]) for level in lv[1:]) or nv == 0
    none, levels = m.product_tree(wait=False)
    check(lib().ark_hip_synchronize(), "ark_hip_synchronize")
    assert none is None and (nv == 0 or np.array_equal(levels[0].owner.to_host(), want))
    assert np.array_equal(m.to_evaluations(), a), (kind, "input changed")
    if nv:
        levels[0].owner.free()
    m.free()


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("nv", NVS)
def test_product_tree(fname, nv):
    for kind in ("planted", "last-zero", "random"):     # "random": a nonzero product and dense last levels
        check_tree(fname, nv, kind)


def test_an_overlapping_tree_is_refused():
    for fname in FR:
        nv = 5
        m = MLE.from_evaluations(fname, nv, table(fname, nv, "planted")[0])
        big = A.DeviceVec(fname, 3 << nv)
        base = m.evaluations.ptr.value
        out = np.zeros(4, dtype=np.uint64)
        f = lib().ark_hip_mle_product_tree_device
        for ptr in (base, base + 32, base + 32 * 31, base - 32 * 30):
            assert f(m.field, m.evaluations.ptr, nv, C.c_void_p(ptr), out.ctypes.data_as(C.c_void_p)) == ERR_ARG
            assert f(m.field, m.evaluations.ptr, nv, C.c_void_p(ptr), None) == ERR_ARG
        # inside one allocation: the table in the middle third, the tree right before and right behind it
        mid = big.ptr.value + (32 << nv)
        check(lib().ark_hip_memcpy_d2d(C.c_void_p(mid), m.evaluations.ptr, 32 << nv), "ark_hip_memcpy_d2d")
        want = np.asarray(m.product_tree()[0])
        for ptr in (mid + (32 << nv), mid - 32 * 31):
            check(f(m.field, C.c_void_p(mid), nv, C.c_void_p(ptr), out.ctypes.data_as(C.c_void_p)), "adjacent, not overlapping")
            assert np.array_equal(out, want)
        big.free()
        m.free()


# ---- the linear combination ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_linear_combination(fname, K):
    p, fid = modulus(fname), O.FID[fname]
    Rm = pyref.R_of(p)
    rnd = ints(O.gen_scalars(fid, 300 + K, K + 1, montgomery=True))
    coeffs = [(0, p - 1, x)[k % 3] if K > 1 else x for k, x in enumerate(rnd[:K])]      # canonical; zero and p - 1 among them
    if K == 8:
        coeffs[3], coeffs[4] = 1, rnd[4]
    c0 = rnd[K]
    kc = G.mont_ints(coeffs, p).reshape(-1, 4)
    g = G.enc(c0, p)
    for n in (1, 63, 64, 65, 513, 4097):
        host = [O.gen_scalars(fid, 400 + 10 * K + k, n, montgomery=True).copy() for k in range(K)]
        if n >= 4:
            host[0][1] = 0
            host[K - 1][2] = pyref.to_limbs(p - 1, 4)
        tabs = [ints(h) for h in host]
        for with_c0 in (True, False):
            want = limbs(R.lincomb(tabs, coeffs, c0 * Rm % p if with_c0 else 0, p))
            for alias in (None, 0, K - 1):
                dev = [A.DeviceVec.from_host(fname, h) for h in host]
                out = A.DeviceVec(fname, n) if alias is None else dev[alias]
                ptrs = (C.c_void_p * K)(*[d.ptr.value for d in dev])
                check(lib().ark_hip_fr_lincomb_device(dev[0].field, ptrs, K, kc.ctypes.data_as(C.c_void_p),
                                                      g.ctypes.data_as(C.c_void_p) if with_c0 else None, out.ptr, n), "ark_hip_fr_lincomb_device")
                got = out.to_host()
                assert np.array_equal(got, want), (n, with_c0, alias, np.nonzero((got != want).any(axis=1))[0][:5])
                for k, d in enumerate(dev):
                    if k != alias:
                        assert np.array_equal(d.to_host(), host[k]), (n, alias, "table", k, "changed")
                    d.free()
                if alias is None:
                    out.free()
    # partial overlaps of the output with a table are refused
    dev = A.DeviceVec(fname, 64)
    ptrs = (C.c_void_p * 1)(dev.ptr.value)
    assert lib().ark_hip_fr_lincomb_device(dev.field, ptrs, 1, kc.ctypes.data_as(C.c_void_p), None, C.c_void_p(dev.ptr.value + 32), 32) == ERR_ARG
    dev.free()


def test_linear_combination_of_the_mirror():
    fname, nv = "BLS12_381_FR", 7
    p = modulus(fname)
    hosts = [O.gen_scalars(O.FID[fname], 500 + k, 1 << nv, montgomery=True) for k in range(3)]
    ms = [MLE.from_evaluations(fname, nv, h) for h in hosts]
    coeffs, gamma = [3, p - 2, 5], 11
    out = MLE.linear_combination(ms, G.mont_ints(coeffs, p).reshape(-1, 4), G.enc(gamma, p))
    assert out.num_vars == nv
    assert np.array_equal(out.to_evaluations(), limbs(R.lincomb([ints(h) for h in hosts], coeffs, gamma * pyref.R_of(p) % p, p)))
    none = MLE.linear_combination(ms[:1], G.mont_ints(coeffs[:1], p).reshape(-1, 4))
    assert np.array_equal(none.to_evaluations(), limbs(R.lincomb([ints(hosts[0])], coeffs[:1], 0, p)))
    with pytest.raises(ValueError):
        MLE.linear_combination(ms, G.mont_ints(coeffs[:2], p).reshape(-1, 4))
    with pytest.raises(ValueError):
        MLE.linear_combination([], np.zeros((0, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        MLE.linear_combination([ms[0], MLE.from_evaluations(fname, 0, hosts[0][:1])], G.mont_ints(coeffs[:2], p).reshape(-1, 4))
    for m in ms + [out, none]:
        m.free()


# ---- the layered proof -----------------------------------------------------------------------------------------------
def prove_and_verify(fname, m, canon):
    """GrandProduct.prove with transcript-derived challenges, accepted by the model's verifier; -> (proof, canonical product)"""
    p = modulus(fname)
    nv = m.num_vars
    device_challenge, model_challenge = R.hash_challenge(p)
    before = m.to_evaluations()
    proof = A.GrandProduct(m).prove(device_challenge)
    product, layers, point = R.decode_proof(proof, p)
    assert product == R.tree(list(canon), p)[0], "product"
    assert len(proof.layers) == nv and proof.point.shape == (nv, 4)
    assert all((sc is None) == (k == 0) for k, (sc, _) in enumerate(proof.layers))
    ok, vpoint, claim = R.verify(nv, product, layers, model_challenge, p)
    assert ok, "the model's verifier rejects"
    assert vpoint == point, "the proof's point is the transcript's"
    assert np.array_equal(m.evaluate(proof.point), S.encode([claim], p)[0]), "f(point) on the device is the verifier's last claim"
    assert claim == mle_ref.evaluate(list(canon), point, p)
    assert np.array_equal(m.to_evaluations(), before), "input changed"
    return proof, product


@pytest.mark.parametrize("fname,nv", [(f, nv) for f in FR for nv in (0, 1, 2, 3, 9)] + [("BLS12_381_FR", 12)])
def test_proof(fname, nv):
    a, canon = table(fname, nv, "planted" if nv in (3, 12) else "last-zero" if nv == 2 else "random")
    m = MLE.from_evaluations(fname, nv, a)
    proof, product = prove_and_verify(fname, m, canon)
    if nv == 9:                                        # the model's own prover writes the same proof
        want = R.prove(list(canon), R.hash_challenge(modulus(fname))[1], modulus(fname))
        assert (want[0], want[2]) == (product, R.decode_proof(proof, modulus(fname))[2])
        assert want[1] == R.decode_proof(proof, modulus(fname))[1]
    m.free()


def test_a_view_is_an_extension():
    """a DeviceSegment as the evaluations of a DenseMultilinearExtension: the binding entries run on it, free() frees nothing"""
    fname, nv = "BLS12_381_FR", 6
    p = modulus(fname)
    a, _ = table(fname, nv, "planted")
    m = MLE.from_evaluations(fname, nv, a)
    half = MLE(nv - 1, A.DeviceSegment(m.evaluations, 1 << (nv - 1), 1 << (nv - 1)))
    pt = G.points(fname, nv - 1, 5)[3]
    assert np.array_equal(half.evaluate(pt[1]), pyref.to_limbs(mle_ref.evaluate(ints(a[1 << (nv - 1):]), pt[2], p), 4))
    assert np.array_equal(half.to_evaluations(), a[1 << (nv - 1):])
    half.free()
    assert np.array_equal(m.to_evaluations(), a), "the owner outlives its view's free()"
    m.free()


def test_permutation_check_end_to_end():
    """fingerprints gamma + sum_k c_k T_k[i] of three tables and of the same rows permuted have the same grand product, and
    both layered proofs are accepted"""
    fname, nv = "BLS12_381_FR", 7
    p, fid = modulus(fname), O.FID[fname]
    n = 1 << nv
    Rinv = pow(pyref.R_of(p), -1, p)
    hosts = [O.gen_scalars(fid, 700 + k, n, montgomery=True) for k in range(3)]
    perm = np.random.default_rng(7).permutation(n)
    assert (perm != np.arange(n)).any()
    rnd = ints(O.gen_scalars(fid, 710, 4, montgomery=True))
    coeffs, gamma = rnd[:3], rnd[3]
    kc, g = G.mont_ints(coeffs, p).reshape(-1, 4), G.enc(gamma, p)
    products = []
    for rows in (hosts, [h[perm] for h in hosts]):
        ms = [MLE.from_evaluations(fname, nv, h) for h in rows]
        leaves = MLE.linear_combination(ms, kc, g)
        canon = [(gamma + sum(c * (t * Rinv % p) for c, t in zip(coeffs, ts))) % p for ts in zip(*[ints(h) for h in rows])]
        assert np.array_equal(leaves.to_evaluations(), S.encode(canon, p))
        proof, product = prove_and_verify(fname, leaves, canon)
        products.append((product, np.asarray(proof.product).tolist()))
        for m in ms + [leaves]:
            m.free()
    assert products[0] == products[1] and products[0][0] != 0
    # one row changed: another product
    bad = [h.copy() for h in hosts]
    bad[1][5] = hosts[1][6]
    ms = [MLE.from_evaluations(fname, nv, h) for h in bad]
    leaves = MLE.linear_combination(ms, kc, g)
    assert np.asarray(leaves.product_tree()[0]).tolist() != products[0][1]
    for m in ms + [leaves]:
        m.free()
