"""Fractional sums on the device (ark_hip_mle_fraction_tree_device, ark_hip_fr_count_indices_device, FractionalSum.prove) limb
for limb against the big-integer model of tests/fraction_sum_ref.py -- never against the code under test.  Every value the
entries write is the canonical Montgomery residue, whatever the schedule of the products: no tolerance anywhere.

The model works on canonical values (sumcheck_ref.decode / encode).  Which sizes run which kernel variant is read from the
library's own plan."""
import ctypes as C
import functools

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd._lib import check, lib
import fraction_sum_ref as R
import mle_ref
import oracle_lib as O
import pyref
import sumcheck_ref as S
import test_gpu_mle as G                 # enc(), mont_ints(): section 12's constructions

pytestmark = pytest.mark.gpu

FR = G.FR
MLE = A.DenseMultilinearExtension
ERR_ARG = -1
GUARD = 67                               # elements behind a buffer that must stay as they were
NVS = list(range(0, 13))
KINDS = ("planted", "last-zero", "random")


def modulus(fname):
    return pyref.MODULI[fname][0]


def variants(nvs):
    return {v for nv in nvs for has_num in (True, False) for v in A.mle_fraction_tree_launches(nv, has_num)}


def test_the_cases_run_every_kernel_variant():
    """every (levels, numerators read) the plan reports for up to 26 variables is run by the sizes of the grid"""
    assert variants(NVS) == variants(range(27)), variants(range(27)) - variants(NVS)
    assert variants(NVS) == {(w, r) for w in range(1, A.mle.FRACTION_TREE_LEVELS + 1) for r in (True, False)}
    # log2 of the outputs of the first launch: below one wave of 64, one wave, several waves
    outs = {nv - min(nv, A.mle.FRACTION_TREE_LEVELS) for nv in NVS if nv}
    assert min(outs) < 6 and 6 in outs and max(outs) >= 8


@functools.lru_cache(maxsize=None)
def table(fname, nv, kind, seed=0):
    """2^nv elements, cached and never written to.  "planted": random with the residues 0, 1, p - 1 and R mod p planted;
    "last-zero": random with its ONLY zero in the last cell; "random": as drawn"""
    fid, p = O.FID[fname], modulus(fname)
    n = 1 << nv
    a = O.gen_scalars(fid, 2100 + 50 * seed + nv, n, montgomery=True).copy()
    assert a.any(axis=1).all()
    if kind == "planted":
        cells = ((1, 0), (2, 1), (3, p - 1), (4, pyref.R_of(p)), (n - 2, 0)) if seed == 0 else \
            ((1, p - 1), (2, 0), (3, pyref.R_of(p)), (5, 1), (n - 1, 0))
        for at, v in cells:
            if 0 <= at < n and n >= 8:
                a[at] = pyref.to_limbs(v, 4)
    elif kind == "last-zero":
        a[n - 1] = 0
    a.setflags(write=False)
    return a, tuple(S.decode(a, p))


@functools.lru_cache(maxsize=None)
def model_tree(fname, nv, kind, has_num):
    """the model's root and tree buffers as Montgomery limbs, computed once per case"""
    p = modulus(fname)
    den = list(table(fname, nv, kind)[1])
    # "last-zero" keeps the single zero in the denominators: the numerators are random there
    num = list(table(fname, nv, "random" if kind == "last-zero" else kind, seed=1)[1]) if has_num else None
    root, nflat, dflat = R.tree(num, den, p)
    enc = lambda xs: S.encode(xs, p) if xs else np.zeros((0, 4), dtype=np.uint64)   # noqa: E731
    return root, S.encode(list(root), p), enc(nflat), enc(dflat)


def check_tree(fname, nv, kind, has_num):
    p = modulus(fname)
    n = 1 << nv
    da, dcanon = table(fname, nv, kind)
    na, ncanon = table(fname, nv, "random" if kind == "last-zero" else kind, seed=1) if has_num else (None, None)
    root, want_root, want_n, want_d = model_tree(fname, nv, kind, has_num)
    den = MLE.from_evaluations(fname, nv, da)
    num = MLE.from_evaluations(fname, nv, na) if has_num else None
    # the raw entry into buffers with a guard region behind the 2^nv - 1 elements of each tree
    pattern = O.gen_scalars(O.FID[fname], 78, n - 1 + GUARD, montgomery=True)
    for wait in (True, False):
        bufs = [A.DeviceVec.from_host(fname, pattern) for _ in range(2)]
        out = np.zeros((2, 4), dtype=np.uint64)
        check(lib().ark_hip_mle_fraction_tree_device(den.field, num.evaluations.ptr if has_num else None, den.evaluations.ptr, nv,
                                                     bufs[0].ptr if nv else None, bufs[1].ptr if nv else None,
                                                     out.ctypes.data_as(C.c_void_p) if wait else None), "ark_hip_mle_fraction_tree_device")
        if not wait:
            check(lib().ark_hip_synchronize(), "ark_hip_synchronize")
        for buf, want, name in ((bufs[0], want_n, "numerators"), (bufs[1], want_d, "denominators")):
            got = buf.to_host()
            assert np.array_equal(got[:n - 1], want), (kind, has_num, wait, name, np.nonzero((got[:n - 1] != want).any(axis=1))[0][:5])
            assert np.array_equal(got[n - 1:], pattern[n - 1:]), (kind, has_num, wait, name, "the guard region was written")
            buf.free()
        if wait:
            assert np.array_equal(out, want_root), (kind, has_num, "root")
    # the mirror: the levels of each tree as views of one vector
    got_root, nlevels, dlevels = den.fraction_tree(num)
    assert np.array_equal(got_root, want_root) and len(nlevels) == len(dlevels) == nv
    ns, ds = R.levels(None if num is None else list(ncanon), list(dcanon), p)
    for levels, lv in ((nlevels, ns), (dlevels, ds)):
        for j, seg in enumerate(levels, 1):
            assert seg.offset == R.level_offset(nv, j) and len(seg) == R.level_len(nv, j)
            assert np.array_equal(seg.to_host(), S.encode(lv[j], p)), (kind, has_num, "level", j)
        if nv:
            assert all(s.owner is levels[0].owner for s in levels) and len(levels[0].owner) == n - 1, "views into one vector"
            levels[0].owner.free()
    if kind == "last-zero":
        assert root[1] == 0 and (nv == 0 or all(level[-1] == 0 and all(level[:-1]) for level in ds[1:]))
    none, nlevels, dlevels = den.fraction_tree(num, wait=False)
    check(lib().ark_hip_synchronize(), "ark_hip_synchronize")
    assert none is None
    if nv:
        assert np.array_equal(nlevels[0].owner.to_host(), want_n) and np.array_equal(dlevels[0].owner.to_host(), want_d)
        nlevels[0].owner.free()
        dlevels[0].owner.free()
    assert np.array_equal(den.to_evaluations(), da), (kind, "denominators changed")
    den.free()
    if has_num:
        assert np.array_equal(num.to_evaluations(), na), (kind, "numerators changed")
        num.free()


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("nv", NVS)
def test_fraction_tree(fname, nv):
    for kind in KINDS:
        for has_num in (True, False):
            check_tree(fname, nv, kind, has_num)


def test_overlapping_buffers_are_refused():
    for fname in FR:
        nv = 5
        n = 1 << nv
        den = MLE.from_evaluations(fname, nv, table(fname, nv, "planted")[0])
        num = MLE.from_evaluations(fname, nv, table(fname, nv, "planted", seed=1)[0])
        big = A.DeviceVec(fname, 4 * n)
        other = A.DeviceVec(fname, n)
        out = np.zeros((2, 4), dtype=np.uint64)
        out_p = out.ctypes.data_as(C.c_void_p)
        f = lib().ark_hip_mle_fraction_tree_device
        dbase, nbase, free = den.evaluations.ptr.value, num.evaluations.ptr.value, other.ptr
        for base, nm in ((dbase, num.evaluations.ptr), (dbase, None), (nbase, num.evaluations.ptr)):
            for ptr in (base, base + 32, base + 32 * (n - 1), base - 32 * (n - 2)):
                assert f(den.field, nm, den.evaluations.ptr, nv, C.c_void_p(ptr), free, out_p) == ERR_ARG
                assert f(den.field, nm, den.evaluations.ptr, nv, free, C.c_void_p(ptr), None) == ERR_ARG
        at = big.ptr.value + 32 * n                            # the two trees on each other
        for ptr in (at, at + 32 * (n - 2), at - 32 * (n - 2)):
            assert f(den.field, None, den.evaluations.ptr, nv, C.c_void_p(at), C.c_void_p(ptr), out_p) == ERR_ARG
        # inside one allocation, everything adjacent: [num tree | den table | den tree]
        mid = big.ptr.value + 32 * n
        check(lib().ark_hip_memcpy_d2d(C.c_void_p(mid), den.evaluations.ptr, 32 * n), "ark_hip_memcpy_d2d")
        want = den.fraction_tree(None)
        check(f(den.field, None, C.c_void_p(mid), nv, C.c_void_p(mid - 32 * (n - 1)), C.c_void_p(mid + 32 * n), out_p), "adjacent, not overlapping")
        assert np.array_equal(out, want[0])
        for levels in want[1:]:
            levels[0].owner.free()
        for v in (big, other):
            v.free()
        den.free()
        num.free()


# ---- the multiplicities ----------------------------------------------------------------------------------------------
def index_sets(n, table_len, seed):
    rng = np.random.default_rng(seed)
    yield "uniform", rng.integers(0, table_len, size=n, dtype=np.uint32)
    yield "all-equal", np.full(n, table_len - 1, dtype=np.uint32)
    out = rng.integers(table_len, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    out[:1], out[1:2] = table_len, 0xFFFFFFFF                # the first index past the table and the largest
    yield "all-out-of-range", out
    mix = rng.integers(0, table_len, size=n, dtype=np.uint32)
    mix[rng.random(n) < 0.3] = table_len + 5                 # about a third of them are skipped
    yield "mix", mix


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("table_len", [1, 2, 64, 1000])
def test_count_indices(fname, table_len):
    p, fid = modulus(fname), O.FID[fname]
    pattern = O.gen_scalars(fid, 79, table_len + GUARD, montgomery=True).copy()
    pattern[:table_len] = 0xFFFFFFFFFFFFFFFF                 # every 32-bit word of the cells the entry must clear and rewrite
    for n in (0, 1, 63, 64, 65, 4097):
        for name, idx in index_sets(n, table_len, 100 * table_len + n):
            assert idx.dtype == np.uint32 and idx.shape == (n,)
            m = R.counts([int(i) for i in idx], table_len)
            skipped = int((idx >= table_len).sum())
            assert sum(m) == n - skipped and (name != "all-out-of-range" or skipped == n) and (name != "all-equal" or m[-1] == n)
            if name == "mix" and n >= 63:
                assert 0 < skipped < n
            want = S.encode(m, p)
            out = A.DeviceVec.from_host(fname, pattern)
            d_idx = A.DeviceVec(fname, n // 8 + 1)            # 32 bytes per element: room for n uint32
            if n:
                check(lib().ark_hip_memcpy_h2d(d_idx.ptr, idx.ctypes.data_as(C.c_void_p), idx.nbytes), "ark_hip_memcpy_h2d")
            check(lib().ark_hip_fr_count_indices_device(out.field, d_idx.ptr if n else None, n, out.ptr, table_len), "ark_hip_fr_count_indices_device")
            got = out.to_host()
            assert np.array_equal(got[:table_len], want), (n, name, np.nonzero((got[:table_len] != want).any(axis=1))[0][:5])
            assert np.array_equal(got[table_len:], pattern[table_len:]), (n, name, "the guard region was written")
            out.free()
            d_idx.free()
            # the mirror: an extension for a power of two, else a vector
            mv = MLE.count_indices(fname, idx, table_len)
            if table_len & (table_len - 1) == 0:
                assert isinstance(mv, MLE) and 1 << mv.num_vars == table_len
                assert np.array_equal(mv.to_evaluations(), want), (n, name, "mirror")
            else:
                assert isinstance(mv, A.DeviceVec) and np.array_equal(mv.to_host(), want), (n, name, "mirror")
            mv.free()
    # the output on the indices is refused
    buf = A.DeviceVec(fname, 64)
    f = lib().ark_hip_fr_count_indices_device
    assert f(buf.field, buf.ptr, 16, buf.ptr, 2) == ERR_ARG
    assert f(buf.field, C.c_void_p(buf.ptr.value + 32), 8, buf.ptr, 2) == ERR_ARG
    buf.free()


# ---- the layered proof -----------------------------------------------------------------------------------------------
def prove_and_verify(fname, num, den, ncanon, dcanon):
    """FractionalSum.prove with transcript-derived challenges, accepted by the model's verifier; -> (proof, canonical root)"""
    p = modulus(fname)
    nv = den.num_vars
    has_num = num is not None
    device_challenge, model_challenge = R.hash_challenge(p)
    before = den.to_evaluations(), (num.to_evaluations() if has_num else None)
    proof = A.FractionalSum(num, den).prove(device_challenge)
    root, layers, point = R.decode_proof(proof, p)
    assert root == R.tree(None if ncanon is None else list(ncanon), list(dcanon), p)[0], "root"
    assert len(proof.layers) == nv and proof.point.shape == (nv, 4)
    assert all((sc is None) == (k == 0) for k, (sc, _) in enumerate(proof.layers))
    ok, vpoint, claim_n, claim_d = R.verify(nv, has_num, root, layers, model_challenge, p)
    assert ok, "the model's verifier rejects"
    assert vpoint == point, "the proof's point is the transcript's"
    assert np.array_equal(den.evaluate(proof.point), S.encode([claim_d], p)[0]), "den(point) on the device is the verifier's last claim"
    assert claim_d == mle_ref.evaluate(list(dcanon), point, p)
    if has_num:
        assert np.array_equal(num.evaluate(proof.point), S.encode([claim_n], p)[0]), "num(point) on the device is the verifier's last claim"
        assert np.array_equal(num.to_evaluations(), before[1]), "numerators changed"
    else:
        assert claim_n == 1 or nv == 0
    assert np.array_equal(den.to_evaluations(), before[0]), "denominators changed"
    return proof, root


@pytest.mark.parametrize("has_num", [True, False])
@pytest.mark.parametrize("fname,nv", [(f, nv) for f in FR for nv in (0, 1, 2, 3, 9)] + [("BLS12_381_FR", 12)])
def test_proof(fname, nv, has_num):
    kind = "planted" if nv in (3, 12) else "last-zero" if nv == 2 else "random"
    da, dcanon = table(fname, nv, kind)
    na, ncanon = table(fname, nv, "random" if kind == "last-zero" else kind, seed=1) if has_num else (None, None)
    den = MLE.from_evaluations(fname, nv, da)
    num = MLE.from_evaluations(fname, nv, na) if has_num else None
    proof, root = prove_and_verify(fname, num, den, ncanon, dcanon)
    if nv == 9:                                        # the model's own prover writes the same proof
        p = modulus(fname)
        want = R.prove(None if ncanon is None else list(ncanon), list(dcanon), R.hash_challenge(p)[1], p)
        got = R.decode_proof(proof, p)
        assert (want[0], want[2]) == (got[0], got[2]) and want[1] == got[1]
    den.free()
    if has_num:
        num.free()


# ---- a lookup end to end ---------------------------------------------------------------------------------------------
def test_lookup_end_to_end():
    """sum_i 1 / (gamma + w_i) = sum_j m_j / (gamma + t_j): m from count_indices, the denominators from
    ark_hip_fr_lincomb_device, both layered proofs accepted, and the roots agree as fractions; not so once a witness cell
    holds a value outside the table"""
    fname = "BLS12_381_FR"
    p = modulus(fname)
    t, idx, gamma, outside = R.lookup_case(p)      # tests/test_fraction_sum_host.py checks the seeds on the model
    one = G.mont_ints([1], p).reshape(-1, 4)
    g = G.enc(gamma, p)
    m = MLE.count_indices(fname, idx, 64)
    mcanon = R.counts([int(i) for i in idx], 64)
    assert np.array_equal(m.to_evaluations(), S.encode(mcanon, p))
    tm = MLE.from_evaluations(fname, 6, S.encode(t, p))
    tden = MLE.linear_combination([tm], one, g)
    tcanon = [(gamma + v) % p for v in t]
    assert np.array_equal(tden.to_evaluations(), S.encode(tcanon, p))
    _, (pt, qt) = prove_and_verify(fname, m, tden, mcanon, tcanon)
    for altered in (False, True):
        w = [t[i] for i in idx]
        if altered:
            w[77] = outside                            # the index array, and with it m, stays
        wm = MLE.from_evaluations(fname, 9, S.encode(w, p))
        wden = MLE.linear_combination([wm], one, g)
        wcanon = [(gamma + v) % p for v in w]
        assert np.array_equal(wden.to_evaluations(), S.encode(wcanon, p))
        _, (pw, qw) = prove_and_verify(fname, None, wden, None, wcanon)
        assert (pw * qt % p == pt * qw % p) == (not altered), altered
        wm.free()
        wden.free()
    for x in (m, tm, tden):
        x.free()
