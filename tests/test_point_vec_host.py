"""CPU-side checks of the point-vector entries (no GPU needed): ark_hip_sw_mul(_device), ark_hip_sw_add_device and
ark_hip_sw_fold_device are C ABI with the same arity in the header, `_lib.SYMBOLS`, ark-hip-sys and ark_hip.hpp; argument
errors come before any device is looked for; and the HOST builds of the per-lane functions the kernels run (csrc/pointvec.cuh:
pv_chain_point, pv_add_point, behind ark_hip_test_host_sw_mul / _add / _fold) give the oracle's group elements on all five
curves -- affine forms compared bit for bit.  Points outside the prime-order subgroup are checked against the unreduced
Python-integer ladder of tests/check_fixtures.py.  The kernels are checked on the GPU by tests/test_gpu_point_vec.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from algebra_amd import _lib
import check_fixtures as CF
import oracle_lib as O
import point_fixtures as PF
import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = {"ark_hip_sw_mul_device": 8, "ark_hip_sw_mul": 8, "ark_hip_sw_add_device": 6, "ark_hip_sw_fold_device": 9}
HOOKS = {"ark_hip_test_host_sw_mul": 9, "ark_hip_test_host_sw_add": 6, "ark_hip_test_host_sw_fold": 10}
ERR_ARG = -1
AFFINE, PROJECTIVE = 0, 1
CURVES = O.CURVES
G1 = ("BN254_G1", "BLS12_381_G1", "BLS12_377_G1")
A4 = np.array([0xA11CE, 1, 2, 0], dtype=np.uint64)
B4 = np.array([0xB0B, 3, 0, 0], dtype=np.uint64)
NPTS = 40


def impls(cname):
    """0: the form the device entry runs by default (carry-free for G1, saturated for G2); 1: saturated (differs for G1 only)"""
    return (0, 1) if cname in G1 else (0,)


def limbs4(k):
    return P.to_limbs(k, 4).astype(np.uint64)


def mont4(cname, k):
    r = PF.curve(cname).r
    return limbs4((k % r) * P.R_of(r) % r)


def edge_scalars(r):
    """the digit-recoding carries and the [-8, 7] boundaries of the signed 4-bit windows, the group order's neighbourhood and
    the extremes of 256 bits"""
    return [0, 1, 2, 7, 8, 9, 15, 16, 17, r - 1, r, r + 1, 1 << 255, (1 << 256) - 1, int("7" * 64, 16), int("8" * 64, 16),
            int("F" * 64, 16)]


def unreduced_doubling_scalar(r):
    """the construction of tests/test_gpu_msm_prepared.py: s = d 2^252 + (d 2^252 - r) with 0 <= d 2^252 - r < 2^252"""
    d = next(d for d in range(1, 16) if 0 <= (d << 252) - r < (1 << 252))
    s = (d << 252) + ((d << 252) - r)
    assert s < (1 << 256)
    return s


def recode(k):
    """the chain's digits, most significant first: [carry, d_63, .., d_0] with k = carry 16^64 + sum d_w 16^w, d_w in [-8, 7]"""
    v = k + int("8" * 64, 16)
    out = [v >> 256]
    for w in range(63, -1, -1):
        out.append(((v >> (4 * w)) & 15) - 8)
    assert out[0] in (0, 1) and sum(d << (4 * (64 - i)) for i, d in enumerate(out)) == k
    return out


def branch_events(ks, order):
    """(doublings, cancellations) the chain meets for a point of exact order `order` under the scalars ks (one table each, one
    joint chain): the accumulator is [m]P with m an integer mod order, so an addition of [d]P doubles iff m = d != 0 and cancels
    iff m = -d != 0 (mod order); a digit that is 0 mod order adds the identity."""
    digs = [recode(k) for k in ks]
    dbl = cancel = 0
    acc = 0
    for w in range(65):
        acc = acc * 16 % order
        for dg in digs:
            d = dg[w]
            if d % order == 0:
                continue
            if acc != 0:
                if (acc - d) % order == 0:
                    dbl += 1
                elif (acc + d) % order == 0:
                    cancel += 1
            acc = (acc + d) % order
    return dbl, cancel


def host_mul(cname, pts, form, scalars, mont, impl):
    cid = O.CID[cname]
    fw = O.fe_words(cid)
    pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, (2 if form == AFFINE else 3) * fw)
    sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    n = pts.shape[0]
    out = np.zeros((n, 3 * fw), dtype=np.uint64)
    rc = _lib.test_lib().ark_hip_test_host_sw_mul(cid, pts.ctypes.data_as(C.c_void_p), form, sc.ctypes.data_as(C.c_void_p), sc.shape[0],
                                                  int(mont), impl, n, out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out


def host_fold(cname, lo, hi, form, a, b, mont, impl):
    cid = O.CID[cname]
    fw = O.fe_words(cid)
    lo = np.ascontiguousarray(lo, dtype=np.uint64).reshape(-1, (2 if form == AFFINE else 3) * fw)
    hi = np.ascontiguousarray(hi, dtype=np.uint64).reshape(lo.shape)
    out = np.zeros((lo.shape[0], 3 * fw), dtype=np.uint64)
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    rc = _lib.test_lib().ark_hip_test_host_sw_fold(cid, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), form,
                                                   a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), int(mont), impl,
                                                   lo.shape[0], out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out


def host_add(cname, a, b, negate, out=None):
    cid = O.CID[cname]
    fw = O.fe_words(cid)
    a = a if out is a else np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 3 * fw)
    b = b if out is b else np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 3 * fw)
    if out is None:
        out = np.zeros_like(a)
    rc = _lib.test_lib().ark_hip_test_host_sw_add(cid, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), int(negate),
                                                  a.shape[0], out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out


def affine_of(cname, jac):
    cid = O.CID[cname]
    return O.to_affine(cid, jac).reshape(-1, 2 * O.fe_words(cid))


@functools.lru_cache(maxsize=None)
def subgroup_points(cname):
    pts = O.gen_bases(O.CID[cname], A4, B4, NPTS)
    pts.setflags(write=False)
    return pts


def oracle_mul(cname, pt_xy, k):
    """affine limbs of [k] P for a subgroup point: the oracle's scalar_mul of k mod r, through to_affine"""
    cid = O.CID[cname]
    if not np.any(pt_xy):
        return np.zeros(2 * O.fe_words(cid), dtype=np.uint64)
    return O.to_affine(cid, O.scalar_mul(cid, pt_xy, limbs4(k % PF.curve(cname).r)))


def jacobian(cname, xy, lam=None):
    """Jacobian limbs of affine limbs: z = 1, or z = lam (tests/point_fixtures.lift); the identity as (1, 1, 0)"""
    cv = PF.curve(cname)
    pt = cv.dec(xy)
    if pt is None:
        return PF.identity_rows(cname, 1, 0)[0]
    return PF.lift(cname, pt, cv.F.from_int(1) if lam is None else lam)


# ---- ABI --------------------------------------------------------------------------------------------------------------
def _decls(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char\*)\s+(ark_hip_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_the_entries_are_c_abi_and_the_hooks_are_hooks():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    i, j = hdr.index("#ifdef ARK_HIP_TEST_HOOKS"), hdr.index("#endif /* ARK_HIP_TEST_HOOKS */")
    public, hooks = _decls(hdr[:i] + hdr[j:]), _decls(hdr[i:j])
    L, T = _lib.lib(), _lib.test_lib()
    for name, arity in PUBLIC.items():
        assert public.get(name) == arity and name not in hooks, name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == arity, name
        assert hasattr(L, name), name
    for name, arity in HOOKS.items():
        assert hooks.get(name) == arity and name not in public, name
        assert name in _lib.TEST_SYMBOLS and len(_lib.TEST_SYMBOLS[name][1]) == arity, name
        assert hasattr(T, name) and not hasattr(L, name), name


def test_rust_and_cpp_mirrors_have_the_entries():
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    found = dict((n, len([a for a in args.split(",") if a.strip()]))
                 for n, args in re.findall(r"pub fn (ark_hip_\w+)\s*\(([^;]*?)\)\s*(?:->\s*[^;]+)?;", ext, flags=re.S))
    for name, arity in PUBLIC.items():
        assert found.get(name) == arity, name
    rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "points.rs")).read()
    for name in ("ark_hip_sw_mul_device", "ark_hip_sw_add_device", "ark_hip_sw_fold_device"):
        assert "sys::" + name + "(" in rs, name
    assert "pub struct DevicePoints" in rs and "DevicePoints" in open(os.path.join(ROOT, "rust", "ark-hip", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for name in PUBLIC:
        assert name + "(" in hpp, name
    assert "class DevicePoints" in hpp
    import algebra_amd
    assert callable(algebra_amd.DevicePoints)


# ---- argument validation without a device -----------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_is_looked_for():
    L = _lib.lib()
    vp = C.c_void_p
    base = 1 << 24                               # "device pointers" that are never dereferenced
    pts, sc, out = vp(base), vp(base + (1 << 22)), vp(base + (2 << 22))
    a = limbs4(3)
    ap = a.ctypes.data_as(vp)
    n = 8
    for curve in (-1, 5):
        assert L.ark_hip_sw_mul_device(curve, pts, AFFINE, sc, n, 1, n, out) == ERR_ARG
        assert L.ark_hip_sw_mul(curve, pts, AFFINE, sc, n, 1, n, out) == ERR_ARG
        assert L.ark_hip_sw_add_device(curve, pts, sc, 0, n, out) == ERR_ARG
        assert L.ark_hip_sw_fold_device(curve, pts, sc, AFFINE, ap, ap, 1, n, out) == ERR_ARG
        assert L.ark_hip_sw_mul_device(curve, pts, AFFINE, sc, 0, 1, 0, out) == ERR_ARG      # also with n = 0
    for form in (-1, 2):
        assert L.ark_hip_sw_mul_device(1, pts, form, sc, n, 1, n, out) == ERR_ARG
        assert L.ark_hip_sw_mul(1, pts, form, sc, n, 1, n, out) == ERR_ARG
        assert L.ark_hip_sw_fold_device(1, pts, sc, form, ap, ap, 1, n, out) == ERR_ARG
    for ns in (0, 2, n - 1, n + 1):
        assert L.ark_hip_sw_mul_device(1, pts, AFFINE, sc, ns, 1, n, out) == ERR_ARG
        assert L.ark_hip_sw_mul(1, pts, AFFINE, sc, ns, 1, n, out) == ERR_ARG
    for args in ((None, sc, out), (pts, None, out), (pts, sc, None)):
        assert L.ark_hip_sw_mul_device(1, args[0], AFFINE, args[1], n, 1, n, args[2]) == ERR_ARG
        assert L.ark_hip_sw_mul(1, args[0], AFFINE, args[1], n, 1, n, args[2]) == ERR_ARG
        assert L.ark_hip_sw_add_device(1, args[0], args[1], 0, n, args[2]) == ERR_ARG
        assert L.ark_hip_sw_fold_device(1, args[0], args[1], AFFINE, ap, ap, 1, n, args[2]) == ERR_ARG
    assert L.ark_hip_sw_fold_device(1, pts, sc, AFFINE, None, ap, 1, n, out) == ERR_ARG
    assert L.ark_hip_sw_fold_device(1, pts, sc, AFFINE, ap, None, 1, n, out) == ERR_ARG
    for off in (4, 8):                            # device pointers are 16-byte aligned
        for args in ((vp(base + off), sc, out), (pts, vp(sc.value + off), out), (pts, sc, vp(out.value + off))):
            assert L.ark_hip_sw_mul_device(1, args[0], AFFINE, args[1], n, 1, n, args[2]) == ERR_ARG
            assert L.ark_hip_sw_add_device(1, args[0], args[1], 0, n, args[2]) == ERR_ARG
            assert L.ark_hip_sw_fold_device(1, args[0], args[1], AFFINE, ap, ap, 1, n, args[2]) == ERR_ARG
    # partial overlap of out with an input (BLS12-381 G1: 96 B affine, 144 B projective); exact aliasing of an AFFINE input
    # is refused as well (other stride), exact aliasing of a Projective input is allowed -- and then only the device is missing
    part = vp(base + 144)
    assert L.ark_hip_sw_mul_device(1, pts, PROJECTIVE, sc, n, 1, n, part) == ERR_ARG
    assert L.ark_hip_sw_mul_device(1, part, PROJECTIVE, sc, n, 1, n, pts) == ERR_ARG
    assert L.ark_hip_sw_mul_device(1, pts, AFFINE, sc, n, 1, n, pts) == ERR_ARG
    assert L.ark_hip_sw_mul_device(1, pts, AFFINE, sc, n, 1, n, vp(base + 96)) == ERR_ARG
    assert L.ark_hip_sw_mul_device(1, pts, PROJECTIVE, sc, n, 1, n, vp(sc.value + 16)) == ERR_ARG     # out over the scalars
    assert L.ark_hip_sw_add_device(1, pts, sc, 0, n, part) == ERR_ARG
    assert L.ark_hip_sw_add_device(1, sc, pts, 1, n, part) == ERR_ARG
    assert L.ark_hip_sw_fold_device(1, pts, sc, PROJECTIVE, ap, ap, 1, n, part) == ERR_ARG
    assert L.ark_hip_sw_fold_device(1, sc, pts, PROJECTIVE, ap, ap, 1, n, part) == ERR_ARG
    assert L.ark_hip_sw_fold_device(1, pts, sc, AFFINE, ap, ap, 1, n, pts) == ERR_ARG
    hostbuf = np.zeros(n * 18 + 18, dtype=np.uint64)
    hp = hostbuf.ctypes.data
    assert L.ark_hip_sw_mul(1, vp(hp), PROJECTIVE, sc, n, 1, n, vp(hp + 144)) == ERR_ARG
    # n = 0 succeeds and touches nothing, whatever the pointers are
    assert L.ark_hip_sw_mul_device(1, None, AFFINE, None, 0, 1, 0, None) == 0
    assert L.ark_hip_sw_mul_device(1, None, AFFINE, None, 1, 0, 0, None) == 0
    assert L.ark_hip_sw_mul(1, None, PROJECTIVE, None, 1, 1, 0, None) == 0
    assert L.ark_hip_sw_add_device(4, None, None, 1, 0, None) == 0
    assert L.ark_hip_sw_fold_device(3, None, None, AFFINE, ap, ap, 0, 0, None) == 0
    # a well-formed call gets past the argument checks (exact aliasing included): without a GPU it reports NO_DEVICE
    from algebra_amd._lib import lib
    if lib().ark_hip_device_count() == 0:
        assert L.ark_hip_sw_mul_device(1, pts, PROJECTIVE, sc, 1, 1, n, pts) == -5
        assert L.ark_hip_sw_add_device(1, pts, sc, 1, n, pts) == -5
        assert L.ark_hip_sw_add_device(1, pts, sc, 1, n, sc) == -5
        assert L.ark_hip_sw_fold_device(1, pts, sc, PROJECTIVE, ap, ap, 1, n, sc) == -5
    T = _lib.test_lib()
    assert T.ark_hip_test_host_sw_mul(5, ap, AFFINE, ap, 1, 1, 0, 1, ap) == ERR_ARG
    assert T.ark_hip_test_host_sw_mul(1, ap, AFFINE, ap, 1, 1, 2, 1, ap) == ERR_ARG
    assert T.ark_hip_test_host_sw_fold(1, ap, ap, 2, ap, ap, 1, 0, 1, ap) == ERR_ARG
    assert T.ark_hip_test_host_sw_add(-1, ap, ap, 0, 1, ap) == ERR_ARG


# ---- elementwise multiplication -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_mul_edge_scalars_shared_and_canonical(cname):
    """every edge scalar as ONE canonical scalar shared by 40 affine subgroup points (+ the identity (0, 0)), multiplied exactly"""
    cv = PF.curve(cname)
    pts = np.vstack([subgroup_points(cname), np.zeros((1, 2 * cv.fw), dtype=np.uint64)])
    for k in edge_scalars(cv.r) + [unreduced_doubling_scalar(cv.r)]:
        exp = np.stack([oracle_mul(cname, p, k) for p in pts[:6]])       # the oracle on a few, the twin forms against each other
        got = [affine_of(cname, host_mul(cname, pts, AFFINE, limbs4(k), False, impl)) for impl in impls(cname)]
        assert np.array_equal(got[0][:6], exp), (cname, hex(k))
        assert not got[0][NPTS].any()
        for g in got[1:]:
            assert np.array_equal(g, got[0]), (cname, hex(k))
        full = np.stack([oracle_mul(cname, p, k) for p in pts]) if k in (cv.r - 1, (1 << 256) - 1, int("8" * 64, 16)) else None
        if full is not None:
            assert np.array_equal(got[0], full), (cname, hex(k))


@pytest.mark.parametrize("form", [AFFINE, PROJECTIVE])
@pytest.mark.parametrize("cname", CURVES)
def test_mul_per_point_scalars_montgomery_and_canonical(cname, form):
    """one scalar per point: the edge scalars planted among 40 random ones, as Montgomery Fr and as canonical integers; Affine
    input, and Projective input with z != 1 and both encodings of the identity"""
    cid = O.CID[cname]
    cv = PF.curve(cname)
    fid = O.curve_info(cid)[1]
    rnd = [P.from_limbs(s) for s in O.gen_scalars(fid, 7, NPTS)]
    ks = edge_scalars(cv.r) + rnd
    n = len(ks)
    base = subgroup_points(cname)
    xy = np.stack([base[i % NPTS] for i in range(n)])
    ident = (3, n - 1)
    xy[list(ident)] = 0
    if form == AFFINE:
        pts = xy
    else:
        lams = PF.lambdas(cname, n, 11)
        pts = np.stack([jacobian(cname, xy[i], lams[i]) for i in range(n)])
        pts[n - 1] = PF.identity_rows(cname, 2, 5)[1]                    # (x, y, 0) with arbitrary x, y
    exp = np.stack([oracle_mul(cname, xy[i], ks[i]) for i in range(n)])
    canon = np.stack([limbs4(k) for k in ks])
    mont = np.stack([mont4(cname, k) for k in ks])
    for impl in impls(cname):
        assert np.array_equal(affine_of(cname, host_mul(cname, pts, form, canon, False, impl)), exp), (cname, impl)
        assert np.array_equal(affine_of(cname, host_mul(cname, pts, form, mont, True, impl)), exp), (cname, impl)


@pytest.mark.parametrize("cname", CURVES)
def test_mul_reaches_the_doubling_and_cancellation_branches(cname):
    """k = r + 2 d with d = the signed low digit of -r makes the last addition meet the accumulator's own point (it must
    double); k = r makes it meet the opposite point (it must land on the identity).  branch_events() proves both from the
    digits.  Points outside the subgroup and of small order (tests/check_fixtures.py) reach the same branches in the middle
    of the chain; their expected values are the unreduced Python-integer ladder's."""
    cv = PF.curve(cname)
    r = cv.r
    d0 = ((-r + 8) % 16) - 8
    k_dbl = r + 2 * d0
    assert recode(k_dbl)[-1] == d0 and d0 != 0
    assert branch_events([k_dbl], r) == (1, 0)
    assert branch_events([r], r) == (0, 1)
    pts = subgroup_points(cname)[:4]
    for k, want in ((k_dbl, None), (r, "identity")):
        exp = np.stack([oracle_mul(cname, p, k) for p in pts])
        for impl in impls(cname):
            got = affine_of(cname, host_mul(cname, pts, AFFINE, limbs4(k), False, impl))
            assert np.array_equal(got, exp), (cname, hex(k), impl)
            if want == "identity":
                assert not got.any()
    planted = [q for q in CF.planted(cname) if q.cls in ("off_subgroup", "small_order")]
    orders = {"order3_a": 3, "order3_b": 3, "order2": 2, "order11": 11, "order11_neg": 11, "order13": 13, "order13_neg": 13}
    rng = np.random.default_rng(0x90D + O.CID[cname])
    ks = [1, 2, 3, 8, 16, 17, r, (1 << 256) - 1, int("7" * 64, 16)] + [int.from_bytes(rng.bytes(32), "little") for _ in range(3)]
    seen = [0, 0]
    for q in planted[:8] if cname != "BN254_G1" else planted[:3]:
        pt = cv.dec(q.row)
        if q.name in orders:
            ev = [branch_events([k], orders[q.name]) for k in ks]
            seen[0] += sum(e[0] for e in ev)
            seen[1] += sum(e[1] for e in ev)
        exp = np.stack([cv.enc(CF.ladder(cv, pt, k)) for k in ks])
        rows = np.stack([q.row] * len(ks))
        canon = np.stack([limbs4(k) for k in ks])
        for impl in impls(cname):
            assert np.array_equal(affine_of(cname, host_mul(cname, rows, AFFINE, canon, False, impl)), exp), (cname, q.name, impl)
    if any(q.name in orders for q in planted):
        assert seen[0] > 0 and seen[1] > 0, "the small-order points no longer reach both branches"


# ---- elementwise addition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_add_all_pairs_both_signs_and_aliasing(cname):
    cid = O.CID[cname]
    cv = PF.curve(cname)
    base = subgroup_points(cname)
    Pt, Qt = cv.dec(base[0]), cv.dec(base[1])
    lam = PF.lambdas(cname, 1, 3)[0]
    twoP = cv.add(Pt, Pt)
    five = [PF.identity_rows(cname, 2, 9)[1], jacobian(cname, base[0]), jacobian(cname, cv.enc(cv.neg(Pt))), jacobian(cname, base[1], lam),
            PF.lift(cname, twoP, lam)]
    a = np.stack([x for x in five for _ in five])
    b = np.stack([y for _ in five for y in five])
    negb = b.copy()
    fw = cv.fw
    for i in range(len(negb)):
        negb[i, fw:2 * fw] = O.basefield_op(cid, "neg", negb[i, fw:2 * fw])
    for negate, bb in ((0, b), (1, negb)):
        exp = affine_of(cname, np.stack([O.point_op(cid, "jac_add", a[i], bb[i]) for i in range(len(a))]))
        assert np.array_equal(affine_of(cname, host_add(cname, a, b, negate)), exp), (cname, negate)
        a2 = a.copy()
        assert host_add(cname, a2, b, negate, out=a2) is a2                  # out aliases a
        assert np.array_equal(affine_of(cname, a2), exp)
        b2 = b.copy()
        host_add(cname, a, b2, negate, out=b2)                               # out aliases b
        assert np.array_equal(affine_of(cname, b2), exp)
    # the pairs cover every branch: O + O, O + X, X + O, P + P and 2P + 2P (doubling), P + (-P) (identity), P + Q
    pairs = affine_of(cname, host_add(cname, a, b, 0))
    assert not pairs[0].any() and not pairs[1 * 5 + 2].any() and np.array_equal(pairs[1 * 5 + 1], cv.enc(twoP))


# ---- fold -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [AFFINE, PROJECTIVE])
@pytest.mark.parametrize("cname", CURVES)
def test_fold_against_the_oracle(cname, form):
    cid = O.CID[cname]
    cv = PF.curve(cname)
    r = cv.r
    fid = O.curve_info(cid)[1]
    base = subgroup_points(cname)
    m = 6
    lo_xy, hi_xy = base[:m].copy(), base[m:2 * m].copy()
    lo_xy[2] = 0                                                             # identities on either side
    hi_xy[4] = 0
    u = P.from_limbs(O.gen_scalars(fid, 21, 1)[0])
    k = P.from_limbs(O.gen_scalars(fid, 22, 1)[0])
    ra, rb = (P.from_limbs(s) for s in O.gen_scalars(fid, 23, 2))
    cases = [(0, 0, False), (1, 0, False), (0, 1, False), (1, 1, False), (r - 1, 1, False), (pow(u, -1, r), u, False), (k, k, True),
             (ra, rb, False), ((1 << 256) - 1, r + 1, False)]
    lams = PF.lambdas(cname, 2 * m, 17)

    def enc(xy, off):
        return xy if form == AFFINE else np.stack([jacobian(cname, xy[i], lams[off + i]) for i in range(len(xy))])

    for a, b, opposite in cases:
        hx = hi_xy
        if opposite:                                                         # Lo = -Hi: every lane's two chains cancel
            hx = np.stack([cv.enc(cv.neg(cv.dec(x))) for x in lo_xy])
        exp = []
        for i in range(m):
            x = O.scalar_mul(cid, lo_xy[i], limbs4(a % r)) if lo_xy[i].any() else PF.identity_rows(cname, 1, 0)[0]
            y = O.scalar_mul(cid, hx[i], limbs4(b % r)) if hx[i].any() else PF.identity_rows(cname, 1, 0)[0]
            exp.append(O.point_op(cid, "jac_add", x, y))
        exp = affine_of(cname, np.stack(exp))
        if opposite:
            assert not exp.any()
        lo, hi = enc(lo_xy, 0), enc(hx, m)
        for impl in impls(cname):
            got = affine_of(cname, host_fold(cname, lo, hi, form, limbs4(a), limbs4(b), False, impl))
            assert np.array_equal(got, exp), (cname, hex(a), hex(b), impl)
            if a < r and b < r:
                got = affine_of(cname, host_fold(cname, lo, hi, form, mont4(cname, a), mont4(cname, b), True, impl))
                assert np.array_equal(got, exp), (cname, hex(a), hex(b), impl, "montgomery")
    # (k, k) with Lo = Hi: the second table's addition meets the first one's result -- the joint chain must double
    assert branch_events([5, 5], r)[0] > 0
    exp = affine_of(cname, np.stack([O.scalar_mul(cid, lo_xy[i], limbs4(10)) for i in (0, 1)]))
    for impl in impls(cname):
        got = affine_of(cname, host_fold(cname, enc(lo_xy[:2], 0), enc(lo_xy[:2], 0), form, limbs4(5), limbs4(5), False, impl))
        assert np.array_equal(got, exp)
