"""Polynomial operations on device-resident vectors (ark_hip_poly_evaluate_device, _divide_linear_device,
_divide_by_vanishing_device, ark_hip_domain_lagrange_coefficients_device, ark_hip_fr_inner_product_device) through the
Python mirror, limb for limb against Python big integers and the oracle's field arithmetic -- never against the code
under test.  Outputs are canonical Montgomery residues: no tolerance anywhere.

Python side of the big-integer references: a Montgomery residue a R is used as the plain integer it is.  The recurrences
checked here are linear in the coefficients, so with the POINT converted to its canonical value z the Montgomery factor R
rides along: (a R) + z (s R) = (a + z s) R.  That avoids 4 million conversions per case."""
import ctypes as C

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd._lib import lib
import oracle_lib as O
import pyref
from poly_ops_ref import lagrange_reference, mont_list, synthetic_division, vanishing_reference

pytestmark = pytest.mark.gpu

FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]


def plan(n):
    t, lv = C.c_int(), C.c_int()
    assert lib().ark_hip_poly_scan_plan(n, C.byref(t), C.byref(lv)) == 0
    return t.value, lv.value


T = plan(0)[0]


def ints(a):
    """numpy [n, 4] uint64 -> list of the n integers the limbs spell (Montgomery residues as they are)"""
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def limbs(xs):
    if not xs:
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def enc(x, p):
    return pyref.to_mont(x % p, p)


def coefficients(fname, n, seed):
    """n random coefficients with zero, p - 1 (as a residue and as a value) and an all-zero tail planted"""
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    a = O.gen_scalars(fid, seed, max(n, 1), montgomery=True)[:n].copy()
    if n >= 8:
        a[1] = 0
        a[n // 2] = 0
        a[2] = pyref.to_limbs(p - 1, 4)               # the largest residue
        a[3] = enc(p - 1, p)                          # the value -1
        a[n - max(1, n // 16):] = 0                   # trailing zero coefficients: a device vector is not truncated
    if n >= 3 * T:
        a[T - 1] = pyref.to_limbs(p - 1, 4)           # the two sides of a tile seam
        a[T] = 0
        a[2 * T - 3:2 * T + 3] = 0
    return a


def points(fname, seed):
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    w = pyref.root_of_unity(fname, T.bit_length() - 1)   # order T: z^T = 1, every level above the first sees the point 1
    assert pow(w, T, p) == 1 and pow(w, T // 2, p) != 1
    return [("0", enc(0, p)), ("1", enc(1, p)), ("p-1", enc(p - 1, p)), ("random", O.gen_scalars(fid, seed, 1, montgomery=True)[0]),
            ("root of unity", enc(w, p))]


SEAMS = sorted({n for lv in (2, 3) for n in (T ** (lv - 1), T ** (lv - 1) + 1, T ** (lv - 1) + 2)})   # first n of each further level, +- 1
SIZES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, (1 << 16) + 3, 1 << 20]
CASES = [(f, n) for f in FR for n in SIZES] + [("BLS12_381_FR", n) for n in SEAMS if n not in SIZES]


def test_the_seam_sizes_are_where_the_plan_says():
    assert plan(T)[1] == 1 and plan(T + 1)[1] == 2 and plan(T * T)[1] == 2 and plan(T * T + 1)[1] == 3
    assert T * T + 1 in SEAMS and T + 1 in SEAMS


@pytest.mark.parametrize("fname,n", CASES)
def test_evaluate_and_divide_by_linear(fname, n):
    p = pyref.MODULI[fname][0]
    a = coefficients(fname, n, 100 + n % 97)
    cm = ints(a)
    dp = A.DeviceVec.from_host(fname, a)
    L = lib()
    for label, z in points(fname, 7 + n % 5):
        zc = pyref.from_mont(z, p)
        q_want, r_want = synthetic_division(cm, zc, p)
        if n <= 1 << 17:                                 # Horner on its own (beyond that the division's s[0] IS the Horner value)
            horner = 0
            for c in reversed(cm):
                horner = (horner * zc + c) % p
            assert horner == r_want
        r_want, q_want = pyref.to_limbs(r_want, 4), limbs(q_want)
        ev = dp.evaluate(z)
        assert np.array_equal(ev, r_want), (label, "evaluate")
        # out of place: every quotient coefficient, the remainder, and the input untouched
        q, rem = dp.divide_by_linear(z)
        assert len(q) == max(n, 1) - 1
        got = q.to_host()
        assert np.array_equal(got, q_want), (label, "quotient", np.nonzero((got != q_want).any(axis=1))[0][:5])
        assert np.array_equal(rem, r_want) and np.array_equal(rem, ev), (label, "remainder")
        assert np.array_equal(dp.to_host(), a), (label, "input changed")
        # in place: the same quotient, element n - 1 of the buffer left alone
        w = dp.clone()
        full = w.len
        q2, rem2 = w.divide_by_linear(z, in_place=True)
        assert q2 is w and len(w) == max(n, 1) - 1 and np.array_equal(rem2, r_want), (label, "in place")
        w.len = full                                     # look at the whole buffer again
        buf = w.to_host()
        assert np.array_equal(buf[:max(n, 1) - 1], q_want), (label, "in-place quotient")
        if n:
            assert np.array_equal(buf[n - 1], a[n - 1]), (label, "element n - 1 was written")
        # out_rem = NULL: asynchronous, the same quotient after ark_hip_synchronize
        q3 = A.DeviceVec(fname, max(n, 1) - 1)
        assert L.ark_hip_poly_divide_linear_device(dp.field, dp.ptr, n, z.ctypes.data_as(C.c_void_p), q3.ptr, None) == 0
        assert L.ark_hip_synchronize() == 0
        assert np.array_equal(q3.to_host(), q_want), (label, "out_rem = NULL")
        for v in (q, w, q3):
            v.free()
    dp.free()


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("m", [1, 2, 1 << 10, 1 << 16])
def test_divide_by_vanishing_poly(fname, m):
    fid = O.FID[fname]
    dom = A.Radix2EvaluationDomain.new(fname, m)
    coset = dom.get_coset(enc(3, pyref.MODULI[fname][0]))
    assert dom.size() == m and coset.size() == m
    for n in sorted({min(v, 1 << 20) for v in (0, m - 1, m, m + 1, 2 * m, 2 * m + 1, 3 * m + 5, 7 * m - 1)}):
        a = coefficients(fname, n, 300 + n % 89)
        q_want, r_want = vanishing_reference(fid, a, m)
        dp = A.DeviceVec.from_host(fname, a)
        for d in (dom, coset):                          # only the size of the domain enters: the divisor is x^m - 1 for both
            q, r = dp.divide_by_vanishing_poly(d)
            assert len(q) == max(n - m, 0) and len(r) == min(n, m)
            assert np.array_equal(q.to_host(), q_want), (m, n, "quotient")
            assert np.array_equal(r.to_host(), r_want), (m, n, "remainder")
            q.free()
            r.free()
        assert np.array_equal(dp.to_host(), a)
        dp.free()


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("log_n", list(range(15)) + [20])
def test_lagrange_coefficients(fname, log_n):
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    m = 1 << log_n
    g = pyref.root_of_unity(fname, log_n)
    base = A.Radix2EvaluationDomain.new(fname, m)
    rng = np.random.default_rng(1000 + log_n)
    for dom, h in ((base, 1), (base.get_coset(enc(3, p)), 3)):
        tau = int.from_bytes(rng.bytes(40), "little") % p
        want = mont_list(lagrange_reference(fname, log_n, h, tau), p)
        lv = dom.evaluate_all_lagrange_coefficients(enc(tau, p))
        assert len(lv) == m
        got = lv.to_host()
        assert np.array_equal(got, want), (log_n, h, np.nonzero((got != want).any(axis=1))[0][:5])
        assert np.array_equal(dom.evaluate_vanishing_polynomial(enc(tau, p)), enc(pow(tau, m, p) - pow(h, m, p), p))
        # P(tau) = sum_i L_i(tau) P(h g^i) for deg P < m, all of it on the device
        coeffs = O.gen_scalars(fid, 50 + log_n, m, montgomery=True)
        pv = A.DeviceVec.from_host(fname, coeffs)
        at_tau = pv.evaluate(enc(tau, p))
        ev = pv.clone().evaluate_over_domain(dom)
        assert np.array_equal(lv.inner_product(ev), at_tau), (log_n, h, "inner product identity")
        for v in (lv, pv, ev):
            v.free()
        # tau in the domain: exactly one coefficient is one, the others are zero
        for i in sorted({0, 1 % m, m // 2, m - 1}):
            t = h * pow(g, i, p) % p
            hot = dom.evaluate_all_lagrange_coefficients(enc(t, p))
            got = hot.to_host()
            want = np.zeros((m, 4), dtype=np.uint64)
            want[i] = enc(1, p)
            assert np.array_equal(got, want), (log_n, h, i)
            assert not dom.evaluate_vanishing_polynomial(enc(t, p)).any()
            hot.free()


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("n", [0, 1, 255, 4097, 1 << 20])
def test_inner_product(fname, n):
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    a, b = coefficients(fname, n, 21), coefficients(fname, n, 22)[::-1].copy()
    rinv = pow(pyref.R_of(p), -1, p)
    want = sum(x * y for x, y in zip(ints(a), ints(b))) * rinv % p      # (a R)(b R) / R = (a b) R
    da, db = A.DeviceVec.from_host(fname, a), A.DeviceVec.from_host(fname, b)
    assert np.array_equal(da.inner_product(db), pyref.to_limbs(want, 4))
    assert np.array_equal(da.to_host(), a) and np.array_equal(db.to_host(), b)
    longer = A.DeviceVec(fname, n + 1)
    with pytest.raises(ValueError):
        da.inner_product(longer)
    for v in (da, db, longer):
        v.free()


@pytest.mark.parametrize("log_n", [12, 16])
def test_kzg_commit_open_verify_without_leaving_the_device(log_n):
    """C = <srs, p>; (q, y) = p / (x - z) in place; W = <srs[:n-1], q>; then C - y G == (tau - z) W.  After the one upload of p
    neither p nor q is copied to the host: the MSMs read the Montgomery coefficients where the division left them."""
    import torch
    cname, fname = "BLS12_381_G1", "BLS12_381_FR"
    cid, fid, r = O.CID[cname], O.FID[fname], pyref.MODULI[fname][0]
    fw = O.fe_words(cid)
    n = 1 << log_n
    L = lib()
    rng = np.random.default_rng(77 + log_n)
    tau, z = (int.from_bytes(rng.bytes(40), "little") % r for _ in range(2))
    G = O.generator(cid)
    one = O.field_const(O.curve_info(cid)[0], 1)
    pw, powers = 1, []
    for _ in range(n):
        powers.append(pw)
        pw = pw * tau % r
    srs = A.batch_mul(cid, np.concatenate([G, one]), torch.from_numpy(mont_list(powers, r).view(np.int64)).cuda())   # tau^i G, affine, on the device
    p = A.DeviceVec.from_host(fname, O.gen_scalars(fid, 5, n, montgomery=True))

    def commit(vec, count):
        out = np.zeros(3 * fw, dtype=np.uint64)
        assert L.ark_hip_msm_sw_device(cid, srs.data_ptr(), vec.ptr, count, 1, out.ctypes.data_as(C.c_void_p)) == 0
        return out

    torch.cuda.synchronize()
    Cm = commit(p, n)
    q, y = p.divide_by_linear(enc(z, r), in_place=True)
    assert q is p and len(q) == n - 1
    W = commit(q, n - 1)
    yc = pyref.from_mont(y, r)
    lhs = O.point_op(cid, "jac_add", Cm, O.scalar_mul(cid, G, pyref.to_limbs((-yc) % r, 4)))
    rhs = O.scalar_mul(cid, O.to_affine(cid, W), pyref.to_limbs((tau - z) % r, 4))
    assert np.array_equal(O.to_affine(cid, lhs), O.to_affine(cid, rhs))
    assert O.to_affine(cid, W).any()
