"""Prefix products, sums and ratio accumulators on device vectors (ark_hip_fr_prefix_product_device, _sum_device,
_ratio_device) through the Python mirror, limb for limb against the big-integer model of tests/prefix_scan_ref.py -- never
against the code under test.  Outputs are canonical Montgomery residues: no tolerance anywhere.

At the two level seams (tile^2 and tile^2 + 1, about 4 million elements) the big-integer loop is replaced by the recurrence
itself: element 0 is compared directly and out[i + 1] = out[i] (op) a[i + 1] is evaluated for every i by ONE call of the
existing pointwise entries on views shifted by one element, then compared on the host."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd._lib import lib
import oracle_lib as O
import prefix_scan_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
OPS = {"product": 0, "sum": 1, "ratio": 2}
T = A.prefix_scan_plan("product", 0)[0]
TR = A.prefix_scan_plan("ratio", 0)[0]
SIZES = [0, 1, 2, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, (1 << 16) + 3]
SEAMS = [T * T, T * T + 1]
CASES = [(f, n) for f in FR for n in SIZES] + [("BLS12_381_FR", n) for n in SEAMS]
RSIZES = sorted(set(SIZES) | {TR - 1, TR, TR + 1, 3 * TR + 5})
RCASES = [(f, n) for f in FR for n in RSIZES] + [("BLS12_381_FR", n) for n in (TR * TR, TR * TR + 1)]


def test_the_seam_sizes_are_where_the_plan_says():
    for op, t in (("product", T), ("sum", T), ("ratio", TR)):
        assert A.prefix_scan_plan(op, 0) == (t, 1)
        assert [A.prefix_scan_plan(op, n)[1] for n in (t, t + 1, t * t, t * t + 1)] == [1, 2, 2, 3]


@functools.lru_cache(maxsize=None)
def field(fname):
    return R.Field(fname)


def vector(fname, n, seed, tile, zeros):
    """n random stored values; planted: one, the value -1, the largest residue p - 1, and both sides of every tile seam.
    zeros: also zeros, anywhere (the sum); otherwise the vector is free of them (a zero would hide a wrong carry behind it)"""
    f = field(fname)
    a = O.gen_scalars(O.FID[fname], seed, max(n, 1), montgomery=True)[:n].copy()
    special = R.limbs([f.one, f.enc(-1), f.p - 1])
    if n >= 8:
        a[1:4] = special
    for s in range(tile, n, tile):                    # both sides of every tile seam
        a[s - 1] = special[(s // tile) % 3]
        a[s] = special[(s // tile + 1) % 3]
    a[~a.any(axis=1)] = special[0]                    # a random zero (never seen; the guarantee is explicit)
    if zeros and n >= 8:
        a[5] = 0
        a[n // 2] = 0
        a[n - 1] = 0
        if n > tile + 1:
            a[tile - 1] = 0
            a[tile + 1] = 0
    return a


def scan_raw(entry, v, exclusive, out, total):
    return getattr(lib(), entry)(v.field, v.ptr, v.len, exclusive, out.ptr, None if total is None else total.ctypes.data_as(C.c_void_p))


def check_recurrence(fname, op, a, da, out, exclusive, total):
    """out[0] and out[i + 1] = out[i] (op) a[i + 1 - exclusive] for every i, the latter by one pointwise call on shifted views"""
    f = field(fname)
    n = a.shape[0]
    L = lib()
    pointwise = L.ark_hip_fr_mul_device if op == "product" else L.ark_hip_fr_add_device
    combine = f.mul if op == "product" else (lambda x, y: (x + y) % f.p)
    ident = f.one if op == "product" else 0
    got = out.to_host()
    first = R.ints(got[:1])[0]
    assert first == (ident if exclusive else R.ints(a[:1])[0]), "element 0"
    step = A.DeviceVec(fname, n - 1, _zero=False)
    shift = 0 if exclusive else 32                    # exclusive: out[i + 1] = out[i] a[i]; inclusive: out[i + 1] = out[i] a[i + 1]
    assert pointwise(da.field, out.ptr, C.c_void_p(da.ptr.value + shift), step.ptr, n - 1) == 0
    want_tail = step.to_host()
    step.free()
    assert np.array_equal(got[1:], want_tail), ("recurrence", np.nonzero((got[1:] != want_tail).any(axis=1))[0][:5])
    if op == "product":
        assert got.any(axis=1).all(), "a zero output"
    last = R.ints(got[n - 1:])[0]
    assert R.ints(total.reshape(1, 4))[0] == (combine(last, R.ints(a[n - 1:])[0]) if exclusive else last), "total"
    return got


@pytest.mark.parametrize("op", ["product", "sum"])
@pytest.mark.parametrize("fname,n", CASES)
def test_prefix_product_and_sum(op, fname, n):
    f = field(fname)
    a = vector(fname, n, 200 + n % 89, T, zeros=(op == "sum"))
    if op == "product":
        assert a.any(axis=1).all()
    entry = "ark_hip_fr_prefix_%s_device" % op
    model = R.prefix_product if op == "product" else R.prefix_sum
    da = A.DeviceVec.from_host(fname, a)
    big = n in SEAMS
    ai = None if big else R.ints(a)
    for exclusive in (False, True):
        # out of place: every element, the total, the input untouched
        out, total = (da.prefix_product if op == "product" else da.prefix_sum)(exclusive=exclusive)
        assert out is not da and len(out) == n
        if big:
            want = check_recurrence(fname, op, a, da, out, exclusive, total)
        else:
            w, t = model(f, ai, exclusive)
            if op == "product":
                assert all(w) and t, "an expected output is zero"
            want, want_total = R.limbs(w), R.limbs([t])[0]
            got = out.to_host()
            assert np.array_equal(got, want), (exclusive, "out of place", np.nonzero((got != want).any(axis=1))[0][:5])
            assert np.array_equal(total, want_total), (exclusive, "total")
        want_total = total.copy()
        assert np.array_equal(da.to_host(), a), (exclusive, "input changed")
        out.free()
        # in place
        w1 = da.clone()
        o1, t1 = (w1.prefix_product if op == "product" else w1.prefix_sum)(exclusive=exclusive, in_place=True)
        assert o1 is w1 and len(w1) == n
        assert np.array_equal(w1.to_host(), want), (exclusive, "in place")
        assert np.array_equal(t1, want_total), (exclusive, "in place total")
        w1.free()
        # out_total = NULL: asynchronous, the same vector after ark_hip_synchronize
        o2 = A.DeviceVec(fname, n)
        assert scan_raw(entry, da, int(exclusive), o2, None) == 0
        assert lib().ark_hip_synchronize() == 0
        assert np.array_equal(o2.to_host(), want), (exclusive, "out_total = NULL")
        o2.free()
    da.free()


def check_ratio_recurrence(fname, num, den, dnum, dden, out, last):
    """out[0] = 1 and out[i + 1] den[i] = out[i] num[i] for every i, by two pointwise products on views"""
    f = field(fname)
    n = num.shape[0]
    L = lib()
    got = out.to_host()
    assert R.ints(got[:1])[0] == f.one, "out[0] = 1"
    lhs, rhs = A.DeviceVec(fname, n - 1, _zero=False), A.DeviceVec(fname, n - 1, _zero=False)
    assert L.ark_hip_fr_mul_device(out.field, C.c_void_p(out.ptr.value + 32), dden.ptr, lhs.ptr, n - 1) == 0
    assert L.ark_hip_fr_mul_device(out.field, out.ptr, dnum.ptr, rhs.ptr, n - 1) == 0
    a, b = lhs.to_host(), rhs.to_host()
    lhs.free()
    rhs.free()
    assert np.array_equal(a, b), ("recurrence", np.nonzero((a != b).any(axis=1))[0][:5])
    assert got.any(axis=1).all(), "a zero output"
    z_last, n_last, d_last = (R.ints(x[n - 1:])[0] for x in (got, num, den))
    assert f.mul(R.ints(last.reshape(1, 4))[0], d_last) == f.mul(z_last, n_last), "last"
    return got


@pytest.mark.parametrize("fname,n", RCASES)
def test_prefix_ratio(fname, n):
    f = field(fname)
    num, den = vector(fname, n, 300 + n % 83, TR, zeros=False), vector(fname, n, 400 + n % 79, TR, zeros=False)[::-1].copy()
    assert num.any(axis=1).all() and den.any(axis=1).all()
    dnum, dden = A.DeviceVec.from_host(fname, num), A.DeviceVec.from_host(fname, den)
    out, last = dnum.prefix_ratio(dden)
    assert len(out) == n and out is not dnum and out is not dden
    if n >= TR * TR:
        want = check_ratio_recurrence(fname, num, den, dnum, dden, out, last)
        want_last = last.copy()
    else:
        w, t = R.prefix_ratio(f, R.ints(num), R.ints(den))
        assert all(w) and t, "an expected output is zero"
        want, want_last = R.limbs(w), R.limbs([t])[0]
        got = out.to_host()
        assert np.array_equal(got, want), ("out of place", np.nonzero((got != want).any(axis=1))[0][:5])
        assert np.array_equal(last, want_last), "last"
    assert np.array_equal(dnum.to_host(), num) and np.array_equal(dden.to_host(), den), "input changed"
    out.free()
    # d_out IS d_num, d_out IS d_den
    for which in (0, 1):
        cn, cd = dnum.clone(), dden.clone()
        o, l = cn.prefix_ratio(cd, out=(cn, cd)[which])
        assert o is (cn, cd)[which]
        assert np.array_equal(o.to_host(), want), ("aliased with", ("num", "den")[which])
        assert np.array_equal(l, want_last)
        assert np.array_equal((cd, cn)[which].to_host(), (den, num)[which]), "the other input changed"
        cn.free()
        cd.free()
    # out_last = NULL: asynchronous
    o2 = A.DeviceVec(fname, n)
    assert lib().ark_hip_fr_prefix_ratio_device(dnum.field, dnum.ptr, dden.ptr, n, o2.ptr, None) == 0
    assert lib().ark_hip_synchronize() == 0
    assert np.array_equal(o2.to_host(), want), "out_last = NULL"
    for v in (o2, dnum, dden):
        v.free()


# ---- zeros ------------------------------------------------------------------------------------------------------------
def zero_places(tile):
    n = 3 * tile + 5
    return n, [(0,), (5,), (tile - 1,), (tile,), (tile + 3,), (n - 1,), (tile - 2, 2 * tile + 7), (3, 3 * tile + 1)]


@pytest.mark.parametrize("fname", FR)
def test_zeros_in_a_product(fname):
    f = field(fname)
    n, places = zero_places(T)
    base = vector(fname, n, 510, T, zeros=False)
    for at in places:
        a = base.copy()
        a[list(at)] = 0
        da = A.DeviceVec.from_host(fname, a)
        for exclusive in (False, True):
            w, t = R.prefix_product(f, R.ints(a), exclusive)
            first = at[0] + (1 if exclusive else 0)
            assert all(w[:first]) and not any(w[first:]) and t == 0           # exact before the zero, zero after it
            out, total = da.prefix_product(exclusive=exclusive)
            got = out.to_host()
            assert np.array_equal(got, R.limbs(w)), (at, exclusive, np.nonzero((got != R.limbs(w)).any(axis=1))[0][:5])
            assert not total.any(), (at, exclusive)
            out.free()
        da.free()


@pytest.mark.parametrize("fname", FR)
def test_zero_denominators_and_numerators(fname):
    f = field(fname)
    n, places = zero_places(TR)
    num, den = vector(fname, n, 520, TR, zeros=False), vector(fname, n, 521, TR, zeros=False)[::-1].copy()
    dnum = A.DeviceVec.from_host(fname, num)
    for at in places:
        d = den.copy()
        d[list(at)] = 0
        w, t = R.prefix_ratio(f, R.ints(num), R.ints(d))
        assert all(w[:at[0] + 1]) and not any(w[at[0] + 1:]) and t == 0      # exact up to AND INCLUDING the first zero's index
        dd = A.DeviceVec.from_host(fname, d)
        out, last = dnum.prefix_ratio(dd)
        got = out.to_host()
        assert np.array_equal(got, R.limbs(w)), (at, np.nonzero((got != R.limbs(w)).any(axis=1))[0][:5])
        assert not last.any(), at
        out.free()
        dd.free()
    dden = A.DeviceVec.from_host(fname, den)
    for at in ((0,), (TR + 3,), (n - 1,)):                                    # a zero numerator is just a value
        m = num.copy()
        m[list(at)] = 0
        w, t = R.prefix_ratio(f, R.ints(m), R.ints(den))
        assert all(w[:at[0] + 1]) and not any(w[at[0] + 1:]) and t == 0
        dm = A.DeviceVec.from_host(fname, m)
        out, last = dm.prefix_ratio(dden)
        assert np.array_equal(out.to_host(), R.limbs(w)), at
        assert not last.any()
        out.free()
        dm.free()
    # a zero numerator BEFORE a zero denominator, and after one
    m, d = num.copy(), den.copy()
    m[7] = 0
    d[TR + 1] = 0
    m[2 * TR] = 0
    w, t = R.prefix_ratio(f, R.ints(m), R.ints(d))
    dm, dd = A.DeviceVec.from_host(fname, m), A.DeviceVec.from_host(fname, d)
    out, last = dm.prefix_ratio(dd)
    assert np.array_equal(out.to_host(), R.limbs(w)) and np.array_equal(last, R.limbs([t])[0])
    for v in (out, dm, dd, dnum, dden):
        v.free()


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_permutation_argument_without_leaving_the_device():
    """A copy-constraint argument at 2^12 rows and 3 columns: num = prod_k (w_k + beta id_k + gamma) and den = prod_k (w_k + beta
    sigma_k + gamma) are built on the device with lincomb and fr_mul from a random permutation sigma of the cells that only
    moves a cell to one holding the same value; z = prefix_ratio(num, den) has z[0] = 1, closes (last = 1) and satisfies
    z[i + 1] den[i] = z[i] num[i] on every row.  With one cell changed the product no longer closes.  The vectors leave the
    device for the final comparison only."""
    fname = "BLS12_381_FR"
    f = field(fname)
    fid = O.FID[fname]
    L = lib()
    rows, cols = 1 << 12, 3
    cells = rows * cols
    rng = np.random.default_rng(2024)
    pool = O.gen_scalars(fid, 91, 64, montgomery=True)
    cls = rng.integers(0, 64, size=cells)
    values = pool[cls]                                                        # cell c = k rows + i holds pool[cls[c]]
    sigma = np.arange(cells)
    for v in range(64):                                                       # a random cycle through every class of equal cells
        members = rng.permutation(np.nonzero(cls == v)[0])
        sigma[members] = np.roll(members, 1)
    assert (cls[sigma] == cls).all() and (sigma != np.arange(cells)).sum() > cells // 2
    ids = R.limbs([f.enc(c + 1) for c in range(cells)])                       # distinct identities of the cells
    beta, gamma = O.gen_scalars(fid, 92, 2, montgomery=True)

    def accumulator(vals):
        w = [A.DeviceVec.from_host(fname, vals[k * rows:(k + 1) * rows]) for k in range(cols)]
        did = [A.DeviceVec.from_host(fname, ids[k * rows:(k + 1) * rows]) for k in range(cols)]
        dsg = [A.DeviceVec.from_host(fname, ids[sigma[k * rows:(k + 1) * rows]]) for k in range(cols)]
        coeffs = np.stack([R.limbs([f.one])[0], beta])

        def grand(tags):
            acc = None
            for k in range(cols):
                fac = A.DeviceVec(fname, rows, _zero=False)
                ptrs = (C.c_void_p * 2)(w[k].ptr.value, tags[k].ptr.value)
                assert L.ark_hip_fr_lincomb_device(fid, ptrs, 2, coeffs.ctypes.data_as(C.c_void_p), gamma.ctypes.data_as(C.c_void_p),
                                                   fac.ptr, rows) == 0
                if acc is None:
                    acc = fac
                else:
                    acc *= fac
                    fac.free()
            return acc
        num, den = grand(did), grand(dsg)
        z, last = num.prefix_ratio(den)
        lhs, rhs = A.DeviceVec(fname, rows - 1, _zero=False), A.DeviceVec(fname, rows - 1, _zero=False)
        assert L.ark_hip_fr_mul_device(fid, C.c_void_p(z.ptr.value + 32), den.ptr, lhs.ptr, rows - 1) == 0
        assert L.ark_hip_fr_mul_device(fid, z.ptr, num.ptr, rhs.ptr, rows - 1) == 0
        res = z.to_host(), last, lhs.to_host(), rhs.to_host(), num.to_host()[rows - 1], den.to_host()[rows - 1]
        for v in w + did + dsg + [num, den, z, lhs, rhs]:
            v.free()
        return res

    one = R.limbs([f.one])[0]
    z, last, lhs, rhs, n_last, d_last = accumulator(values)
    assert np.array_equal(z[0], one) and np.array_equal(last, one)
    assert np.array_equal(lhs, rhs)                                           # the recurrence on every row
    assert f.mul(f.one, R.ints(d_last.reshape(1, 4))[0]) == f.mul(R.ints(z[rows - 1:])[0], R.ints(n_last.reshape(1, 4))[0])   # and into `last`
    assert len(set(R.ints(z))) > rows // 2                                    # not a column of ones
    bad = values.copy()
    c = int(np.nonzero(sigma != np.arange(cells))[0][17])
    bad[c] = pool[(cls[c] + 1) % 64]
    z, last, lhs, rhs, _, _ = accumulator(bad)
    assert np.array_equal(z[0], one) and np.array_equal(lhs, rhs)
    assert not np.array_equal(last, one)


# ---- scratch -------------------------------------------------------------------------------------------------------------
def test_small_calls_on_poisoned_scratch():
    """tests/prefix_scan_scratch_child.py: every entry warm, then with every scratch buffer poisoned
    (ark_hip_test_scratch_poison), then on poisoned scratch left behind by a larger call: the model's results each time,
    nothing written past what was asked for"""
    env = dict(os.environ, ARK_HIP_LIB=os.path.join(ROOT, "algebra_amd", "libark_hip_test.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "prefix_scan_scratch_child.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "prefix-scan scratch ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
