"""The kernels that work on ARRAYS of field and group elements outside the MSM, at their edges (GPU): the lane-batched
inversion (lane_batch_inverse, csrc/ec.cuh) behind `Evaluations /=`, batch_inverse, normalize_batch and batch_mul, under
every pattern of zeros a lane can meet and across the lane and workgroup seams; sw_add_affine_kernel on its identity,
doubling and cancellation branches; the transform over group elements on the two curves it never ran on and on inputs
that make its butterflies double and cancel; and the ARK_HIP_MSM_LAZY=0 build of batch_mul and the MSM in a process of
its own.  Expected values: tests/pyref.py (Python integers) wherever it is fast enough, the oracle for bulk scalar
multiplications.  Every comparison is limb for limb."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd._lib import check, lib
import oracle_lib as O
import point_fixtures as X
import pyref as P
from test_gpu_group_fft import _expected, test_group_fft_matches_the_transform_of_the_discrete_logs as _dlog_test

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR_FIELDS = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _host(t, cols):
    return t.cpu().numpy().view(np.uint64).reshape(-1, cols)


# ---- (a) field division and batch inversion -------------------------------------------------------------------------
def _fr_case(fname, n):
    """numerators and non-zero denominators as integers, and their Montgomery limbs"""
    p = P.MODULI[fname][0]
    rng = np.random.default_rng(0xD1 + 7 * n + O.FID[fname])
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % p
    num = [rnd() for _ in range(n)]
    den = [1 + rnd() % (p - 1) for _ in range(n)]
    for k, v in enumerate((1, p - 1, P.R_of(p))):          # spread over the lanes; whatever n holds of them
        if k * 3 < n:
            den[(k * 3 + n // 2) % n] = v
    if n > 1:
        num[1] = 0                                         # 0 / x = 0 with x != 0
    enc = lambda vals: np.stack([P.to_mont(v, p) for v in vals])
    return p, num, den, enc(num), enc(den)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("fname", FR_FIELDS)
def test_fr_div_and_batch_inverse_under_every_zero_pattern(fname, n):
    """fr_div_kernel: 8 values per lane, 128 lanes per workgroup -- the lane seam at 8 and the workgroup seam at 1024 (at
    1025 lanes 122..128 are ragged, lane 128 alone in the second workgroup).  In all three aliasing forms: `/=` (r = num),
    batch_inverse (r = den) and the C entries with an output buffer of their own."""
    fid = O.FID[fname]
    p, num, den, num_l, den_l = _fr_case(fname, n)
    assert [P.from_mont(row, p) for row in den_l[:4]] == den[:4] and [P.from_mont(row, p) for row in num_l[:4]] == num[:4]
    inv = [pow(d, -1, p) for d in den]
    quo_l = np.stack([P.to_mont(a * i % p, p) for a, i in zip(num, inv)])
    inv_l = np.stack([P.to_mont(i, p) for i in inv])
    masks = X.zero_masks(n, X.B_FR)
    assert len(masks) == 8 or n <= 9
    L = lib()
    for name, zero in masks.items():
        d_l, q_l, i_l = den_l.copy(), quo_l.copy(), inv_l.copy()
        d_l[zero] = 0                                      # a zero divisor gives zero
        q_l[zero] = 0
        i_l[zero] = 0
        a = A.DeviceVec.from_host(fid, num_l)
        b = A.DeviceVec.from_host(fid, d_l)
        a /= b                                             # r aliases num
        assert np.array_equal(a.to_host(), q_l), (fname, n, name, "/=")
        assert np.array_equal(b.to_host(), d_l), (fname, n, name, "/= left its divisor alone")
        b.batch_inverse()                                  # r aliases den
        assert np.array_equal(b.to_host(), i_l), (fname, n, name, "batch_inverse")
        a2 = A.DeviceVec.from_host(fid, num_l)
        b2 = A.DeviceVec.from_host(fid, d_l)
        r = A.DeviceVec.from_host(fid, np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
        check(L.ark_hip_fr_div_device(fid, a2.ptr, b2.ptr, r.ptr, n), "ark_hip_fr_div_device")
        assert np.array_equal(r.to_host(), q_l), (fname, n, name, "fr_div_device")
        r2 = A.DeviceVec.from_host(fid, np.full((n, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
        check(L.ark_hip_fr_inverse_device(fid, b2.ptr, r2.ptr, n), "ark_hip_fr_inverse_device")
        assert np.array_equal(r2.to_host(), i_l), (fname, n, name, "fr_inverse_device")
        assert np.array_equal(a2.to_host(), num_l) and np.array_equal(b2.to_host(), d_l), (fname, n, name, "operands")
        for v in (a, b, a2, b2, r, r2):
            v.free()


# ---- (b) normalize_batch --------------------------------------------------------------------------------------------
def _sizes(B):
    return [1, B - 1, B + 1, 128 * B - 1, 128 * B + 1]


_LIFTED = {}


def _lifted(cname):
    """128 B + 1 affine points of a Curve.add chain, each lifted to (x l^2, y l^3, l): computed once per curve"""
    if cname not in _LIFTED:
        n = 128 * X.lane_batch(cname) + 1
        chain = X.affine_chain(cname, n)
        lam = X.lambdas(cname, n, 0xB0 + O.CID[cname])
        cv = X.curve(cname)
        jac = np.stack([X.lift(cname, pt, l) for pt, l in zip(chain, lam)])
        aff = np.stack([cv.enc(pt) for pt in chain])
        jac.setflags(write=False)
        aff.setflags(write=False)
        _LIFTED[cname] = (jac, aff)
    return _LIFTED[cname]


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("cname", O.CURVES)
def test_normalize_batch_under_every_identity_pattern(cname, k):
    """sw_normalize_batch_kernel at n = 1, B - 1, B + 1, 128 B - 1, 128 B + 1 (B = 8, Fp2: 4): one lane, ragged lanes, a
    second workgroup.  Every input has z != 1 -- random, 1 is among them, p - 1, over Fp2 also z with c0 = 0 and with
    c1 = 0 -- and identities sit where the masks say, as (1, 1, 0) and as (x, y, 0) with arbitrary x, y."""
    cid = O.CID[cname]
    B = X.lane_batch(cname)
    n = _sizes(B)[k]
    jac_all, aff_all = _lifted(cname)
    masks = X.zero_masks(n, B)
    assert len(masks) == 8 or n <= B + 1
    for name, zero in masks.items():
        jac, exp = jac_all[:n].copy(), aff_all[:n].copy()
        jac[zero] = X.identity_rows(cname, zero.size, 5 + n)
        exp[zero] = 0
        got = _host(A.normalize_batch(cid, _dev(jac)), exp.shape[1])
        assert np.array_equal(got, exp), (cname, n, name, "device entry")
        assert np.array_equal(A.normalize_batch(cid, jac), exp), (cname, n, name, "host-pointer entry")


# ---- (c) batch_mul's batched normalisation --------------------------------------------------------------------------
@pytest.mark.parametrize("cname", O.CURVES)
def test_batch_mul_normalises_lanes_of_identities(cname):
    """xyzz_to_affine_batched_kernel behind batch_mul at n = 128 B + 1: scalar 0 (an identity among the results) over two
    whole lanes, in the last slot of every third lane and in every slot but the last of two lanes.  Then a base equal
    to the identity: every table entry is the identity, so EVERY lane of the table's normalisation inverts `one`."""
    cid = O.CID[cname]
    B = X.lane_batch(cname)
    n = 128 * B + 1
    masks = X.zero_masks(n, B)
    zero = np.unique(np.concatenate([masks[k] for k in ("lanes_0_and_last", "last_slot_of_lanes_1_mod_3",
                                                        "lanes_2_and_Lm2_but_last_slot")]))
    sf = O.curve_info(cid)[1]
    canon = O.gen_scalars(sf, 0xBA7C, n)
    assert canon.any(axis=1).all()
    canon[zero] = 0
    base = O.scalar_mul(cid, O.generator(cid), np.array([0xC0FFEE, 7, 0, 0], dtype=np.uint64))   # a Projective with z != 1
    exp = O.batch_mul(cid, base, canon)
    assert not exp[zero].any() and exp[np.setdiff1d(np.arange(n), zero)].any(axis=1).all()
    t = A.BatchMulPreprocessing(cid, base, n)
    got = t.batch_mul(canon, montgomery=False)
    t.free()
    assert np.array_equal(got, exp), cname
    for ident in X.identity_rows(cname, 2, 3):                       # (1, 1, 0) and (x, y, 0)
        t = A.BatchMulPreprocessing(cid, ident, n)
        got = t.batch_mul(canon, montgomery=False)
        t.free()
        assert got.shape == exp.shape and not got.any(), cname


# ---- (d) ark_hip_sw_add_affine_device -------------------------------------------------------------------------------
AT_DELTA = (0, 63, 64, 129)         # rows equal to delta: the doubling inside xyzz_madd, at both ends of both workgroups
AT_MINUS_DELTA = (1, 65, 128)       # rows equal to -delta: the sum is the identity, stored as (0, 0)
AT_IDENTITY = (2, 62, 66, 127)      # rows (0, 0): the sum is delta


@pytest.mark.parametrize("cname", O.CURVES)
def test_sw_add_affine_on_identity_equal_and_opposite_rows(cname):
    import torch
    cid = O.CID[cname]
    cv = X.curve(cname)
    n = 130                          # 128 lanes per workgroup: two workgroups
    chain = X.affine_chain(cname, n + 1)
    delta = chain[n]
    rows = list(chain[:n])
    for i in AT_DELTA:
        rows[i] = delta
    for i in AT_MINUS_DELTA:
        rows[i] = cv.neg(delta)
    for i in AT_IDENTITY:
        rows[i] = None
    inp = np.stack([cv.enc(r) for r in rows])
    L = lib()
    for d in (delta, None):          # delta = (0, 0): every row comes back as it went in, identities stay (0, 0)
        exp = np.stack([cv.enc(cv.add(r, d)) for r in rows])
        if d is None:
            assert np.array_equal(exp, inp)
        else:
            assert not exp[list(AT_MINUS_DELTA)].any() and np.array_equal(exp[2], cv.enc(delta))
        dl = np.ascontiguousarray(cv.enc(d))
        src = _dev(inp)
        dst = torch.full_like(src, 0x5A5A5A5A5A5A5A5A)
        torch.cuda.synchronize()
        check(L.ark_hip_sw_add_affine_device(cid, src.data_ptr(), dst.data_ptr(), n, dl.ctypes.data_as(C.c_void_p)), "out of place")
        assert np.array_equal(_host(dst, inp.shape[1]), exp), (cname, "out of place", d is None)
        assert np.array_equal(_host(src, inp.shape[1]), inp), (cname, "input untouched")
        check(L.ark_hip_sw_add_affine_device(cid, src.data_ptr(), src.data_ptr(), n, dl.ctypes.data_as(C.c_void_p)), "in place")
        assert np.array_equal(_host(src, inp.shape[1]), exp), (cname, "in place", d is None)


# ---- (e) the transform over group elements --------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [2, 5])
@pytest.mark.parametrize("cname", ["BLS12_377_G1", "BLS12_381_G2"])
def test_group_fft_on_the_remaining_curves(cname, log_n):
    """plain, coset and inverse against the transform of the discrete logs, as tests/test_gpu_group_fft.py has it for the
    other three curves"""
    _dlog_test(cname, log_n)


def _rescale(cname, jac_row, lam):
    """another Jacobian representative of the same point: (x l^2, y l^3, z l)"""
    F = X.curve(cname).F
    fw = X.curve(cname).fw
    x, y, z = (F.dec(jac_row[k * fw:(k + 1) * fw]) for k in range(3))
    l2 = F.mul(lam, lam)
    return np.concatenate([F.enc(F.mul(x, l2)), F.enc(F.mul(y, F.mul(l2, lam))), F.enc(F.mul(z, lam))])


def _neg_rows(cid, rows):
    fw = O.fe_words(cid)
    out = rows.copy()
    out[:, fw:2 * fw] = O.basefield_op(cid, "neg", np.ascontiguousarray(rows[:, fw:2 * fw])).reshape(-1, fw)
    return out


_GFFT_N = 256       # 128 butterflies per stage: two workgroups of 64 lanes
_GFFT_PTS = {}


def _gfft_points(cname):
    """128 distinct points [a_i] G as the oracle's scalar multiplication leaves them (z != 1), and the a_i"""
    if cname not in _GFFT_PTS:
        cid = O.CID[cname]
        r = X.curve(cname).r
        rng = np.random.default_rng(0xF7 + cid)
        dl = [1 + int.from_bytes(rng.bytes(40), "little") % (r - 1) for _ in range(_GFFT_N // 2)]
        assert len(set(dl) | {r - a for a in dl}) == _GFFT_N
        g = O.generator(cid)
        pts = np.stack([O.scalar_mul(cid, g, P.to_limbs(a, 4)) for a in dl])
        fw = O.fe_words(cid)
        one = np.zeros(fw, dtype=np.uint64)
        m1 = O.field_const(O.curve_info(cid)[0], 1)
        one[:m1.size] = m1
        assert not (pts[:, 2 * fw:] == one).all(axis=1).any()          # no z = 1 among them
        pts.setflags(write=False)
        _GFFT_PTS[cname] = (pts, dl)
    return _GFFT_PTS[cname]


def _gfft_pattern(cname, pattern):
    cid = O.CID[cname]
    r = X.curve(cname).r
    n, h = _GFFT_N, _GFFT_N // 2
    pts, dl = _gfft_points(cname)
    neg = _neg_rows(cid, pts)
    if pattern == "all_equal":
        # one point P, in a different representative at every odd index: lo == hi in every butterfly of the first stage (the
        # sum doubles, the difference is the identity and meets a twiddle), and again on the doubled points after it
        lam = X.lambdas(cname, n, 0x11)
        rows = np.stack([pts[0] if i % 2 == 0 else _rescale(cname, pts[0], lam[i]) for i in range(n)])
        scal = [dl[0]] * n
    elif pattern == "alternating":
        # P, -P, P, -P: stage 0 pairs equal points (i and i + n / 2 have the same parity), the last stage pairs P with -P
        rows = np.stack([pts[0] if i % 2 == 0 else neg[0] for i in range(n)])
        scal = [dl[0] if i % 2 == 0 else r - dl[0] for i in range(n)]
    elif pattern == "halves_opposite":
        # P_(i + n/2) = -P_i: every sum of stage 0 cancels, every difference doubles and is multiplied by its twiddle
        rows = np.concatenate([pts, neg])
        scal = dl + [r - a for a in dl]
    else:
        # P_(i + n/2) = P_i, distinct in the lower half: every sum of stage 0 doubles, every difference is the identity and
        # (for j != 0) is handed to the scalar multiplication with a non-trivial twiddle
        assert pattern == "halves_equal"
        rows = np.concatenate([pts, pts])
        scal = dl + dl
    return np.ascontiguousarray(rows), scal


@pytest.mark.parametrize("pattern", ["all_equal", "alternating", "halves_opposite", "halves_equal"])
@pytest.mark.parametrize("cname", ["BLS12_381_G1", "BN254_G1", "BLS12_377_G2"])
def test_group_fft_butterflies_that_double_and_cancel(cname, pattern, monkeypatch):
    """gfft_stage_kernel's xyzz_add on lo == hi and lo == -hi, and an identity difference with a non-trivial twiddle.  The
    inputs go in with z != 1; expected: the oracle's field transform of the discrete logs, one oracle scalar
    multiplication per output."""
    cid = O.CID[cname]
    sf = O.curve_info(cid)[1]
    n, log_n = _GFFT_N, 8
    rows, scal = _gfft_pattern(cname, pattern)
    fname = O.FIELDS[sf]
    dom = A.Radix2EvaluationDomain.new(fname, n)
    exp_f = _expected(cid, sf, scal, log_n, None, False)
    exp_i = _expected(cid, sf, scal, log_n, None, True)
    zero_rows = lambda e: np.flatnonzero(~e.any(axis=1))
    if pattern == "all_equal":          # [n] P at index 0 and identities elsewhere; the inverse leaves P at index 0
        assert zero_rows(exp_f).tolist() == list(range(1, n)) and zero_rows(exp_i).tolist() == list(range(1, n))
        assert np.array_equal(exp_i[0], O.to_affine(cid, rows[0]))
    got_f = dom.fft_group_in_place(cname, rows.copy())
    assert np.array_equal(A.into_affine(cid, got_f), exp_f), (cname, pattern, "forward")
    got_i = dom.fft_group_in_place(cname, rows.copy(), inverse=True)
    assert np.array_equal(A.into_affine(cid, got_i), exp_i), (cname, pattern, "inverse")
    if pattern == "halves_opposite":    # the same in slabs of 64 lanes: two launches per stage, one set of window tables
        monkeypatch.setenv("ARK_HIP_GFFT_SLAB_LOG", "6")
        slab_f = dom.fft_group_in_place(cname, rows.copy())
        slab_i = dom.fft_group_in_place(cname, rows.copy(), inverse=True)
        monkeypatch.delenv("ARK_HIP_GFFT_SLAB_LOG")
        assert np.array_equal(A.into_affine(cid, slab_f), exp_f), (cname, pattern, "forward, slabs")
        assert np.array_equal(A.into_affine(cid, slab_i), exp_i), (cname, pattern, "inverse, slabs")


# ---- the ARK_HIP_MSM_LAZY=0 kernels, in a process of their own ---------------------------------------------------------
def test_saturated_kernels_behind_the_lazy_switch_match_the_oracle():
    """ARK_HIP_MSM_LAZY is read once per process: tests/msm_saturated_child.py runs batch_mul and the MSM with it off."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "msm_saturated_child.py")], cwd=ROOT,
                         env=dict(os.environ, ARK_HIP_MSM_LAZY="0"), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stdout.rstrip().endswith("saturated-kernels ok"), (out.stdout[-1500:], out.stderr[-3000:])
