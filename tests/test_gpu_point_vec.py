"""The point-vector kernels on the GPU (csrc/pointvec.cuh through ark_hip_sw_mul_device / ark_hip_sw_mul / ark_hip_sw_add_device /
ark_hip_sw_fold_device and algebra_amd.DevicePoints) against the oracle, affine forms compared bit for bit: block and wave
edges on all five curves, per-point and shared scalars, both input forms, in place and out of place, the identity at lane 0,
at the last lane and over a whole wave, the scalars and points that force the doubling and cancellation branches, the slab
seams and the saturated form (child processes: tests/point_vec_child.py), the chunk seam of the host-slice entry, and the
round trip into the device MSM.  The expected values of a curve are computed once (n = NMAX) and shared by every size."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd._lib import check, lib
import check_fixtures as CF
import oracle_lib as O
import point_fixtures as PF
import pyref as P
import test_point_vec_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SIZES = (0, 1, 2, 63, 64, 65, 129, 1000)
NMAX = 1000
AFFINE, PROJECTIVE = 0, 1


class Data:
    pass


@functools.lru_cache(maxsize=None)
def data(cname):
    """NMAX subgroup points (affine and lifted to z != 1), per-point canonical scalars with the edge scalars and the
    branch-forcing ones planted at the block and wave edges, two shared scalars, and the oracle's results for all three"""
    cid = O.CID[cname]
    cv = PF.curve(cname)
    fid = O.curve_info(cid)[1]
    d = Data()
    d.cid, d.r, d.fw = cid, cv.r, cv.fw
    d.xy = O.gen_bases(cid, H.A4, H.B4, NMAX)
    lams = PF.lambdas(cname, NMAX, 29)
    d.jac = np.stack([PF.lift(cname, cv.dec(d.xy[i]), lams[i]) for i in range(NMAX)])
    ks = [P.from_limbs(s) for s in O.gen_scalars(fid, 0x5EED, NMAX)]
    d0 = ((-cv.r + 8) % 16) - 8
    special = H.edge_scalars(cv.r) + [cv.r + 2 * d0, H.unreduced_doubling_scalar(cv.r)]
    where = [0, 1, 62, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 255, 256, 511, 512, 998, 999]
    for i, k in zip(where, special):
        if i < NMAX:
            ks[i] = k
    d.ks = ks
    d.canon = np.stack([H.limbs4(k) for k in ks])
    d.mont = np.stack([H.mont4(cname, k) for k in ks])
    d.a, d.b = (P.from_limbs(s) for s in O.gen_scalars(fid, 0xF01D, 2))
    one = PF.identity_rows(cname, 1, 0)[0]

    def jmul(xy, k):
        return O.scalar_mul(cid, xy, H.limbs4(k % cv.r)) if k % cv.r else one

    d.exp_jac = np.stack([jmul(d.xy[i], ks[i]) for i in range(NMAX)])
    d.exp = H.affine_of(cname, d.exp_jac)
    d.ea_jac = np.stack([jmul(d.xy[i], d.a) for i in range(NMAX)])
    d.eb_jac = np.stack([jmul(d.xy[i], d.b) for i in range(NMAX)])
    d.ea = H.affine_of(cname, d.ea_jac)
    # fold of Lo = P_i, Hi = P_(i + 1 mod NMAX)
    d.hi = np.roll(np.arange(NMAX), -1)
    d.efold = H.affine_of(cname, np.stack([O.point_op(cid, "jac_add", d.ea_jac[i], d.eb_jac[d.hi[i]]) for i in range(NMAX)]))
    return d


def identity_lanes(n):
    """lane 0, the last lane, and the whole second wave"""
    s = {0, n - 1} if n else set()
    if n >= 129:
        s |= set(range(64, 128))
    return sorted(i for i in s if n > 2 or i == 0)


def points_of(cname, n, form, ident, idx=None):
    d = data(cname)
    idx = np.arange(n) if idx is None else idx[:n]
    src = (d.xy if form == AFFINE else d.jac)[idx].copy()
    if form == AFFINE:
        src[ident] = 0
    else:
        rows = PF.identity_rows(cname, max(len(ident), 1), 77)
        for j, i in enumerate(ident):
            src[i] = rows[j]
    return src


def got_affine(cname, pts):
    return H.affine_of(cname, pts.to_host()) if len(pts) else np.zeros((0, 2 * data(cname).fw), dtype=np.uint64)


def check_mul(cname, n, form, shared=False, montgomery=False, in_place=False):
    d = data(cname)
    ident = identity_lanes(n)
    v = A.DevicePoints.from_host(d.cid, points_of(cname, n, form, ident), affine=form == AFFINE)
    if shared:
        sc = (H.mont4(cname, d.a) if montgomery else H.limbs4(d.a)).reshape(1, 4)
        exp = d.ea[:n].copy()
    else:
        sc = (d.mont if montgomery else d.canon)[:n]
        exp = d.exp[:n].copy()
    exp[ident] = 0
    if n == 0 and not shared:
        sc = np.zeros((0, 4), dtype=np.uint64)
    out = v.mul(sc, montgomery=montgomery, in_place=in_place)
    assert (out is v) == in_place
    got = got_affine(cname, out)
    assert np.array_equal(got, exp), (cname, n, form, shared, montgomery, in_place, np.flatnonzero((got != exp).any(axis=1))[:8])


def check_fold(cname, n, form, montgomery=False, in_place=False):
    d = data(cname)
    ident = identity_lanes(n)
    lo = A.DevicePoints.from_host(d.cid, points_of(cname, n, form, ident), affine=form == AFFINE)
    hi = A.DevicePoints.from_host(d.cid, points_of(cname, n, form, [], d.hi), affine=form == AFFINE)
    exp = d.efold[:n].copy()
    for i in ident:                               # Lo_i = O: [b] Hi_i alone
        exp[i] = H.affine_of(cname, d.eb_jac[d.hi[i]])[0]
    a, b = (H.mont4(cname, k) if montgomery else H.limbs4(k) for k in (d.a, d.b))
    out = lo.fold(hi, a, b, montgomery=montgomery, in_place=in_place)
    got = got_affine(cname, out)
    assert np.array_equal(got, exp), (cname, n, form, montgomery, in_place, np.flatnonzero((got != exp).any(axis=1))[:8])


@pytest.mark.parametrize("cname", O.CURVES)
def test_mul_block_and_wave_edges(cname):
    for n in SIZES:
        check_mul(cname, n, AFFINE)
        check_mul(cname, n, PROJECTIVE, in_place=True)
    for n in (1, 65, 129):
        check_mul(cname, n, PROJECTIVE)
        check_mul(cname, n, AFFINE, montgomery=True)
        check_mul(cname, n, AFFINE, shared=True)
        check_mul(cname, n, PROJECTIVE, shared=True, montgomery=True, in_place=True)
    check_mul(cname, NMAX, PROJECTIVE, shared=True)


@pytest.mark.parametrize("cname", O.CURVES)
def test_fold_block_and_wave_edges(cname):
    for n in SIZES:
        check_fold(cname, n, AFFINE if n % 2 else PROJECTIVE, in_place=n % 2 == 0)
    for n in (65, 129):
        check_fold(cname, n, PROJECTIVE, montgomery=True)
        check_fold(cname, n, AFFINE, montgomery=True)


@pytest.mark.parametrize("cname", O.CURVES)
def test_add_block_and_wave_edges(cname):
    """A_i = [k_i] P_i and B_i = [a] P_(i+1) (both with z != 1); planted: O + O, O + X, X + O, X + X (doubling), X + (-X)"""
    d = data(cname)
    cid, fw = d.cid, d.fw
    one = PF.identity_rows(cname, 2, 3)
    a_all, b_all = d.exp_jac.copy(), d.ea_jac[d.hi].copy()
    neg = lambda row: np.concatenate([row[:fw], O.basefield_op(cid, "neg", row[fw:2 * fw]), row[2 * fw:]])   # noqa: E731
    for base in (0, 60):                          # at lane 0.. and across the first wave's end
        a_all[base + 0], b_all[base + 0] = one[0], one[1]
        a_all[base + 1] = one[1]
        b_all[base + 2] = one[0]
        b_all[base + 3] = a_all[base + 3]
        b_all[base + 4] = neg(a_all[base + 4])
        b_all[base + 5] = d.jac[0]
        a_all[base + 5] = PF.lift(cname, PF.curve(cname).dec(d.xy[0]), PF.lambdas(cname, 1, 99)[0])   # the same point, another z
    nb_all = np.stack([neg(r) for r in b_all])
    exp = {0: H.affine_of(cname, np.stack([O.point_op(cid, "jac_add", a_all[i], b_all[i]) for i in range(NMAX)])),
           1: H.affine_of(cname, np.stack([O.point_op(cid, "jac_add", a_all[i], nb_all[i]) for i in range(NMAX)]))}
    assert not exp[0][4].any() and not exp[1][3].any() and not exp[0][0].any()
    for n in SIZES:
        for negate in (0, 1):
            va = A.DevicePoints.from_host(cid, a_all[:n], affine=False)
            vb = A.DevicePoints.from_host(cid, b_all[:n], affine=False)
            out = A.DevicePoints(cid, n, affine=False)
            check(lib().ark_hip_sw_add_device(cid, va.ptr, vb.ptr, negate, n, out.ptr), "ark_hip_sw_add_device")   # out of place
            assert np.array_equal(got_affine(cname, out), exp[negate][:n]), (cname, n, negate)
            if n:
                check(lib().ark_hip_sw_add_device(cid, va.ptr, vb.ptr, negate, n, vb.ptr), "ark_hip_sw_add_device")  # out aliases b
                assert np.array_equal(got_affine(cname, vb), exp[negate][:n]), (cname, n, negate, "alias b")
            if negate:
                va -= A.DevicePoints.from_host(cid, b_all[:n], affine=False)                                           # out aliases a
            else:
                va += A.DevicePoints.from_host(cid, b_all[:n], affine=False)
            assert np.array_equal(got_affine(cname, va), exp[negate][:n]), (cname, n, negate, "in place")


@pytest.mark.parametrize("cname", O.CURVES)
def test_mul_points_outside_the_subgroup_and_of_small_order(cname):
    """on-curve points outside the prime-order subgroup and of order 2, 3, 11, 13 (tests/check_fixtures.py): the accumulator
    meets +-[d]P in the middle of the chain; expected values from the unreduced Python-integer ladder"""
    cv = PF.curve(cname)
    cid = O.CID[cname]
    planted = [q for q in CF.planted(cname) if q.cls in ("off_subgroup", "small_order")]
    planted = planted[:3] if cname == "BN254_G1" else planted
    rng = np.random.default_rng(0x90D + cid)
    ks = [1, 2, 3, 8, 16, 17, cv.r, (1 << 256) - 1, int("7" * 64, 16)] + [int.from_bytes(rng.bytes(32), "little") for _ in range(3)]
    rows = np.stack([q.row for q in planted for _ in ks])
    canon = np.stack([H.limbs4(k) for _ in planted for k in ks])
    exp = np.stack([cv.enc(CF.ladder(cv, cv.dec(q.row), k)) for q in planted for k in ks])
    v = A.DevicePoints.from_host(cid, rows, affine=True)
    assert np.array_equal(got_affine(cname, v.mul(canon, montgomery=False)), exp), cname
    # the same points as Lo of a fold whose Hi is a subgroup point: [k] Q + [1] P
    d = data(cname)
    k = ks[-1]
    lo = A.DevicePoints.from_host(cid, np.stack([q.row for q in planted]), affine=True)
    hi = A.DevicePoints.from_host(cid, d.xy[:len(planted)], affine=True)
    exp = np.stack([cv.enc(cv.add(CF.ladder(cv, cv.dec(q.row), k), cv.dec(d.xy[i]))) for i, q in enumerate(planted)])
    assert np.array_equal(got_affine(cname, lo.fold(hi, H.limbs4(k), H.limbs4(1), montgomery=False)), exp), cname


def _child(mode, env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "point_vec_child.py"), mode], cwd=ROOT,
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stdout.rstrip().endswith("point-vec-child ok " + mode), (out.stdout[-1500:], out.stderr[-3000:])


def test_slabs_of_64_lanes_at_n_200():
    """ARK_HIP_POINTVEC_SLAB_LOG=6: three slabs and a ragged tail for mul (the fold's slab is half: six and a tail)"""
    _child("slabs", {"ARK_HIP_POINTVEC_SLAB_LOG": "6"})


def test_saturated_form_behind_the_lazy_switch():
    """ARK_HIP_MSM_LAZY=0 is read once per process: the G1 curves on saturated limbs at n = 65 and n = 1000"""
    _child("saturated", {"ARK_HIP_MSM_LAZY": "0"})


@pytest.mark.parametrize("cname", ["BLS12_381_G1", "BLS12_377_G2"])
def test_sum_of_the_products_is_the_msm(cname):
    d = data(cname)
    sc = d.canon.copy()
    for i in range(NMAX):
        sc[i] = H.limbs4(d.ks[i] % d.r)          # the MSM entries take scalars below r
    exp = O.to_affine(d.cid, O.msm(d.cid, d.xy, sc, O.WNAF, 4))
    v = A.DevicePoints.from_host(d.cid, d.xy, affine=True)
    prod = v.mul(sc, montgomery=False)
    assert np.array_equal(A.into_affine(d.cid, A.sum_projective(d.cid, prod.to_host())), exp)
    assert np.array_equal(A.into_affine(d.cid, v.msm(sc, montgomery=False)), exp)


def test_device_points_round_trip_into_the_msm():
    """from_host -> mul (a DeviceVec of Montgomery scalars that never leaves the device) -> fold -> normalize -> device MSM"""
    cname = "BLS12_381_G1"
    d = data(cname)
    cid, r, n = d.cid, d.r, 65
    fid = O.curve_info(cid)[1]
    kv = A.DeviceVec.from_host(fid, d.mont[:n])
    kv *= kv                                                                  # k_i^2, computed on the device
    lo = A.DevicePoints.from_host(cid, d.xy[:n], affine=True).mul(kv)
    assert len(lo) == n and not lo.affine
    hi = A.DevicePoints.from_host(cid, d.jac[d.hi[:n]], affine=False)
    c = lo.clone()
    folded = lo.fold(hi, H.mont4(cname, d.a), H.mont4(cname, d.b), in_place=True)
    assert folded is lo
    aff = folded.normalize()
    assert aff.affine and len(aff) == n
    s = O.gen_scalars(fid, 0xABC, n)
    got = A.into_affine(cid, aff.msm(s, montgomery=False))
    one = PF.identity_rows(cname, 1, 0)[0]
    g = []
    for i in range(n):
        k2 = d.ks[i] * d.ks[i] % r
        x = O.scalar_mul(cid, d.xy[i], H.limbs4(k2 * d.a % r)) if k2 * d.a % r else one
        g.append(O.point_op(cid, "jac_add", x, d.eb_jac[d.hi[i]]))
    g = H.affine_of(cname, np.stack(g))
    assert np.array_equal(got_affine(cname, folded), g)
    assert np.array_equal(aff.to_host(), g)
    assert np.array_equal(got, O.to_affine(cid, O.msm(cid, g, s, O.WNAF, 4)))
    exp_c = np.stack([H.oracle_mul(cname, d.xy[i], d.ks[i] * d.ks[i]) for i in range(n)])
    assert np.array_equal(got_affine(cname, c), exp_c)                          # the clone kept the products
    for v in (lo, hi, c, aff, kv):
        v.free()
    assert len(lo) == 0


def test_host_slice_entry_in_two_chunks(monkeypatch):
    """ark_hip_sw_mul at n = 1000 with the chunk length forced to 600 points: two chunks are staged"""
    monkeypatch.setenv("ARK_HIP_POINTVEC_CHUNK_POINTS", "600")
    for cname, form, shared in (("BLS12_381_G1", AFFINE, False), ("BN254_G1", PROJECTIVE, True), ("BLS12_381_G2", AFFINE, False)):
        d = data(cname)
        pts = np.ascontiguousarray(d.xy if form == AFFINE else d.jac)
        sc = np.ascontiguousarray(H.limbs4(d.a).reshape(1, 4) if shared else d.canon)
        out = np.zeros((NMAX, 3 * d.fw), dtype=np.uint64)
        check(lib().ark_hip_sw_mul(d.cid, pts.ctypes.data_as(C.c_void_p), form, sc.ctypes.data_as(C.c_void_p), sc.shape[0], 0, NMAX,
                                   out.ctypes.data_as(C.c_void_p)), "ark_hip_sw_mul")
        assert np.array_equal(H.affine_of(cname, out), d.ea if shared else d.exp), cname
