"""The base-set check on the GPU (ark_hip_sw_check_device / ark_hip_sw_check, csrc/pointcheck.cuh), all five curves: status
bytes and the four summary words against the Python-integer model of tests/check_fixtures.py, exactly.  Planted points (not
field elements, off the curve, on the curve outside the subgroup, of small order) sit at the lane, wave and workgroup seams
of arrays of valid points; one case per curve has 2^16 points on a device-grown set, where many workgroups race for the
smallest bad index.  BLS12-377 G2 has no small-order case (its cofactor has no prime factor below 200 000); it shares the
kernel template with BLS12-381 G2."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd._lib import check, lib
import check_fixtures as CF
import oracle_lib as O
import point_fixtures as PF
import pyref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 63, 64, 65, 1000, 4097]


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _device_check(cname, t, n, checks, method=1, with_status=True):
    """ark_hip_sw_check_device on a tensor of n points -> (status bytes or None, the four summary words)"""
    import torch
    st = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda") if with_status else None
    torch.cuda.synchronize()
    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    check(lib().ark_hip_sw_check_device(O.CID[cname], t.data_ptr() if n else None, n, checks, method,
                                        st.data_ptr() if with_status else None, out), "ark_hip_sw_check_device")
    return (st.cpu().numpy()[:n] if with_status else None), [int(v) for v in out]


def _host_check(cname, rows, checks, method=1, with_status=True):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    n = rows.shape[0]
    st = np.full(max(n, 1), 0xEE, dtype=np.uint8)
    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    check(lib().ark_hip_sw_check(O.CID[cname], rows.ctypes.data_as(C.c_void_p) if n else None, n, checks, method,
                                 st.ctypes.data_as(C.c_void_p) if with_status else None, out), "ark_hip_sw_check")
    return (st[:n] if with_status else None), [int(v) for v in out]


def _cases(cname, n):
    """{name: (rows, planted indices)}: all valid; one bad point, the last; every planted point at the seams; all bad"""
    bad = CF.bad_rows(cname)
    allp = CF.planted_rows(cname)
    cases = {"all_valid": CF.plant(cname, n, ()), "seams": CF.plant(cname, n, allp)}
    if n:
        cases["one_bad_last"] = CF.plant(cname, n, bad[n % len(bad):][:1], where=(n - 1,))
        cases["all_bad"] = CF.plant(cname, n, bad, where=range(n))
        cases["seams_bad_from_64"] = CF.plant(cname, n, bad, where=[i for i in CF.PLANT_AT + (n - 1,) if i >= 64])
    return cases


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_status_and_summary_are_exact(cname, n):
    for name, (rows, where) in _cases(cname, n).items():
        want_st, want = CF.expected(cname, rows, where, 3)
        if name == "all_valid":
            assert want == [n, 0, 0, 0]
        if name == "all_bad":
            assert want[0] == 0 and sum(want[1:]) == n
        if name == "one_bad_last":
            assert want[0] == n - 1 and sum(want[1:]) == 1
        if name == "seams_bad_from_64" and n > 64:
            assert want[0] == 64                  # several classes present: the smallest bad index, not the first class
        t = _dev(rows) if n else None
        st, out = _device_check(cname, t, n, 3)
        assert st.tolist() == want_st.tolist(), (cname, n, name, np.nonzero(st != want_st)[0][:8])
        assert out == want, (cname, n, name)
        _, out2 = _device_check(cname, t, n, 3, with_status=False)      # d_status = NULL: the same summary
        assert out2 == want, (cname, n, name, "no status")
        if n:
            assert np.array_equal(t.cpu().numpy().view(np.uint64).reshape(rows.shape), rows), "the input is not modified"


@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_every_mask_and_method_agrees_with_the_model(cname):
    n = 1000
    rows, where = CF.plant(cname, n, CF.planted_rows(cname), where=CF.PLANT_AT + tuple(range(300, 330)) + (n - 1,))
    assert len(where) >= len(CF.planted(cname))          # every planted point is in
    t = _dev(rows)
    got = {}
    for checks in (1, 2, 3):
        for method in (0, 1, 2):
            if method == 2 and cname != "BLS12_381_G1":
                continue
            want_st, want = CF.expected(cname, rows, where, checks, 2 if method == 2 else 1)
            st, out = _device_check(cname, t, n, checks, method)
            assert st.tolist() == want_st.tolist(), (cname, checks, method, np.nonzero(st != want_st)[0][:8])
            assert out == want, (cname, checks, method)
            got[checks, method] = st
    if cname == "BLS12_381_G1":                          # the two methods: byte-identical status
        for checks in (1, 3):
            assert got[checks, 1].tobytes() == got[checks, 2].tobytes() == got[checks, 0].tobytes()
    else:
        out = (C.c_uint64 * 4)()
        assert lib().ark_hip_sw_check_device(O.CID[cname], t.data_ptr(), n, 3, 2, None, out) == -1   # method 2 elsewhere


@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_host_slice_entry_equals_the_device_entry(cname, monkeypatch):
    n = 1000
    rows, where = CF.plant(cname, n, CF.planted_rows(cname), where=CF.PLANT_AT + tuple(range(640, 670)) + (n - 1,))
    want_st, want = CF.expected(cname, rows, where, 3)
    st_d, out_d = _device_check(cname, _dev(rows), n, 3)
    assert st_d.tolist() == want_st.tolist() and out_d == want
    for chunk in (None, "333", "64", "7"):               # one upload; four chunks with a ragged last one; whole workgroups; a few lanes
        if chunk is None:
            monkeypatch.delenv("ARK_HIP_CHECK_CHUNK_POINTS", raising=False)
        else:
            monkeypatch.setenv("ARK_HIP_CHECK_CHUNK_POINTS", chunk)
        m = n if chunk != "7" else 130
        st_h, out_h = _host_check(cname, rows[:m], 3)
        w_st, w = CF.expected(cname, rows[:m], [i for i in where if i < m], 3)
        assert st_h.tolist() == w_st.tolist() and out_h == w, (cname, chunk)
        assert _host_check(cname, rows[:m], 3, with_status=False)[1] == w, (cname, chunk)
    monkeypatch.delenv("ARK_HIP_CHECK_CHUNK_POINTS", raising=False)
    assert _host_check(cname, rows[:0], 3)[1] == [0, 0, 0, 0]


def _grown(cname, n, m=256):
    """n points [7 + 11 i] G on the device, grown from the first m by P[i + k] = P[i] + [11 k] G (valid by construction)"""
    import torch
    cv = PF.curve(cname)
    cid = O.CID[cname]
    words = 2 * cv.fw
    t = torch.zeros(n * words, dtype=torch.int64, device="cuda")
    t[:m * words] = _dev(CF.plant(cname, m, ())[0]).reshape(-1)
    torch.cuda.synchronize()
    k = m
    while k < n:
        delta = np.ascontiguousarray(cv.enc(cv.mul(PF.generator(cname), 11 * k)))
        check(lib().ark_hip_sw_add_affine_device(cid, t.data_ptr(), t.data_ptr() + k * words * 8, k, delta.ctypes.data_as(C.c_void_p)),
              "ark_hip_sw_add_affine_device")
        k *= 2
    return t


@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_many_workgroups_race_for_the_first_bad_index(cname):
    """2^16 points (512 workgroups): a valid set grown on the device, then about 40 planted points copied in"""
    import torch
    n = 1 << 16
    cv = PF.curve(cname)
    words = 2 * cv.fw
    t = _grown(cname, n)
    st, out = _device_check(cname, t, n, 3)
    assert out == [n, 0, 0, 0] and not st.any()
    last = t.view(n, words)[n - 1].cpu().numpy().view(np.uint64)
    assert np.array_equal(last, cv.enc(cv.mul(PF.generator(cname), 7 + 11 * (n - 1))))     # the set is what it claims to be
    rng = np.random.default_rng(0x16 + O.CID[cname])
    planted = CF.planted_rows(cname)
    where = sorted(set([40961, 40960, 40959, n - 1, n - 128, 65000] + [int(i) for i in rng.integers(41000, n, size=34)]))
    assert 38 <= len(where) <= 40
    order = rng.permutation(len(where))                  # which planted point goes where: not in index order
    bad_rows = CF.bad_rows(cname)                        # ten slots cycle through every planted point, the rest through the bad ones
    rows = np.stack([planted[(7 + int(k)) % len(planted)] if k < 10 else bad_rows[int(k) % len(bad_rows)] for k in order])
    t.view(n, words)[torch.tensor(where, device="cuda")] = _dev(rows)
    torch.cuda.synchronize()
    want = np.zeros(n, dtype=np.uint8)
    for i, row in zip(where, rows):
        want[i] = CF.model_status(cname, row, 3)
    bad = np.nonzero(want)[0]
    assert bad.size >= 20 and len(set(i // 128 for i in bad)) >= 15        # many workgroups have something to report
    summary = [int(bad[0])] + [int((want == k).sum()) for k in (1, 2, 3)]
    st, out = _device_check(cname, t, n, 3)
    assert np.array_equal(st, want), np.nonzero(st != want)[0][:8]
    assert out == summary
    assert _device_check(cname, t, n, 3, with_status=False)[1] == summary
    if cname == "BLS12_381_G1":
        st2, out2 = _device_check(cname, t, n, 3, method=2)
        assert st2.tobytes() == st.tobytes() and out2 == summary


@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_a_checked_tensor_gives_the_same_msm(cname):
    n = 1000
    cid = O.CID[cname]
    rows, _ = CF.plant(cname, n, ())
    t = _dev(rows)
    scalars = O.gen_scalars(O.curve_info(cid)[1], 5, n)
    s = _dev(scalars)
    before = A.into_affine(cid, A.msm_bigint(cid, t, s))
    res = A.check_bases(cname, t, return_status=True)
    assert res.ok and res.first_bad == n and not res.status.cpu().numpy().any()
    assert np.array_equal(t.cpu().numpy().view(np.uint64).reshape(rows.shape), rows)
    assert np.array_equal(A.into_affine(cid, A.msm_bigint(cid, t, s)), before)


@pytest.mark.parametrize("cname", ["BLS12_381_G1", "BLS12_377_G2"])
def test_python_mirror(cname):
    n = 300
    rows, where = CF.plant(cname, n, CF.planted_rows(cname), where=CF.PLANT_AT + tuple(range(100, 130)) + (n - 1,))
    for subgroup, checks in ((True, 3), (False, 1)):
        want_st, want = CF.expected(cname, rows, where, checks)
        for pts in (rows, _dev(rows)):
            r = A.check_bases(cname, pts, subgroup=subgroup, return_status=True)
            st = r.status if isinstance(r.status, np.ndarray) else r.status.cpu().numpy()
            assert st.tolist() == want_st.tolist()
            assert [r.first_bad, r.not_reduced, r.off_curve, r.off_subgroup] == want and r.ok is False
            r = A.check_bases(cname, pts, subgroup=subgroup)
            assert r.status is None and [r.first_bad, r.not_reduced, r.off_curve, r.off_subgroup] == want
    want_st, want = CF.expected(cname, rows, where, 2)              # "assuming on curve"
    r = A.check_bases(cname, rows, on_curve=False, return_status=True)
    assert r.status.tolist() == want_st.tolist() and r.first_bad == want[0]
    good = A.check_bases(cname, CF.plant(cname, 64, ())[0])
    assert good.ok and good == A.BaseCheck(True, 64, 0, 0, 0, None)
    assert A.check_bases(cname, np.zeros((0, rows.shape[1]), dtype=np.uint64)).first_bad == 0


def test_cpp_mirror(tmp_path):
    """check_bases / check_bases_device of include/ark_hip.hpp from a compiled C++ program: the points and the expected status
    bytes travel in a file"""
    cname = "BLS12_381_G1"
    n = 300
    rows, where = CF.plant(cname, n, CF.planted_rows(cname), where=CF.PLANT_AT + tuple(range(100, 130)) + (n - 1,))
    want_st, want = CF.expected(cname, rows, where, 3)
    path = str(tmp_path / "points.bin")
    with open(path, "wb") as f:
        f.write(np.array([n] + want, dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(rows).tobytes())
        f.write(want_st.tobytes())
    exe = str(tmp_path / "check_bases_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "check_bases_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd")],
                          timeout=300)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
