"""The compressed-point codec on the GPU (ark_hip_sw_decompress_device / ark_hip_sw_decompress / ark_hip_sw_compress*,
csrc/pointcodec.cuh), all five curves: points, status bytes and the five summary words against the Python-integer model of
tests/compress_fixtures.py, exactly.  Planted encodings (refused flags, components that are no field elements, x without a root,
points outside the subgroup) sit at the lane, wave and workgroup seams of arrays of valid encodings; one case per curve has 2^16
points on a device-grown set, where many workgroups race for the smallest bad index."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd import _lib
from algebra_amd._lib import check, lib
import check_fixtures as CF
import compress_fixtures as X
import oracle_lib as O
import point_fixtures as PF
import pyref as P
from test_gpu_check_bases import _grown
from test_point_codec_host import sqrt_vectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = [0, 1, 63, 64, 65, 1000, 4097]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev_bytes(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _device_decompress(cname, t, n, validate, method=0, with_status=True):
    """ark_hip_sw_decompress_device on a uint8 tensor of n encodings -> (points, status bytes or None, the five summary words)"""
    import torch
    words = 2 * PF.curve(cname).fw
    pts = torch.full((max(n, 1), words), -1, dtype=torch.int64, device="cuda")
    st = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda") if with_status else None
    torch.cuda.synchronize()
    out = (C.c_uint64 * 5)(9, 9, 9, 9, 9)
    check(lib().ark_hip_sw_decompress_device(O.CID[cname], t.data_ptr() if n else None, n, validate, method, pts.data_ptr() if n else None,
                                             st.data_ptr() if with_status else None, out), "ark_hip_sw_decompress_device")
    return pts.cpu().numpy().view(np.uint64)[:n], (st.cpu().numpy()[:n] if with_status else None), [int(v) for v in out]


def _host_decompress(cname, rows, validate, method=0, with_status=True):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n = rows.shape[0]
    pts = np.full((max(n, 1), 2 * PF.curve(cname).fw), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    st = np.full(max(n, 1), 0xEE, dtype=np.uint8)
    out = (C.c_uint64 * 5)(9, 9, 9, 9, 9)
    check(lib().ark_hip_sw_decompress(O.CID[cname], _vp(rows) if n else None, n, validate, method, _vp(pts) if n else None,
                                      _vp(st) if with_status else None, out), "ark_hip_sw_decompress")
    return pts[:n], (st[:n] if with_status else None), [int(v) for v in out]


def _cases(cname, n, validate):
    bad = X.bad_rows(cname, validate)
    allp = X.planted_rows(cname)
    cases = {"all_valid": X.plant(cname, n, ()), "seams": X.plant(cname, n, allp)}
    if n:
        cases["one_bad_last"] = X.plant(cname, n, bad[n % len(bad):][:1], where=(n - 1,))
        cases["seams_bad_from_64"] = X.plant(cname, n, bad, where=[i for i in CF.PLANT_AT + (n - 1,) if i >= 64])
        cases["all_bad"] = X.plant(cname, n, bad, where=range(n))
    return cases


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_points_status_and_summary_are_exact(cname, n):
    for validate in (1, 0):
        for name, (rows, where) in _cases(cname, n, bool(validate)).items():
            want_pts, want_st, want = X.expected(cname, rows, where, bool(validate))
            if name == "all_valid":
                assert want == [n, 0, 0, 0, 0]
            if name == "all_bad":
                assert want[0] == 0 and sum(want[1:]) == n
            if name == "one_bad_last":
                assert want[0] == n - 1 and sum(want[1:]) == 1
            if name == "seams_bad_from_64" and n > 64:
                assert want[0] == 64
            if not validate:
                assert want[4] == 0
            t = _dev_bytes(rows) if n else None
            pts, st, out = _device_decompress(cname, t, n, validate)
            assert st.tolist() == want_st.tolist(), (cname, n, name, validate, np.nonzero(st != want_st)[0][:8])
            assert np.array_equal(pts, want_pts), (cname, n, name, validate, np.nonzero((pts != want_pts).any(axis=1))[0][:8])
            assert out == want, (cname, n, name, validate)
            pts2, _, out2 = _device_decompress(cname, t, n, validate, with_status=False)      # d_status = NULL
            assert out2 == want and np.array_equal(pts2, want_pts), (cname, n, name, "no status")
            if n:
                assert np.array_equal(t.cpu().numpy(), rows), "the input is not modified"


@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_every_method_agrees_with_the_model(cname):
    n = 300
    rows, where = X.plant(cname, n, X.planted_rows(cname), where=CF.PLANT_AT + tuple(range(100, 140)) + (n - 1,))
    assert len(where) >= len(X.planted(cname))
    t = _dev_bytes(rows)
    for validate in (0, 1):
        want_pts, want_st, want = X.expected(cname, rows, where, bool(validate))
        for method in (0, 1, 2):
            out5 = (C.c_uint64 * 5)()
            if method == 2 and cname != "BLS12_381_G1":
                assert lib().ark_hip_sw_decompress_device(O.CID[cname], t.data_ptr(), n, validate, 2, t.data_ptr(), None, out5) == -1
                continue
            pts, st, out = _device_decompress(cname, t, n, validate, method)
            assert st.tolist() == want_st.tolist() and out == want and np.array_equal(pts, want_pts), (cname, validate, method)


@pytest.mark.parametrize("g, cname", [("g1", "BLS12_381_G1"), ("g2", "BLS12_381_G2")])
def test_the_reference_vectors(g, cname):
    """the reference's compressed k G tables through the device entry and the host-slice entry, and back"""
    cv = PF.curve(cname)
    rows = np.load(os.path.join(GOLDEN, "bls12_381_%s_compressed.npz" % g))["bytes"]
    gold = np.load(os.path.join(GOLDEN, "bls12_381_%s_multiples.npz" % g))
    want = np.zeros((1000, 2 * cv.fw), dtype=np.uint64)
    for k in range(1, 1000):
        want[k] = np.concatenate([P.to_mont(P.from_limbs(c), cv.p) for c in gold["xy"][k].reshape(-1, 6)])
    t = _dev_bytes(rows)
    for validate in (0, 1):
        pts, st, out = _device_decompress(cname, t, 1000, validate)
        assert out == [1000, 0, 0, 0, 0] and not st.any() and np.array_equal(pts, want)
        pts, st, out = _host_decompress(cname, rows, validate)
        assert out == [1000, 0, 0, 0, 0] and not st.any() and np.array_equal(pts, want)
    assert np.array_equal(A.compress_bases(cname, want), rows)
    import torch
    back = A.compress_bases(cname, torch.from_numpy(want.view(np.int64)).cuda())
    assert np.array_equal(back.cpu().numpy(), rows)


@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_host_slice_entry_equals_the_device_entry(cname, monkeypatch):
    n = 1000
    rows, where = X.plant(cname, n, X.planted_rows(cname), where=CF.PLANT_AT + tuple(range(640, 680)) + (n - 1,))
    want_pts, want_st, want = X.expected(cname, rows, where, True)
    pts_d, st_d, out_d = _device_decompress(cname, _dev_bytes(rows), n, 1)
    assert st_d.tolist() == want_st.tolist() and out_d == want and np.array_equal(pts_d, want_pts)
    nv_pts, nv_st, nv = X.expected(cname, rows, where, False)
    assert _device_decompress(cname, _dev_bytes(rows), n, 0)[2] == nv
    canon = A.compress_bases(cname, want_pts)
    for chunk in (None, "1000", "64", "1"):      # one upload; one full chunk; whole workgroups and a ragged last one; one launch per point
        if chunk is None:
            monkeypatch.delenv("ARK_HIP_DECOMPRESS_CHUNK_POINTS", raising=False)
        else:
            monkeypatch.setenv("ARK_HIP_DECOMPRESS_CHUNK_POINTS", chunk)
        if chunk == "1":
            # a thousand single-lane launches: the full array without the subgroup ladder (one lane runs it in tens of milliseconds
            # over Fp2), then a 40-row array whose rows 8 .. 39 are every bad encoding, status 4 included, with the ladder
            pts_h, st_h, out_h = _host_decompress(cname, rows, 0)
            assert st_h.tolist() == nv_st.tolist() and out_h == nv and np.array_equal(pts_h, nv_pts), (cname, chunk)
            bad = X.bad_rows(cname)
            short, sw = X.plant(cname, 40, bad, where=range(8, 40))
            assert len(sw) >= len(bad)
            s_pts, s_st, s_out = X.expected(cname, short, sw, True)
            assert s_out[0] == 8 and (s_out[4] > 0 or cname in CF.COFACTOR_ONE)
            pts_h, st_h, out_h = _host_decompress(cname, short, 1)
            assert st_h.tolist() == s_st.tolist() and out_h == s_out and np.array_equal(pts_h, s_pts), (cname, chunk, "validate")
            assert _host_decompress(cname, short, 1, with_status=False)[2] == s_out, (cname, chunk, "validate, no status")
            assert np.array_equal(A.compress_bases(cname, want_pts), canon), (cname, chunk)
            continue
        pts_h, st_h, out_h = _host_decompress(cname, rows, 1)
        assert st_h.tolist() == want_st.tolist() and out_h == want and np.array_equal(pts_h, want_pts), (cname, chunk)
        pts_h, _, out_h = _host_decompress(cname, rows, 1, with_status=False)
        assert out_h == want and np.array_equal(pts_h, want_pts), (cname, chunk)
        assert np.array_equal(A.compress_bases(cname, want_pts), canon), (cname, chunk)
    monkeypatch.delenv("ARK_HIP_DECOMPRESS_CHUNK_POINTS", raising=False)
    assert _host_decompress(cname, rows[:0], 1)[2] == [0, 0, 0, 0, 0]


@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_round_trip_and_the_race_for_the_first_bad_index(cname):
    """2^16 points (512 workgroups) grown on the device: decompress(compress(P)) == P; compress against the model on 64 sampled
    rows; then about 40 bad encodings planted"""
    import torch
    n = 1 << 16
    cv = PF.curve(cname)
    words = 2 * cv.fw
    t = _grown(cname, n)
    enc = A.compress_bases(cname, t)
    assert enc.shape == (n, X.size(cname))
    pts, res = A.decompress_bases(cname, enc, return_status=True)
    assert res.ok and res.first_bad == n and not res.status.any().item()
    assert torch.equal(pts.reshape(-1), t.reshape(-1))
    rng = np.random.default_rng(0x17 + O.CID[cname])
    sample = sorted(set([0, 1, 127, 128, n - 1] + [int(i) for i in rng.integers(0, n, size=59)]))
    rows_h = t.view(n, words)[torch.tensor(sample, device="cuda")].cpu().numpy().view(np.uint64)
    enc_h = enc[torch.tensor(sample, device="cuda")].cpu().numpy()
    for r, e in zip(rows_h, enc_h):
        assert e.tobytes() == X.encode(cname, cv.dec(r))
    where = sorted(set([40961, 40960, 40959, n - 1, n - 128, 65000] + [int(i) for i in rng.integers(41000, n, size=34)]))
    assert 38 <= len(where) <= 40
    bad = X.bad_rows(cname)
    order = rng.permutation(len(where))
    planted = np.stack([bad[int(k) % len(bad)] for k in order])
    enc[torch.tensor(where, device="cuda")] = _dev_bytes(planted)
    torch.cuda.synchronize()
    want = np.zeros(n, dtype=np.uint8)
    for i, row in zip(where, planted):
        want[i] = X.status(cname, row.tobytes())
    assert (want[where] != 0).all() and len(set(i // 128 for i in where)) >= 15
    pts2, res = A.decompress_bases(cname, enc, return_status=True)
    assert np.array_equal(res.status.cpu().numpy(), want)
    assert [res.first_bad, res.bad_flags, res.not_reduced, res.no_root, res.off_subgroup] == X.summary(want) and not res.ok
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[torch.tensor(where, device="cuda")] = False
    assert torch.equal(pts2[keep], t.view(n, words)[keep]) and not pts2[~keep].any().item()
    _, res = A.decompress_bases(cname, enc)
    assert res.status is None and res.first_bad == where[0]


@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_the_square_root_hook_on_the_device(cname):
    names, a, want, ok = sqrt_vectors(cname)
    reps = 3                                     # more than one wave, the same inputs in different lanes
    a3, want3, ok3 = np.tile(a, (reps, 1)), np.tile(want, (reps, 1)), np.tile(ok, reps)
    out = np.full_like(a3, 0xEEEEEEEEEEEEEEEE)
    got = np.full(len(a3), 0xEE, dtype=np.uint8)
    check(_lib.test_lib().ark_hip_test_coord_sqrt(O.CID[cname], _vp(a3), _vp(out), _vp(got), len(a3)), "ark_hip_test_coord_sqrt")
    assert got.tolist() == ok3.tolist(), [names[i % len(names)] for i in np.nonzero(got != ok3)[0][:8]]
    assert np.array_equal(out, want3)


@pytest.mark.parametrize("cname", P.CURVE_ORDER)
def test_a_decompressed_tensor_gives_the_same_msm(cname):
    import torch
    n = 1000
    cid = O.CID[cname]
    enc, pts = X._chain(cname, n)
    t = torch.from_numpy(pts.view(np.int64).copy()).cuda()
    s = torch.from_numpy(O.gen_scalars(O.curve_info(cid)[1], 5, n).view(np.int64)).cuda()
    before = A.into_affine(cid, A.msm_bigint(cid, t, s))
    dec, res = A.decompress_bases(cname, _dev_bytes(enc))
    assert res.ok and torch.equal(dec.reshape(-1), t.reshape(-1))
    assert np.array_equal(A.into_affine(cid, A.msm_bigint(cid, dec, s)), before)


@pytest.mark.parametrize("cname", ["BLS12_381_G1", "BLS12_377_G2"])
def test_python_mirror(cname):
    n = 300
    rows, where = X.plant(cname, n, X.planted_rows(cname), where=CF.PLANT_AT + tuple(range(100, 140)) + (n - 1,))
    assert A.compressed_size(cname) == X.size(cname)
    for validate in (True, False):
        want_pts, want_st, want = X.expected(cname, rows, where, validate)
        for data in (rows, rows.tobytes(), _dev_bytes(rows)):
            pts, r = A.decompress_bases(cname, data, validate=validate, return_status=True)
            host = isinstance(pts, np.ndarray)
            st = r.status if host else r.status.cpu().numpy()
            assert st.tolist() == want_st.tolist()
            assert np.array_equal(pts if host else pts.cpu().numpy().view(np.uint64), want_pts)
            assert [r.first_bad, r.bad_flags, r.not_reduced, r.no_root, r.off_subgroup] == want and r.ok is False
            pts, r = A.decompress_bases(cname, data, validate=validate)
            assert r.status is None and [r.first_bad, r.bad_flags, r.not_reduced, r.no_root, r.off_subgroup] == want
    enc, pts = X._chain(cname, 64)
    got, good = A.decompress_bases(cname, enc)
    assert good == A.BaseDecode(True, 64, 0, 0, 0, 0, None) and np.array_equal(got, pts)
    assert np.array_equal(A.compress_bases(cname, pts), enc)
    empty, r = A.decompress_bases(cname, np.zeros((0, X.size(cname)), dtype=np.uint8))
    assert empty.shape == (0, pts.shape[1]) and r.first_bad == 0 and r.ok
    assert A.compress_bases(cname, empty).shape == (0, X.size(cname))


def test_cpp_mirror(tmp_path):
    """decompress_bases / decompress_bases_device / compress_bases of include/ark_hip.hpp from a compiled C++ program"""
    cname = "BLS12_381_G1"
    cv = PF.curve(cname)
    n = 300
    rows, where = X.plant(cname, n, X.planted_rows(cname), where=CF.PLANT_AT + tuple(range(100, 140)) + (n - 1,))
    want_pts, want_st, want = X.expected(cname, rows, where, True)
    canon = b"".join(X.encode(cname, cv.dec(r)) for r in want_pts)
    path = str(tmp_path / "encodings.bin")
    with open(path, "wb") as f:
        f.write(np.array([n] + want, dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(rows).tobytes())
        f.write(np.ascontiguousarray(want_pts).tobytes())
        f.write(want_st.tobytes())
        f.write(canon)
    exe = str(tmp_path / "point_codec_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "point_codec_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd")],
                          timeout=300)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
