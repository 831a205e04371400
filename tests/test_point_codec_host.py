"""CPU-side checks of the compressed-point codec (no GPU needed): the five entries and the four hooks are C ABI with the same arity
in the header, `_lib.SYMBOLS` / `TEST_SYMBOLS`, ark-hip-sys and ark_hip.hpp; argument errors come before any device is touched;
and the HOST builds of sw_decompress_point / sw_compress_point / coord_sqrt (csrc/pointcodec.cuh: the functions the kernels run)
agree with the Python-integer model of tests/compress_fixtures.py on every planted encoding of all five curves, on the
reference's own compressed BLS12-381 vectors, and on square-root inputs that no curve point reaches.  Every comparison is exact.
The kernels are checked on the GPU by tests/test_gpu_point_codec.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from algebra_amd import _lib
import check_fixtures as CF
import compress_fixtures as X
import point_fixtures as PF
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PUBLIC = {"ark_hip_sw_compressed_size": 1, "ark_hip_sw_decompress_device": 8, "ark_hip_sw_decompress": 8,
          "ark_hip_sw_compress_device": 4, "ark_hip_sw_compress": 4}
HOOKS = {"ark_hip_test_host_sw_decompress": 7, "ark_hip_test_host_sw_compress": 4, "ark_hip_test_coord_sqrt": 5,
         "ark_hip_test_host_coord_sqrt": 5}
ERR_ARG = -1
G1_381 = pyref.CURVE_ORDER.index("BLS12_381_G1")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


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
    assert "ark_hip_*" in open(os.path.join(ROOT, "algebra_amd", "csrc", "exports.map")).read()
    for cid, cname in enumerate(pyref.CURVE_ORDER):
        assert L.ark_hip_sw_compressed_size(cid) == X.size(cname)
    assert L.ark_hip_sw_compressed_size(5) == ERR_ARG and L.ark_hip_sw_compressed_size(-1) == ERR_ARG


def test_rust_and_cpp_mirrors_have_the_entries():
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    found = dict((n, len([a for a in args.split(",") if a.strip()]))
                 for n, args in re.findall(r"pub fn (ark_hip_\w+)\s*\(([^;]*?)\)\s*(?:->\s*[^;]+)?;", ext, flags=re.S))
    for name, arity in PUBLIC.items():
        assert found.get(name) == arity, name
    msm_rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "msm.rs")).read()
    assert re.search(r"pub fn decompress_bases<P: HipServed>\(", msm_rs) and "sys::ark_hip_sw_decompress(" in msm_rs
    assert re.search(r"pub fn compress_bases<P: HipServed>\(", msm_rs) and "sys::ark_hip_sw_compress(" in msm_rs
    lib_rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "lib.rs")).read()
    assert "decompress_bases" in lib_rs and "compress_bases" in lib_rs
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for name in PUBLIC:
        assert name + "(" in hpp, name
    assert "struct BaseDecode" in hpp
    for fn in ("decompress_bases", "decompress_bases_device", "compress_bases"):
        assert re.search(r"\b%s\(" % fn, hpp), fn
    import algebra_amd
    assert callable(algebra_amd.decompress_bases) and callable(algebra_amd.compress_bases) and callable(algebra_amd.compressed_size)


def test_argument_errors_come_before_any_device_use():
    L, T = _lib.lib(), _lib.test_lib()
    d, d2 = C.c_void_p(1 << 20), C.c_void_p(1 << 24)      # non-null "device pointers" that are never dereferenced
    out = (C.c_uint64 * 5)()
    hb = (C.c_uint8 * 96)()
    hp = (C.c_uint64 * 24)()
    hbp, hpp = C.cast(hb, C.c_void_p), C.cast(hp, C.c_void_p)
    for fn, b, p in ((L.ark_hip_sw_decompress_device, d, d2), (L.ark_hip_sw_decompress, hbp, hpp)):
        out[:] = [7] * 5
        assert fn(5, b, 1, 1, 0, p, None, out) == ERR_ARG and fn(-1, b, 1, 1, 0, p, None, out) == ERR_ARG
        assert fn(1, b, 1, 2, 0, p, None, out) == ERR_ARG and fn(1, b, 1, -1, 0, p, None, out) == ERR_ARG
        assert fn(1, b, 1, 1, 3, p, None, out) == ERR_ARG and fn(1, b, 1, 1, -1, p, None, out) == ERR_ARG
        assert fn(1, None, 1, 1, 0, p, None, out) == ERR_ARG and fn(1, b, 1, 1, 0, None, None, out) == ERR_ARG
        assert fn(1, b, 1, 1, 0, p, None, None) == ERR_ARG
        for curve in range(5):                   # the endomorphism test is BLS12-381 G1's alone -- checked with validate = 0 too
            if curve != G1_381:
                assert fn(curve, b, 1, 1, 2, p, None, out) == ERR_ARG and fn(curve, b, 1, 0, 2, p, None, out) == ERR_ARG, curve
        assert list(out) == [7] * 5
        for curve in range(5):                   # n = 0: zeros, whatever the pointers
            out[:] = [7] * 5
            assert fn(curve, None, 0, 1, 0, None, None, out) == 0 and list(out) == [0] * 5
        if L.ark_hip_device_count() == 0:        # a well-formed call: loud refusal, no CPU fallback
            assert fn(1, b, 1, 1, 0, p, None, out) == -5
    dd = L.ark_hip_sw_decompress_device
    assert dd(1, C.c_void_p((1 << 20) + 2), 1, 1, 0, d2, None, out) == ERR_ARG          # misaligned bytes
    assert dd(1, d, 1, 1, 0, C.c_void_p((1 << 24) + 2), None, out) == ERR_ARG           # misaligned points
    assert dd(1, d, 4, 1, 0, C.c_void_p((1 << 20) + 48), None, out) == ERR_ARG          # overlap: 4 * 48 bytes of input
    assert dd(1, C.c_void_p((1 << 20) + 96), 4, 1, 0, d, None, out) == ERR_ARG          # overlap: 4 * 96 bytes of output
    for fn, p, b in ((L.ark_hip_sw_compress_device, d2, d), (L.ark_hip_sw_compress, hpp, hbp)):
        assert fn(5, p, 1, b) == ERR_ARG and fn(-1, p, 1, b) == ERR_ARG
        assert fn(1, None, 1, b) == ERR_ARG and fn(1, p, 1, None) == ERR_ARG
        assert fn(1, None, 0, None) == 0
        if L.ark_hip_device_count() == 0:
            assert fn(1, p, 1, b) == -5
    cd = L.ark_hip_sw_compress_device
    assert cd(1, d2, 1, C.c_void_p((1 << 20) + 1)) == ERR_ARG and cd(1, C.c_void_p((1 << 24) + 2), 1, d) == ERR_ARG
    assert cd(1, d, 4, C.c_void_p((1 << 20) + 96)) == ERR_ARG
    st = (C.c_uint8 * 4)()
    assert T.ark_hip_test_host_sw_decompress(5, hbp, 1, 1, 1, hpp, st) == ERR_ARG
    assert T.ark_hip_test_host_sw_decompress(1, hbp, 1, 2, 1, hpp, st) == ERR_ARG
    assert T.ark_hip_test_host_sw_decompress(1, hbp, 1, 1, 3, hpp, st) == ERR_ARG
    assert T.ark_hip_test_host_sw_decompress(2, hbp, 1, 1, 2, hpp, st) == ERR_ARG
    assert T.ark_hip_test_host_sw_decompress(1, None, 1, 1, 1, hpp, st) == ERR_ARG
    assert T.ark_hip_test_host_sw_compress(5, hpp, 1, hbp) == ERR_ARG and T.ark_hip_test_host_sw_compress(1, None, 1, hbp) == ERR_ARG
    assert T.ark_hip_test_host_coord_sqrt(5, hpp, hpp, st, 1) == ERR_ARG and T.ark_hip_test_host_coord_sqrt(1, hpp, hpp, None, 1) == ERR_ARG
    assert T.ark_hip_test_coord_sqrt(5, hpp, hpp, st, 1) == ERR_ARG and T.ark_hip_test_coord_sqrt(1, None, hpp, st, 1) == ERR_ARG


def host_decompress(cname, rows, validate, method=0, with_status=True):
    cv = PF.curve(cname)
    rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, X.size(cname))
    n = rows.shape[0]
    pts = np.full((n, 2 * cv.fw), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    st = np.full(n, 0xEE, dtype=np.uint8)
    rc = _lib.test_lib().ark_hip_test_host_sw_decompress(pyref.CURVE_ORDER.index(cname), _vp(rows), n, validate, method, _vp(pts),
                                                         _vp(st) if with_status else None)
    assert rc == 0, (cname, validate, method, rc)
    return pts, st


def host_compress(cname, pts):
    pts = np.ascontiguousarray(pts, dtype=np.uint64)
    out = np.full((pts.shape[0], X.size(cname)), 0xEE, dtype=np.uint8)
    assert _lib.test_lib().ark_hip_test_host_sw_compress(pyref.CURVE_ORDER.index(cname), _vp(pts), pts.shape[0], _vp(out)) == 0
    return out


@pytest.mark.parametrize("cname", pyref.CURVE_ORDER)
def test_host_twin_agrees_with_the_model_on_every_planted_encoding(cname):
    planted = X.planted(cname)                   # asserts the number of encodings per class and each class's status
    rows = X.planted_rows(cname)
    names = [q.name for q in planted]
    for validate in (0, 1):
        want_pts, want_st, _ = X.model(cname, rows, bool(validate))
        for method in (0, 1, 2):
            if method == 2 and cname != "BLS12_381_G1":
                continue
            pts, st = host_decompress(cname, rows, validate, method)
            assert st.tolist() == want_st.tolist(), (cname, validate, method, [n for n, a, b in zip(names, st, want_st) if a != b])
            assert np.array_equal(pts, want_pts), (cname, validate, method, [n for n, a, b in zip(names, pts, want_pts) if not np.array_equal(a, b)])
        assert np.array_equal(host_decompress(cname, rows, validate, 0, with_status=False)[0], want_pts)
    _, st, summary = X.model(cname, rows, True)
    assert summary[0] == 7 and sum(summary[1:]) == int((st != 0).sum())      # six chain points and the identity come first
    assert not want_pts[st != 0].any()           # a refused encoding is written as the identity


@pytest.mark.parametrize("g, cname", [("g1", "BLS12_381_G1"), ("g2", "BLS12_381_G2")])
def test_host_twin_on_the_reference_vectors(g, cname):
    """the reference's compressed k G tables against its uncompressed ones (tests/golden/*_multiples.npz)"""
    cv = PF.curve(cname)
    rows = np.load(os.path.join(GOLDEN, "bls12_381_%s_compressed.npz" % g))["bytes"]
    gold = np.load(os.path.join(GOLDEN, "bls12_381_%s_multiples.npz" % g))
    assert rows.shape == (1000, X.size(cname)) and rows.dtype == np.uint8
    assert int(((rows[:, 0] >> 5) & 1).sum()) == {"g1": 494, "g2": 522}[g] and gold["infinity"].tolist() == [1] + [0] * 999
    want = np.zeros((1000, 2 * cv.fw), dtype=np.uint64)
    for k in range(1, 1000):
        want[k] = np.concatenate([pyref.to_mont(pyref.from_limbs(c), cv.p) for c in gold["xy"][k].reshape(-1, 6)])
    for validate, method in ((0, 0), (1, 1)) + (((1, 2),) if g == "g1" else ()):
        pts, st = host_decompress(cname, rows, validate, method)
        assert not st.any() and np.array_equal(pts, want), (validate, method)
    assert np.array_equal(host_compress(cname, want), rows)
    for k in (0, 1, 2, 500, 999):                # ... and the model reads them the same way
        s, pt = X.decode(cname, rows[k].tobytes())
        assert s == 0 and np.array_equal(cv.enc(pt), want[k])


@pytest.mark.parametrize("cname", pyref.CURVE_ORDER)
def test_compress_is_the_canonical_form(cname):
    cv = PF.curve(cname)
    planted = X.planted(cname)
    rows = X.planted_rows(cname)
    pts, st = host_decompress(cname, rows, 0)
    back = host_compress(cname, pts)
    seen = {}
    for q, s, b, pt in zip(planted, st, back, pts):
        canon = X.encode(cname, cv.dec(pt))      # the model's canonical form of what was decoded
        assert b.tobytes() == canon, q.name
        if s:
            assert b.tobytes() == X.encode(cname, None), q.name
        elif q.cls in ("valid", "identity", "off_subgroup"):
            assert b.tobytes() == q.data, q.name          # canonical in, the same bytes out
        else:
            assert q.cls in ("inf_with_x", "y_zero"), q.name
            seen[q.cls] = seen.get(q.cls, 0) + (b.tobytes() != q.data)
    if not X.FORMS[cname][1]:
        assert seen.get("inf_with_x") == 2       # accepted, not canonical: the identity's canonical form comes back
    if cname == "BLS12_377_G1":
        assert seen.get("y_zero") == 1           # y = 0 with the larger bit: comes back without it
    chain, chain_pts = X._chain(cname, 40)
    assert np.array_equal(host_compress(cname, chain_pts), chain)
    assert np.array_equal(host_decompress(cname, chain, 1)[0], chain_pts)


def sqrt_vectors(cname):
    """(names, inputs, expected outputs, expected ok) of the square-root hook, as Montgomery limbs"""
    cv = PF.curve(cname)
    items = X.sqrt_inputs(cname)
    a = np.stack([cv.F.enc(v) for _, v in items])
    roots = [X.smaller_root(cv, v) for _, v in items]
    want = np.stack([cv.F.enc(r) for r, _ in roots])
    ok = np.array([k for _, k in roots], dtype=np.uint8)
    return [n for n, _ in items], a, want, ok


@pytest.mark.parametrize("cname", pyref.CURVE_ORDER)
def test_the_square_root_hook_on_inputs_no_curve_point_reaches(cname):
    names, a, want, ok = sqrt_vectors(cname)
    cv = PF.curve(cname)
    by = dict(zip(names, ok.tolist()))
    assert by["zero"] == 1 and by["one"] == 1
    if cv.F.beta is None:
        assert by["generator"] == 0 and all(by["square%d" % i] == 1 and by["nonresidue%d" % i] == 0 for i in range(6))
        assert by["p_minus_1"] == (1 if cv.p % 4 == 1 else 0)
        if cname == "BLS12_377_G1":              # every trip count of the Tonelli-Shanks loop; order 2^46 is a non-residue
            assert [by["order_2^%d" % k] for k in range(47)] == [1] * 46 + [0]
    else:
        assert all(by["c1_zero_residue%d" % i] == by["c1_zero_nonresidue%d" % i] == by["c1_zero_beta_square%d" % i] == 1 for i in range(3))
        assert all(by["norm_nonresidue%d" % i] == 0 and by["delta_first%d" % i] == by["delta_second%d" % i] == 1 for i in range(3))
        i = names.index("c1_zero_nonresidue0")   # the purely imaginary root
        assert cv.F.dec(want[i])[0] == 0 and cv.F.dec(want[i])[1] != 0
    out = np.full_like(a, 0xEEEEEEEEEEEEEEEE)
    got = np.full(len(a), 0xEE, dtype=np.uint8)
    assert _lib.test_lib().ark_hip_test_host_coord_sqrt(pyref.CURVE_ORDER.index(cname), _vp(a), _vp(out), _vp(got), len(a)) == 0
    assert got.tolist() == ok.tolist(), [n for n, x, y in zip(names, got, ok) if x != y]
    assert np.array_equal(out, want), [n for n, x, y in zip(names, out, want) if not np.array_equal(x, y)]


def test_generated_codec_constants_are_current():
    """csrc/codec_consts.hpp is what tools/gen_constants.py emits, and its numbers are what they claim to be"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_constants", os.path.join(ROOT, "tools", "gen_constants.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fc = {name: dict(p=p, **gen.field_consts(p, g)) for name, p, g in gen.FIELDS}
    assert gen.codec_consts_header(fc) == open(os.path.join(ROOT, "algebra_amd", "csrc", "codec_consts.hpp")).read()
    assert gen.CODEC_FORMS == X.FORMS
    p = pyref.MODULI["BLS12_377_FQ"][0]
    s, q = pyref.two_adicity(p)
    omega = X.codec_root_of_unity()
    assert s == 46 and pow(omega, 1 << 46, p) == 1 and pow(omega, 1 << 45, p) == p - 1
    for name in ("BN254_FQ", "BLS12_381_FQ"):
        assert pyref.MODULI[name][0] % 4 == 3
    assert gen.sqrt_plan(p, 15)["products"] == 1590


def test_standalone_host_program_under_address_and_ub_sanitizers(tmp_path):
    """sw_decompress_point / sw_compress_point / coord_sqrt in a program of their own (tests/point_codec_host.hip), a host-only
    build with -fsanitize=address,undefined: every planted encoding of every curve, validate 0 / 1, every method"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    files = []
    for cid, cname in enumerate(pyref.CURVE_ORDER):
        cv = PF.curve(cname)
        rows = X.planted_rows(cname)
        combos = [(v, m) for v in (0, 1) for m in ((0, 1, 2) if cname == "BLS12_381_G1" else (0, 1))]
        _, a, want, ok = sqrt_vectors(cname)
        parts = [np.array([cid, len(rows), len(combos), len(a)], dtype=np.uint64).tobytes(), rows.tobytes()]
        for v, m in combos:
            pts, st, _ = X.model(cname, rows, bool(v))
            parts += [np.array([v, m], dtype=np.uint64).tobytes(), st.tobytes(), np.ascontiguousarray(pts).tobytes()]
        first = X.model(cname, rows, False)[0]
        parts.append(b"".join(X.encode(cname, cv.dec(r)) for r in first))
        parts += [np.ascontiguousarray(a).tobytes(), np.ascontiguousarray(want).tobytes(), ok.tobytes()]
        path = str(tmp_path / ("%s.bin" % cname))
        with open(path, "wb") as f:
            f.write(b"".join(parts))
        files.append(path)
    exe = str(tmp_path / "point_codec_host")
    subprocess.check_call([hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "point_codec_host.hip"), "-o", exe], timeout=600)
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(": ok") == 5, out.stdout
