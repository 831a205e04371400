"""CPU-side checks of the base-set validation (no GPU needed): the two entries and the host hook are C ABI with the same
arity in the header, `_lib.SYMBOLS` / `TEST_SYMBOLS`, ark-hip-sys and ark_hip.hpp; argument errors come before any device is
touched; and over the planted points of tests/check_fixtures.py the HOST build of sw_check_point (csrc/pointcheck.cuh: the
function the kernel runs) gives the status bytes of the Python-integer model, for all five curves, every mask and both
methods.  Every comparison is exact.  The kernel is checked on the GPU by tests/test_gpu_check_bases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from algebra_amd import _lib
import check_fixtures as CF
import point_fixtures as PF
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = {"ark_hip_sw_check_device": 7, "ark_hip_sw_check": 7}
HOOKS = {"ark_hip_test_host_sw_check": 6}
ERR_ARG = -1
G1_381 = pyref.CURVE_ORDER.index("BLS12_381_G1")


def _decls(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char\*)\s+(ark_hip_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_the_entries_are_c_abi_and_the_hook_is_a_hook():
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
    msm_rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "msm.rs")).read()
    assert re.search(r"pub fn check_bases<P: HipServed>\(", msm_rs) and "sys::ark_hip_sw_check(" in msm_rs
    assert "check_bases" in open(os.path.join(ROOT, "rust", "ark-hip", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for name in PUBLIC:
        assert name + "(" in hpp, name
    assert "struct BaseCheck" in hpp and re.search(r"\bcheck_bases\(", hpp) and re.search(r"\bcheck_bases_device\(", hpp)
    import algebra_amd
    assert callable(algebra_amd.check_bases)


def test_argument_errors_come_before_any_device_use():
    L, T = _lib.lib(), _lib.test_lib()
    d = C.c_void_p(1 << 20)                      # a non-null "device pointer" that is never dereferenced
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    row = (C.c_uint64 * 24)()
    st = (C.c_uint8 * 4)()
    for fn, ptr in ((L.ark_hip_sw_check_device, d), (L.ark_hip_sw_check, C.cast(row, C.c_void_p))):
        out[:] = [7, 7, 7, 7]
        assert fn(5, ptr, 1, 3, 0, None, out) == ERR_ARG and fn(-1, ptr, 1, 3, 0, None, out) == ERR_ARG
        assert fn(1, ptr, 1, 0, 0, None, out) == ERR_ARG and fn(1, ptr, 1, 4, 0, None, out) == ERR_ARG
        assert fn(1, ptr, 1, 3, 3, None, out) == ERR_ARG and fn(1, ptr, 1, 3, -1, None, out) == ERR_ARG
        assert fn(1, None, 1, 3, 0, None, out) == ERR_ARG
        assert fn(1, ptr, 1, 3, 0, None, None) == ERR_ARG
        for curve in range(5):                   # the endomorphism test is BLS12-381 G1's alone
            if curve != G1_381:
                assert fn(curve, ptr, 1, 3, 2, None, out) == ERR_ARG, curve
        assert list(out) == [7, 7, 7, 7]
        for curve in range(5):                   # n = 0: {0, 0, 0, 0}, whatever the pointers
            out[:] = [7, 7, 7, 7]
            assert fn(curve, None, 0, 3, 0, None, out) == 0 and list(out) == [0, 0, 0, 0]
        if L.ark_hip_device_count() == 0:        # a well-formed call: loud refusal, no CPU fallback
            assert fn(1, ptr, 1, 3, 0, None, out) == -5
    rp = C.cast(row, C.c_void_p)
    assert T.ark_hip_test_host_sw_check(5, rp, 1, 3, 1, st) == ERR_ARG
    assert T.ark_hip_test_host_sw_check(1, rp, 1, 0, 1, st) == ERR_ARG
    assert T.ark_hip_test_host_sw_check(1, rp, 1, 3, 3, st) == ERR_ARG
    assert T.ark_hip_test_host_sw_check(1, None, 1, 3, 1, st) == ERR_ARG
    assert T.ark_hip_test_host_sw_check(1, rp, 1, 3, 1, None) == ERR_ARG
    for curve in range(5):
        if curve != G1_381:
            assert T.ark_hip_test_host_sw_check(curve, rp, 1, 3, 2, st) == ERR_ARG, curve


def _host(cname, rows, checks, method):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    st = np.full(rows.shape[0], 0xEE, dtype=np.uint8)
    rc = _lib.test_lib().ark_hip_test_host_sw_check(pyref.CURVE_ORDER.index(cname), rows.ctypes.data_as(C.c_void_p), rows.shape[0],
                                                    checks, method, st.ctypes.data_as(C.c_void_p))
    assert rc == 0, (cname, checks, method, rc)
    return st


@pytest.mark.parametrize("cname", pyref.CURVE_ORDER)
def test_host_twin_agrees_with_the_model_on_every_planted_point(cname):
    planted = CF.planted(cname)                  # asserts the number of points per class and each class's status
    rows = CF.planted_rows(cname)
    names = [q.name for q in planted]
    for checks in (1, 2, 3):
        for method in (0, 1, 2):
            if method == 2 and cname != "BLS12_381_G1":
                continue
            want, _ = CF.model(cname, rows, checks, 2 if method == 2 else 1)   # the status does not depend on the method
            got = _host(cname, rows, checks, method)
            assert got.tolist() == want.tolist(), (cname, checks, method, [n for n, a, b in zip(names, got, want) if a != b])
    full, summary = CF.model(cname, rows, 3)
    classes = [CF.CLASS_STATUS[q.cls] for q in planted]
    if cname in CF.COFACTOR_ONE:
        classes = [0 if q.cls == "off_subgroup" else c for q, c in zip(planted, classes)]
    assert full.tolist() == classes
    assert summary == [7, classes.count(1), classes.count(2), classes.count(3)]      # seven valid points come first


def test_the_endomorphism_model_agrees_with_the_ladder_over_r():
    """phi(P) = -[x^2]P with the GENERATED beta against [r]P = O on every planted BLS12-381 G1 point: on the curve the two
    predicates are the same (Scott, eprint 2021/1130 section 6); off the curve both masks that look at the curve say 2."""
    cname = "BLS12_381_G1"
    cv = PF.curve(cname)
    beta = CF.endo_beta()
    assert beta != 1 and pow(beta, 3, cv.p) == 1
    g = PF.generator(cname)
    x2 = CF.BLS12_381_X ** 2
    assert (beta * g[0] % cv.p, g[1]) == cv.neg(CF.ladder(cv, g, x2))
    assert cv.r == CF.BLS12_381_X ** 4 - x2 + 1
    for q in CF.planted(cname):
        for checks in (1, 3):
            assert CF.model_status(cname, q.row, checks, 1) == CF.model_status(cname, q.row, checks, 2), (q.name, checks)
        if q.cls in ("valid", "off_subgroup", "small_order"):
            assert CF.model_status(cname, q.row, 2, 1) == CF.model_status(cname, q.row, 2, 2), q.name
    for checks in (1, 3):                        # ... and so do the two methods of the host twin, byte for byte
        rows = CF.planted_rows(cname)
        assert _host(cname, rows, checks, 1).tolist() == _host(cname, rows, checks, 2).tolist()


def test_the_small_order_points_exercise_the_equal_and_opposite_branches():
    """the ladder over r adds with the accumulator at +-P: 78 / 52 / 27 / 17 times for the order-3 points of BLS12-381 G1 and
    BLS12-377 G1, the order-11 point and the order-13 point"""
    assert CF.ladder_meets("BLS12_381_G1", "order3_a") == 78 and CF.ladder_meets("BLS12_381_G1", "order3_b") == 78
    assert CF.ladder_meets("BLS12_377_G1", "order3_a") == 52
    assert CF.ladder_meets("BLS12_381_G1", "order11") == 27
    assert CF.ladder_meets("BLS12_381_G2", "order13") == 17


def test_generated_check_constants_are_current():
    """csrc/check_consts.hpp is what tools/gen_constants.py emits (r, COEFF_B, beta, x^2)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_constants", os.path.join(ROOT, "tools", "gen_constants.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fc = {name: dict(p=p, **gen.field_consts(p, g)) for name, p, g in gen.FIELDS}
    assert gen.check_consts_header(fc) == open(os.path.join(ROOT, "algebra_amd", "csrc", "check_consts.hpp")).read()
    beta, x2 = gen.endo_beta_bls12_381()
    assert beta == CF.endo_beta() and x2 == CF.BLS12_381_X ** 2


def test_standalone_host_program_under_address_and_ub_sanitizers(tmp_path):
    """sw_check_point in a program of its own (tests/check_point_host.hip), a host-only build with
    -fsanitize=address,undefined: every planted point of every curve, every mask, every method"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    files = []
    for cid, cname in enumerate(pyref.CURVE_ORDER):
        rows = CF.planted_rows(cname)
        combos = [(c, m) for c in (1, 2, 3) for m in ((0, 1, 2) if cname == "BLS12_381_G1" else (0, 1))]
        words = [np.array([cid, len(rows), len(combos)], dtype=np.uint64), np.ascontiguousarray(rows).reshape(-1)]
        for c, m in combos:
            words.append(np.array([c, m], dtype=np.uint64))
            words.append(CF.model(cname, rows, c, 2 if m == 2 else 1)[0].astype(np.uint64))
        path = str(tmp_path / ("%s.bin" % cname))
        np.concatenate(words).tofile(path)
        files.append(path)
    exe = str(tmp_path / "check_point_host")
    subprocess.check_call([hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "check_point_host.hip"), "-o", exe], timeout=600)
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(": ok") == 5, out.stdout
