"""CPU-side checks of the polynomial operations on device vectors (no GPU needed): the six entries are part of the public C
ABI (header outside the test-hook block, `_lib.SYMBOLS`, Rust declarations of the same arity), the scan plan that
ark_hip_poly_evaluate_device / ark_hip_poly_divide_linear_device follow is sane, and argument errors are reported before any
device is touched.  The kernels themselves are checked on the GPU by tests/test_gpu_poly_ops.py."""
import ctypes as C
import os
import re

import numpy as np

from algebra_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ark_hip_poly_evaluate_device": 5, "ark_hip_poly_divide_linear_device": 6, "ark_hip_poly_divide_by_vanishing_device": 6,
         "ark_hip_domain_lagrange_coefficients_device": 4, "ark_hip_fr_inner_product_device": 5, "ark_hip_poly_scan_plan": 3}
ERR_ARG = -1


def _decls(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char\*)\s+(ark_hip_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_the_six_entries_are_public_c_abi():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    i, j = hdr.index("#ifdef ARK_HIP_TEST_HOOKS"), hdr.index("#endif /* ARK_HIP_TEST_HOOKS */")
    public, hooks = _decls(hdr[:i] + hdr[j:]), _decls(hdr[i:j])
    L = _lib.lib()
    for name, arity in NAMES.items():
        assert public.get(name) == arity, name
        assert name not in hooks
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == arity, name
        assert hasattr(L, name), name


def test_rust_declarations_have_the_same_arity():
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    found = dict((n, len([a for a in args.split(",") if a.strip()]))
                 for n, args in re.findall(r"pub fn (ark_hip_\w+)\s*\(([^;]*?)\)\s*(?:->\s*[^;]+)?;", ext, flags=re.S))
    for name, arity in NAMES.items():
        assert found.get(name) == arity, name
    dev = open(os.path.join(ROOT, "rust", "ark-hip", "src", "device.rs")).read()
    for name in NAMES:
        if name != "ark_hip_poly_scan_plan":
            assert "sys::%s(" % name in dev, name
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for name in NAMES:
        if name != "ark_hip_poly_scan_plan":
            assert name + "(" in hpp, name


def _plan(n):
    t, lv = C.c_int(), C.c_int()
    assert _lib.lib().ark_hip_poly_scan_plan(n, C.byref(t), C.byref(lv)) == 0
    return t.value, lv.value


def test_scan_plan():
    T, lv = _plan(0)
    assert T >= 256 and T & (T - 1) == 0 and lv == 1
    # one level while a tile holds everything; one more exactly when the tile count exceeds what the levels so far cover
    cover, want = T, 1
    seams = []
    while cover < (1 << 50):
        seams.append((cover, want))
        cover *= T
        want += 1
    for n, lv in seams:
        assert _plan(n) == (T, lv), n
        assert _plan(n + 1) == (T, lv + 1), n
    for n in (1, 2, T - 1, T):
        assert _plan(n)[1] == 1
    for n in (T + 1, 3 * T + 5, T * T - 1, T * T):
        assert _plan(n)[1] == 2
    assert _plan(T * T + 1)[1] == 3
    # monotone in n, the tile never changes
    rng = np.random.default_rng(3)
    sizes = sorted(set(int(v) for v in rng.integers(0, 1 << 34, size=400)) | {0, 1, T, T + 1, T * T, T * T + 1, T ** 3, T ** 3 + 1})
    prev = 0
    for n in sizes:
        t, lv = _plan(n)
        assert t == T and lv >= prev
        prev = lv
        k, m = 1, n                                   # levels = the number of times n is cut into tiles until one is left
        while m > T:
            m = -(-m // T)
            k += 1
        assert lv == k, n
    assert _lib.lib().ark_hip_poly_scan_plan(5, None, None) == ERR_ARG
    assert _lib.lib().ark_hip_poly_scan_plan(5, C.byref(C.c_int()), None) == ERR_ARG


def test_argument_errors_come_before_any_device_use():
    """field = 99 and null pointers give ARK_HIP_ERR_ARG, with or without a GPU: the checks run before a device is looked for
    (without one every well-formed call returns ARK_HIP_ERR_NO_DEVICE instead)."""
    L = _lib.lib()
    FR = 3                                           # BLS12_381_FR
    d = C.c_void_p(4096)                             # a non-null "device pointer" that is never dereferenced
    el = (C.c_uint64 * 4)()
    host = C.cast(el, C.c_void_p)
    dom = _lib.Radix2DomainStruct()
    assert L.ark_hip_radix2_domain_new(FR, 8, C.byref(dom)) == 0
    assert L.ark_hip_poly_evaluate_device(99, d, 4, host, host) == ERR_ARG
    assert L.ark_hip_poly_evaluate_device(0, d, 4, host, host) == ERR_ARG          # a base field is not served
    assert L.ark_hip_poly_evaluate_device(FR, None, 4, host, host) == ERR_ARG
    assert L.ark_hip_poly_evaluate_device(FR, d, 4, None, host) == ERR_ARG
    assert L.ark_hip_poly_evaluate_device(FR, d, 4, host, None) == ERR_ARG
    assert L.ark_hip_poly_divide_linear_device(99, d, 4, host, d, host) == ERR_ARG
    assert L.ark_hip_poly_divide_linear_device(FR, None, 4, host, d, host) == ERR_ARG
    assert L.ark_hip_poly_divide_linear_device(FR, d, 4, None, d, host) == ERR_ARG
    assert L.ark_hip_poly_divide_linear_device(FR, d, 4, host, None, host) == ERR_ARG
    assert L.ark_hip_poly_divide_by_vanishing_device(99, 2, d, 4, d, d) == ERR_ARG
    assert L.ark_hip_poly_divide_by_vanishing_device(FR, 0, d, 4, d, d) == ERR_ARG
    assert L.ark_hip_poly_divide_by_vanishing_device(FR, 2, None, 4, d, d) == ERR_ARG
    assert L.ark_hip_poly_divide_by_vanishing_device(FR, 2, d, 4, None, d) == ERR_ARG
    assert L.ark_hip_poly_divide_by_vanishing_device(FR, 2, d, 4, d, None) == ERR_ARG
    assert L.ark_hip_domain_lagrange_coefficients_device(99, C.byref(dom), host, d) == ERR_ARG
    assert L.ark_hip_domain_lagrange_coefficients_device(FR, None, host, d) == ERR_ARG
    assert L.ark_hip_domain_lagrange_coefficients_device(FR, C.byref(dom), None, d) == ERR_ARG
    assert L.ark_hip_domain_lagrange_coefficients_device(FR, C.byref(dom), host, None) == ERR_ARG
    assert L.ark_hip_domain_lagrange_coefficients_device(1, C.byref(dom), host, d) == ERR_ARG   # a BLS12-381 domain in BN254's Fr
    assert L.ark_hip_fr_inner_product_device(99, d, d, 4, host) == ERR_ARG
    assert L.ark_hip_fr_inner_product_device(FR, None, d, 4, host) == ERR_ARG
    assert L.ark_hip_fr_inner_product_device(FR, d, None, 4, host) == ERR_ARG
    assert L.ark_hip_fr_inner_product_device(FR, d, d, 4, None) == ERR_ARG
    if L.ark_hip_device_count() == 0:                # well-formed calls: loud refusal, no CPU fallback
        assert L.ark_hip_poly_evaluate_device(FR, d, 4, host, host) == -5
        assert L.ark_hip_poly_divide_linear_device(FR, d, 4, host, d, None) == -5
        assert L.ark_hip_poly_divide_by_vanishing_device(FR, 2, d, 4, d, d) == -5
        assert L.ark_hip_domain_lagrange_coefficients_device(FR, C.byref(dom), host, d) == -5
        assert L.ark_hip_fr_inner_product_device(FR, d, d, 4, host) == -5
