"""CPU-side checks of the prefix scans on device vectors (no GPU needed): the big-integer model of tests/prefix_scan_ref.py
against a naive quadratic product, the scan plan, argument errors reported before any device is touched, and the four
entries as part of the public C ABI (header, exports, Python / Rust / C++ mirrors).  The kernels themselves are checked on the
GPU by tests/test_gpu_prefix_scan.py."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from algebra_amd import _lib
import algebra_amd as A
import oracle_lib as O
import prefix_scan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ark_hip_fr_prefix_product_device": 6, "ark_hip_fr_prefix_sum_device": 6, "ark_hip_fr_prefix_ratio_device": 6,
         "ark_hip_prefix_scan_plan": 4}
ERR_ARG = -1
FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]


# ---- the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
def test_the_model_against_a_naive_quadratic_product(fname):
    f = R.Field(fname)
    for n in (0, 1, 2, 9, 40):
        a = R.ints(O.gen_scalars(O.FID[fname], 3 + n, max(n, 1), montgomery=True)[:n])
        if n >= 9:
            a[3] = f.one
            a[4] = f.enc(-1)
            a[5] = f.p - 1
        inc, total = R.prefix_product(f, a, False)
        exc, total2 = R.prefix_product(f, a, True)
        assert inc == [R.naive_product(f, a, i + 1) for i in range(n)]
        assert exc == [R.naive_product(f, a, i) for i in range(n)]
        assert total == total2 == R.naive_product(f, a, n)
        sinc, stotal = R.prefix_sum(f, a, False)
        sexc, _ = R.prefix_sum(f, a, True)
        assert sinc == [sum(a[:i + 1]) % f.p for i in range(n)] and sexc == [sum(a[:i]) % f.p for i in range(n)]
        assert stotal == sum(a) % f.p
        b = R.ints(O.gen_scalars(O.FID[fname], 77 + n, max(n, 1), montgomery=True)[:n])
        z, last = R.prefix_ratio(f, a, b)
        # the recurrence z[i + 1] den[i] = z[i] num[i] and z[0] = 1, on canonical values
        zs = z + [last]
        assert zs[0] == f.one
        for i in range(n):
            assert f.mul(zs[i + 1], b[i]) == f.mul(zs[i], a[i]), (n, i)


def test_the_model_leaves_zeros_in_place():
    f = R.Field("BLS12_381_FR")
    a = [f.enc(v) for v in (2, 3, 5, 7, 11, 13)]
    b = [f.enc(v) for v in (1, 1, 0, 1, 1, 1)]
    z, last = R.prefix_ratio(f, a, b)
    assert z[:3] == [f.enc(1), f.enc(2), f.enc(6)] and z[3:] == [0, 0, 0] and last == 0
    assert f.inv0(0) == 0 and f.mul(f.inv0(f.enc(7)), f.enc(7)) == f.one
    inc, total = R.prefix_product(f, [f.enc(2), 0, f.enc(3)], False)
    assert inc == [f.enc(2), 0, 0] and total == 0
    z, last = R.prefix_ratio(f, [f.enc(2), 0, f.enc(3)], [f.enc(1)] * 3)      # a zero numerator is just a value
    assert z == [f.enc(1), f.enc(2), 0] and last == 0


# ---- the plan -----------------------------------------------------------------------------------------------------------
def _plan(op, n):
    t, lv = C.c_int(), C.c_int()
    assert _lib.lib().ark_hip_prefix_scan_plan(op, n, C.byref(t), C.byref(lv)) == 0
    return t.value, lv.value


@pytest.mark.parametrize("op", [0, 1, 2])
def test_scan_plan(op):
    T, lv = _plan(op, 0)
    assert T >= 256 and T & (T - 1) == 0 and lv == 1
    assert T <= _plan(0, 0)[0]                       # the ratio may use a smaller tile, never a larger one
    assert A.prefix_scan_plan(("product", "sum", "ratio")[op], 5) == (T, 1) == A.prefix_scan_plan(op, 5)
    for n in (1, 2, T - 1, T):
        assert _plan(op, n) == (T, 1), n
    for n in (T + 1, 3 * T + 5, T * T - 1, T * T):
        assert _plan(op, n) == (T, 2), n
    for n in (T * T + 1, T ** 3 if T ** 3 <= 1 << 40 else 1 << 40, 1 << 40):
        assert _plan(op, n)[1] >= 3, n
    assert _plan(op, T * T + 1)[1] == 3
    rng = np.random.default_rng(11 + op)
    prev = 0
    for n in sorted(set(int(v) for v in rng.integers(0, 1 << 40, size=300, endpoint=True)) | {0, 1, T, T + 1, T * T, T * T + 1, 1 << 40}):
        t, lv = _plan(op, n)
        k, m = 1, n                                  # levels = the number of times n is cut into tiles until one is left
        while m > T:
            m = -(-m // T)
            k += 1
        assert t == T and lv == k and lv >= prev, n
        prev = lv


def test_scan_plan_argument_errors():
    L = _lib.lib()
    t, lv = C.c_int(), C.c_int()
    assert L.ark_hip_prefix_scan_plan(0, 5, None, C.byref(lv)) == ERR_ARG
    assert L.ark_hip_prefix_scan_plan(0, 5, C.byref(t), None) == ERR_ARG
    assert L.ark_hip_prefix_scan_plan(3, 5, C.byref(t), C.byref(lv)) == ERR_ARG
    assert L.ark_hip_prefix_scan_plan(-1, 5, C.byref(t), C.byref(lv)) == ERR_ARG


# ---- argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_use():
    """an unknown or unserved field, null pointers with n > 0 and every forbidden overlap give ARK_HIP_ERR_ARG, with or
    without a GPU: the checks run before a device is looked for (without one a well-formed call returns
    ARK_HIP_ERR_NO_DEVICE instead).  The "device pointers" are never dereferenced."""
    L = _lib.lib()
    F = 3                                            # BLS12_381_FR
    n = 64
    a, b, o = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)
    el = (C.c_uint64 * 4)()
    host = C.cast(el, C.c_void_p)

    def off(ptr, elems):
        return C.c_void_p(ptr.value + 32 * elems)

    for entry in (L.ark_hip_fr_prefix_product_device, L.ark_hip_fr_prefix_sum_device):
        for ex in (0, 1):
            assert entry(99, a, n, ex, o, host) == ERR_ARG
            assert entry(0, a, n, ex, o, host) == ERR_ARG                  # a base field is not served
            assert entry(F, None, n, ex, o, host) == ERR_ARG
            assert entry(F, a, n, ex, None, host) == ERR_ARG
            assert entry(F, a, n, ex, off(a, 1), host) == ERR_ARG         # shifted by one element: not the same pointer
            assert entry(F, a, n, ex, off(a, n - 1), None) == ERR_ARG
            assert entry(F, off(a, 5), n, ex, a, None) == ERR_ARG
            assert entry(F, a, (1 << 64) - 1, ex, o, host) == ERR_ARG     # bytes that a size_t cannot count
    ratio = L.ark_hip_fr_prefix_ratio_device
    assert ratio(99, a, b, n, o, host) == ERR_ARG
    assert ratio(0, a, b, n, o, host) == ERR_ARG
    assert ratio(F, None, b, n, o, host) == ERR_ARG
    assert ratio(F, a, None, n, o, host) == ERR_ARG
    assert ratio(F, a, b, n, None, host) == ERR_ARG
    assert ratio(F, a, b, n, off(a, 1), host) == ERR_ARG
    assert ratio(F, a, b, n, off(b, 1), host) == ERR_ARG
    assert ratio(F, a, b, n, off(a, n - 1), None) == ERR_ARG
    assert ratio(F, off(b, 3), b, n, b, None) == ERR_ARG                  # out IS den, but overlaps num
    assert ratio(F, a, off(a, 3), n, a, None) == ERR_ARG                  # out IS num, but overlaps den
    if L.ark_hip_device_count() == 0:                # well-formed calls, allowed aliasing included: loud refusal, no CPU fallback
        for entry in (L.ark_hip_fr_prefix_product_device, L.ark_hip_fr_prefix_sum_device):
            assert entry(F, a, n, 0, o, host) == -5
            assert entry(F, a, n, 1, a, None) == -5
            assert entry(F, None, 0, 0, None, host) == -5
        assert ratio(F, a, b, n, o, host) == -5
        assert ratio(F, a, b, n, a, None) == -5
        assert ratio(F, a, b, n, b, None) == -5


# ---- the public interface ---------------------------------------------------------------------------------------------------
def _decls(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char\*)\s+(ark_hip_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_the_four_entries_are_public_c_abi():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    i, j = hdr.index("#ifdef ARK_HIP_TEST_HOOKS"), hdr.index("#endif /* ARK_HIP_TEST_HOOKS */")
    public, hooks = _decls(hdr[:i] + hdr[j:]), _decls(hdr[i:j])
    block = hdr[hdr.index("polynomial operations on device-resident vectors"):hdr.index("dense multilinear extensions on device-resident")]
    emap = open(os.path.join(ROOT, "algebra_amd", "csrc", "exports.map")).read()
    exported = re.findall(r"global:\s*([^;]+);", emap)
    L = _lib.lib()
    for name, arity in NAMES.items():
        assert public.get(name) == arity, name
        assert name not in hooks and name + "(" in block, name
        assert any(fnmatch.fnmatchcase(name, pat.strip()) for pats in exported for pat in pats.split()), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == arity, name
        assert hasattr(L, name), name


def test_the_mirrors_have_the_entries():
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    found = dict((n, len([a for a in args.split(",") if a.strip()]))
                 for n, args in re.findall(r"pub fn (ark_hip_\w+)\s*\(([^;]*?)\)\s*(?:->\s*[^;]+)?;", ext, flags=re.S))
    dev = open(os.path.join(ROOT, "rust", "ark-hip", "src", "device.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for name, arity in NAMES.items():
        assert found.get(name) == arity, name
        if name != "ark_hip_prefix_scan_plan":
            assert "sys::%s(" % name in dev, name
            assert name + "(" in hpp, name
    for method in ("prefix_product", "prefix_sum", "prefix_ratio"):
        assert hasattr(A.DeviceVec, method)
        assert "pub fn %s(" % method in dev and " %s(" % method in hpp, method
