"""CPU-side checks of the lookup-by-value entries (no GPU needed): the two entries are public C ABI and the slot hook is a test
hook, with the same arity in the header, `_lib.SYMBOLS` / `TEST_SYMBOLS`, ark-hip-sys and both mirrors; the plan answers for
every table length without a device; argument errors come before any device is touched; the hook is deterministic, in range
and sensitive to every word; the search for colliding elements finds the GPU collision test's data; and the dictionary model of
tests/lookup_ref.py agrees with a quadratic search.  The kernels are checked on the GPU by tests/test_gpu_lookup.py."""
import ctypes as C
import os
import re

import numpy as np

from algebra_amd import _lib
import algebra_amd as A
import lookup_ref as R
import pyref
from test_grand_product_host import _decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ark_hip_fr_lookup_device": 8, "ark_hip_fr_lookup_plan": 3}
HOOKS = {"ark_hip_test_lookup_slot": 4}
ERR_ARG, ERR_NO_DEVICE = -1, -5
FIDS = {"BN254_FR": 1, "BLS12_381_FR": 3, "BLS12_377_FR": 5}
MAX_TABLE = 1 << 28


def test_the_entries_are_public_c_abi_and_the_hook_is_a_hook():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    i, j = hdr.index("#ifdef ARK_HIP_TEST_HOOKS"), hdr.index("#endif /* ARK_HIP_TEST_HOOKS */")
    public, hooks = _decls(hdr[:i] + hdr[j:]), _decls(hdr[i:j])
    L, T = _lib.lib(), _lib.test_lib()
    for name, arity in NAMES.items():
        assert public.get(name) == arity and name not in hooks, name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == arity and name not in _lib.TEST_SYMBOLS, name
        assert hasattr(L, name), name
    for name, arity in HOOKS.items():
        assert hooks.get(name) == arity and name not in public, name
        assert name in _lib.TEST_SYMBOLS and len(_lib.TEST_SYMBOLS[name][1]) == arity and name not in _lib.SYMBOLS, name
        assert hasattr(T, name), name
        try:                                                  # the product library does not export it
            getattr(C.CDLL(_lib.LIB_PATH), name)
            exported = os.path.realpath(_lib.LIB_PATH) != os.path.realpath(_lib.TEST_LIB_PATH)
        except AttributeError:
            exported = False
        assert not exported, name
    assert re.search(r"#define ARK_HIP_LOOKUP_MISSING 0xFFFFFFFFu", hdr) and A.mle.LOOKUP_MISSING == R.MISSING == 0xFFFFFFFF
    at = hdr.index("int ark_hip_fr_lookup_device")
    doc = " ".join(hdr[at - 3200:at].split())
    assert "FIRST occurrence receives all the counts and the later ones receive zero" in doc and "sum_j m_j / (gamma + t_j)" in doc
    exports = open(os.path.join(ROOT, "algebra_amd", "csrc", "exports.map")).read()
    assert "global: ark_hip_*;" in exports and "local: *;" in exports      # every entry above matches the one pattern


def test_rust_and_cpp_mirrors_have_the_entries():
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    found = dict((n, len([a for a in args.split(",") if a.strip()]))
                 for n, args in re.findall(r"pub fn (ark_hip_\w+)\s*\(([^;]*?)\)\s*(?:->\s*[^;]+)?;", ext, flags=re.S))
    for name, arity in NAMES.items():
        assert found.get(name) == arity, name
    for name in HOOKS:
        assert name not in src, name
    assert re.search(r"ARK_HIP_LOOKUP_MISSING: u32 = 0xFFFF_FFFF", src)
    rust = open(os.path.join(ROOT, "rust", "ark-hip", "src", "mle.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for name in NAMES:
        assert "sys::%s(" % name in rust, name
        assert name + "(" in hpp, name
    for method in ("lookup", "lookup_plan"):
        assert re.search(r"\bfn %s\b" % method, rust), method
        assert re.search(r"\b%s\(" % method, hpp[hpp.index("class DenseMultilinearExtension"):]), method
    assert callable(A.lookup_plan) and callable(A.DenseMultilinearExtension.lookup)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "`%s`" % name in integ, name


def _plan(table_len):
    c, b = C.c_uint(0xDEAD), C.c_size_t(0xDEAD)
    assert _lib.lib().ark_hip_fr_lookup_plan(table_len, C.byref(c), C.byref(b)) == 0, table_len
    return c.value, b.value


def test_the_plan_answers_for_every_size_without_a_device():
    lens = list(range(1, 1026))
    for k in range(1, 29):
        lens += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    lens = sorted({n for n in lens if 1 <= n <= MAX_TABLE})
    assert lens[-1] == MAX_TABLE
    last = 0
    for n in lens:
        c, b = _plan(n)
        assert c >= 1 and (1 << c) >= 2 * n, (n, c)
        assert c == 1 or (1 << (c - 1)) < 2 * n, (n, c)
        assert b >= last and b >= 4 << c and b % 32 == 0, (n, c, b)      # room for the slots, whole elements, monotone
        last = b
        assert A.lookup_plan(n) == (c, b)
    assert _plan(1) == _plan(1) and _plan(1)[0] == 1 and _plan(64)[0] == 7 and _plan(65)[0] == 8
    f = _lib.lib().ark_hip_fr_lookup_plan
    c, b = C.c_uint(), C.c_size_t()
    assert f(0, C.byref(c), C.byref(b)) == ERR_ARG
    assert f(MAX_TABLE + 1, C.byref(c), C.byref(b)) == ERR_ARG
    assert f(64, None, C.byref(b)) == ERR_ARG
    assert f(64, C.byref(c), None) == ERR_ARG


def test_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    FR = 3
    B = 1 << 24                                      # non-null "device pointers" that are never dereferenced
    p = C.c_void_p
    t, w, ix, m = p(B), p(2 * B), p(3 * B), p(4 * B)
    miss = C.c_uint64(7)
    out = C.byref(miss)
    f = L.ark_hip_fr_lookup_device
    TL, N = 64, 512
    for field in (99, -1, 0, 2, 4):                  # unknown ids and the base fields
        assert f(field, t, TL, w, N, ix, m, out) == ERR_ARG
    assert f(FR, t, 0, w, N, ix, m, out) == ERR_ARG                  # an empty table
    assert f(FR, t, MAX_TABLE + 1, w, N, ix, p(1 << 50), out) == ERR_ARG
    assert f(FR, t, TL, w, 1 << 32, p(1 << 50), m, out) == ERR_ARG   # n >= 2^32
    assert f(FR, None, TL, w, N, ix, m, out) == ERR_ARG              # a null input with a non-zero length
    assert f(FR, t, TL, None, N, ix, m, out) == ERR_ARG
    assert f(FR, None, TL, None, 0, None, m, out) == ERR_ARG
    assert f(FR, t, TL, w, N, None, None, None) == ERR_ARG           # nothing is asked for
    assert f(FR, t, TL, None, 0, None, None, None) == ERR_ARG
    # an output on an input, in one byte at either end
    for buf, blen in ((B, TL * 32), (2 * B, N * 32)):
        for out_m in (buf, buf + blen - 1, buf - TL * 32 + 1):
            assert f(FR, t, TL, w, N, ix, p(out_m), out) == ERR_ARG, (buf, out_m)
            assert f(FR, t, TL, w, N, None, p(out_m), None) == ERR_ARG
        for out_i in (buf, buf + blen - 1, buf - N * 4 + 1):
            assert f(FR, t, TL, w, N, p(out_i), m, out) == ERR_ARG, (buf, out_i)
            assert f(FR, t, TL, w, N, p(out_i), None, None) == ERR_ARG
    # the two outputs on each other
    for out_i in (4 * B, 4 * B + TL * 32 - 1, 4 * B - N * 4 + 1):
        assert f(FR, t, TL, w, N, p(out_i), m, out) == ERR_ARG
    assert miss.value == 7
    if L.ark_hip_device_count() == 0:                # well-formed calls: loud refusal, no CPU fallback
        for fid in (1, 3, 5):
            assert f(fid, t, TL, w, N, ix, m, out) == ERR_NO_DEVICE
            assert f(fid, t, TL, w, N, ix, None, None) == ERR_NO_DEVICE
            assert f(fid, t, TL, w, N, None, m, None) == ERR_NO_DEVICE
            assert f(fid, t, TL, w, N, None, None, out) == ERR_NO_DEVICE      # a membership check
            assert f(fid, t, TL, t, TL, ix, m, out) == ERR_NO_DEVICE          # the inputs may be the same pointer
            assert f(fid, t, TL, p(B + 32), TL - 1, ix, m, out) == ERR_NO_DEVICE     # ... or overlap
            assert f(fid, t, TL, None, 0, None, m, None) == ERR_NO_DEVICE     # no witness: d_values may be null
            assert f(fid, t, TL, w, N, p(B + TL * 32), p(2 * B + N * 32), out) == ERR_NO_DEVICE   # adjacent, not overlapping
            assert f(fid, t, TL, w, N, p(4 * B + TL * 32), m, out) == ERR_NO_DEVICE
            assert f(fid, t, MAX_TABLE, w, (1 << 32) - 1, p(1 << 50), p(1 << 52), out) == ERR_NO_DEVICE


def test_the_hook_is_deterministic_in_range_and_sensitive_to_every_word():
    T = _lib.test_lib()
    f = T.ark_hip_test_lookup_slot
    slot = C.c_uint32()
    el = (C.c_uint64 * 4)(1, 2, 3, 4)
    for field in (99, -1, 0, 2, 4):
        assert f(field, el, 7, C.byref(slot)) == ERR_ARG
    assert f(3, None, 7, C.byref(slot)) == ERR_ARG and f(3, el, 7, None) == ERR_ARG
    assert f(3, el, 0, C.byref(slot)) == ERR_ARG and f(3, el, 30, C.byref(slot)) == ERR_ARG
    for fname, fid in FIDS.items():
        vals = R.random_elements(fname, 64, 11) + [0, pyref.MODULI[fname][0] - 1]
        for c in (1, 2, 7, 17, 29):
            slots = [R.home_slot(T, fid, v, c) for v in vals]
            assert slots == [R.home_slot(T, fid, v, c) for v in vals], "deterministic"
            assert all(0 <= s < (1 << c) for s in slots), c
            assert len(set(slots)) > 1
        # the same words give the same slot in every field: one function of the words and capacity_log
        assert [R.home_slot(T, fid, v, 17) for v in vals[:8]] == [R.home_slot(T, 3, v, 17) for v in vals[:8]]
        # one bit of one word: at capacity 2^20 an unrelated slot agrees once in a million; of 64 elements at most 2 may
        for k in range(8):
            moved = sum(R.home_slot(T, fid, v, 20) != R.home_slot(T, fid, v ^ (1 << (32 * k + 5)), 20) for v in vals[:64])
            assert moved >= 62, (fname, k, moved)
            assert R.words(vals[0] ^ (1 << (32 * k + 5)))[k] != R.words(vals[0])[k]


def test_the_search_finds_the_collision_tests_elements():
    """capacity 2^7, home slot 2^7 - 2: 48 table values and 16 absent ones within the stated budget, in every field"""
    T = _lib.test_lib()
    for fname, fid in FIDS.items():
        found = R.colliding(T, fid, fname, 7, (1 << 7) - 2, 64)
        assert len(found) == 64 and len(set(found)) == 64, (fname, len(found))
        assert all(R.home_slot(T, fid, v, 7) == 126 for v in found)
        assert all(v < pyref.MODULI[fname][0] for v in found)


def test_the_model_against_a_quadratic_search():
    rng = np.random.default_rng(41)
    assert R.lookup([5, 7, 5], [5, 9, 7, 5]) == ([0, R.MISSING, 1, 0], [2, 1, 0], 1)
    assert R.lookup([3], []) == ([], [0], 0)
    for table_len, n, pool in ((1, 5, 2), (7, 40, 5), (64, 300, 40), (100, 257, 300), (33, 0, 10)):
        table = [int(v) for v in rng.integers(0, pool, size=table_len)]      # a small pool: repeated table values
        values = [int(v) for v in rng.integers(0, pool + 3, size=n)]          # ... and cells that are not in the table
        got = R.lookup(table, values)
        assert got == R.lookup_naive(table, values), (table_len, n)
        idx, m, missing = got
        assert sum(m) + missing == n and all(i == R.MISSING or table[i] == v for i, v in zip(idx, values))
        assert all(m[j] == 0 for j in range(table_len) if table.index(table[j]) != j)
