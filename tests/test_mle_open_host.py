"""CPU-side checks of the multilinear-opening entries (no GPU needed): the four entries are public C ABI with the same arity
in the header, `_lib.SYMBOLS`, ark-hip-sys, ark_hip.hpp and the Rust mirror; the two plans answer for every num_vars < 64
without a device and are monotone; argument errors come before any device is touched; and the big-integer model of
tests/mle_open_ref.py satisfies the identities that define what it models.  The kernels are checked on the GPU by
tests/test_gpu_mle_open.py."""
import ctypes as C
import os
import re

import numpy as np

from algebra_amd import _lib
import mle_open_ref as R
import mle_ref
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ark_hip_mle_eq_table_device": 5, "ark_hip_mle_quotients_device": 6, "ark_hip_mle_eq_plan": 5,
         "ark_hip_mle_quotients_plan": 5}
PLANS = ("ark_hip_mle_eq_plan", "ark_hip_mle_quotients_plan")
ERR_ARG, ERR_NO_DEVICE = -1, -5
P = pyref.MODULI["BLS12_381_FR"][0]


def _decls(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char\*)\s+(ark_hip_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_the_entries_are_public_c_abi():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    i, j = hdr.index("#ifdef ARK_HIP_TEST_HOOKS"), hdr.index("#endif /* ARK_HIP_TEST_HOOKS */")
    public, hooks = _decls(hdr[:i] + hdr[j:]), _decls(hdr[i:j])
    L = _lib.lib()
    for name, arity in NAMES.items():
        assert public.get(name) == arity, name
        assert name not in hooks
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == arity, name
        assert hasattr(L, name), name
    at = hdr.index("int ark_hip_mle_quotients_device")
    assert "must not overlap" in hdr[at - 1500:at]


def test_rust_and_cpp_mirrors_have_the_entries():
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    found = dict((n, len([a for a in args.split(",") if a.strip()]))
                 for n, args in re.findall(r"pub fn (ark_hip_\w+)\s*\(([^;]*?)\)\s*(?:->\s*[^;]+)?;", ext, flags=re.S))
    for name, arity in NAMES.items():
        assert found.get(name) == arity, name
    mle = open(os.path.join(ROOT, "rust", "ark-hip", "src", "mle.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for name in NAMES:
        if name not in PLANS:
            assert "sys::%s(" % name in mle, name
            assert name + "(" in hpp, name
    for method in ("eq", "quotients", "open"):
        assert re.search(r"\bfn %s\b" % method, mle), method
        assert re.search(r"\b%s\(" % method, hpp[hpp.index("class DenseMultilinearExtension"):]), method


def _plan(entry, num_vars):
    t, ps = C.c_int(), C.c_int()
    widths, tiles = (C.c_int * 8)(*([-7] * 8)), (C.c_int * 8)(*([-7] * 8))
    assert getattr(_lib.lib(), entry)(num_vars, C.byref(t), C.byref(ps), widths, tiles) == 0, (entry, num_vars)
    return t.value, ps.value, list(widths), list(tiles)


def test_the_plans_answer_for_every_size_without_a_device():
    L = _lib.lib()
    W = _plan(PLANS[0], 0)[0]
    assert 1 <= W <= 16
    for entry in PLANS:
        last_passes = 0
        for nv in range(64):
            t, ps, widths, tiles = _plan(entry, nv)
            assert t == W
            assert ps == max(-(-nv // W), 1 if entry == PLANS[0] else 0), (entry, nv)   # the minimum: a launch takes W variables
            assert ps >= last_passes, (entry, nv)                                       # monotone
            last_passes = ps
            assert sum(widths[:ps]) == nv and all(0 <= w <= W for w in widths[:ps]), (entry, nv, widths)
            assert nv == 0 or all(w >= 1 for w in widths[:ps])
            assert widths[ps:] == [0] * (8 - ps) and tiles[ps:] == [0] * (8 - ps)
            assert all(0 <= g <= 3 for g in tiles[:ps])
            if entry == PLANS[0]:
                # launch p writes the table of the top widths[0] + .. + widths[p] variables: the remainder first, whole
                # tiles per wave only, and no fewer tiles per wave in a larger launch
                assert widths[1:ps] == [W] * (ps - 1)
                m = 0
                for w, g in zip(widths[:ps], tiles[:ps]):
                    m += w
                    assert g == 0 or m >= W + g, (nv, widths, tiles)
                assert tiles[:ps] == sorted(tiles[:ps])
            else:
                assert widths[:ps] == sorted(widths[:ps], reverse=True)                 # the fold's order: the remainder last
        # the eq table's last launch takes no fewer tiles per wave as the table grows
        if entry == PLANS[0]:
            lasts = [_plan(entry, nv)[3][_plan(entry, nv)[1] - 1] for nv in range(64)]
            assert lasts == sorted(lasts)
        t, ps, widths, tiles = C.c_int(), C.c_int(), (C.c_int * 8)(), (C.c_int * 8)()
        f = getattr(L, entry)
        assert f(64, C.byref(t), C.byref(ps), widths, tiles) == ERR_ARG
        assert f(5, None, C.byref(ps), widths, tiles) == ERR_ARG
        assert f(5, C.byref(t), None, widths, tiles) == ERR_ARG
        assert f(5, C.byref(t), C.byref(ps), None, tiles) == ERR_ARG
        assert f(5, C.byref(t), C.byref(ps), widths, None) == ERR_ARG


def test_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    FR = 3                                           # BLS12_381_FR
    d, d2 = C.c_void_p(1 << 20), C.c_void_p(1 << 30)  # non-null "device pointers" that are never dereferenced
    el = (C.c_uint64 * (4 * 64))()
    host = C.cast(el, C.c_void_p)
    eq, quot = L.ark_hip_mle_eq_table_device, L.ark_hip_mle_quotients_device
    for field in (99, -1, 0, 2, 4):                  # unknown ids and the base fields
        assert eq(field, host, 4, host, d) == ERR_ARG
        assert quot(field, d, 4, host, d2, host) == ERR_ARG
    assert eq(FR, None, 4, host, d) == ERR_ARG       # a point is needed once there are variables
    assert eq(FR, host, 4, host, None) == ERR_ARG
    assert eq(FR, host, 0, None, None) == ERR_ARG
    assert eq(FR, host, 64, host, d) == ERR_ARG      # num_vars >= 64
    assert eq(FR, host, 59, host, d) == ERR_ARG      # a table whose bytes a size_t cannot count
    assert eq(FR, host, 63, None, d) == ERR_ARG
    assert quot(FR, None, 4, host, d2, host) == ERR_ARG
    assert quot(FR, d, 4, None, d2, host) == ERR_ARG
    assert quot(FR, d, 4, host, None, host) == ERR_ARG
    assert quot(FR, None, 0, None, None, host) == ERR_ARG
    assert quot(FR, d, 64, host, d2, host) == ERR_ARG
    assert quot(FR, d, 59, host, d2, None) == ERR_ARG
    assert quot(FR, d, 4, host, d, host) == ERR_ARG                                     # no in-place form
    assert quot(FR, d, 4, host, C.c_void_p((1 << 20) + 32 * 15), None) == ERR_ARG      # the table's last element
    assert quot(FR, d, 4, host, C.c_void_p((1 << 20) - 32 * 14), host) == ERR_ARG      # the quotients' last element
    if L.ark_hip_device_count() == 0:                # well-formed calls: loud refusal, no CPU fallback
        for fid in (1, 3, 5):
            assert eq(fid, host, 4, host, d) == ERR_NO_DEVICE
            assert eq(fid, host, 4, None, d) == ERR_NO_DEVICE
            assert eq(fid, None, 0, None, d) == ERR_NO_DEVICE
            assert quot(fid, d, 4, host, d2, host) == ERR_NO_DEVICE
            assert quot(fid, d, 4, host, d2, None) == ERR_NO_DEVICE
            assert quot(fid, d, 0, None, None, host) == ERR_NO_DEVICE
            assert quot(fid, d, 4, host, C.c_void_p((1 << 20) + 32 * 16), host) == ERR_NO_DEVICE   # adjacent, not overlapping
            assert quot(fid, d, 4, host, C.c_void_p((1 << 20) - 32 * 15), host) == ERR_NO_DEVICE


def _rand(rng, count):
    return [int.from_bytes(rng.bytes(40), "little") % P for _ in range(count)]


def test_the_eq_model():
    rng = np.random.default_rng(11)
    assert R.eq_table([], 7, P) == [7]
    assert R.eq_table([5], 1, P) == [(1 - 5) % P, 5]
    for nv in range(0, 9):
        r, s = _rand(rng, nv), _rand(rng, 1)[0]
        t = R.eq_table(r, 1, P)
        assert len(t) == 1 << nv and sum(t) % P == 1                                     # sum_b eq(r, b) = 1
        assert t == [mle_ref.eq(b, r, P) for b in range(1 << nv)]                        # the product, entry by entry
        assert R.eq_table(r, s, P) == [v * s % P for v in t] and sum(R.eq_table(r, s, P)) % P == s
        f = _rand(rng, 1 << nv)
        assert sum(a * b for a, b in zip(f, t)) % P == mle_ref.evaluate(f, r, P)         # <f, eq(r)> = f(r)
        for b in {0, (1 << nv) - 1, int(rng.integers(0, 1 << nv))}:                      # a boolean point: an indicator
            ind = R.eq_table([(b >> i) & 1 for i in range(nv)], 1, P)
            assert ind == [1 if k == b else 0 for k in range(1 << nv)]
        Rm = pyref.R_of(P)
        assert R.eq_table_mont(r, s, P, Rm) == [v * Rm % P for v in R.eq_table(r, s, P)]


def test_the_quotient_model():
    rng = np.random.default_rng(12)
    assert R.quotients([9], [], P) == (9, [])
    for nv in range(1, 7):
        f, z = _rand(rng, 1 << nv), _rand(rng, nv)
        value, qs = R.quotients(f, z, P)
        assert value == mle_ref.evaluate(f, z, P)
        assert [len(q) for q in qs] == [R.segment_len(nv, i) for i in range(nv)]
        for _ in range(3):                                                               # the opening identity at random x
            x = _rand(rng, nv)
            assert (mle_ref.evaluate(f, x, P) - value) % P == R.opening_identity_rhs(qs, z, x, P)
        # linear in the table: a Montgomery table goes in as it is
        Rm = pyref.R_of(P)
        vm, qm = R.quotients([a * Rm % P for a in f], z, P)
        assert vm == value * Rm % P and qm == [[a * Rm % P for a in q] for q in qs]


def test_the_segments_tile_the_output():
    for nv in range(0, 64):
        at = 0
        for i in range(nv):
            assert R.segment_offset(nv, i) == at
            at += R.segment_len(nv, i)
        assert at == (1 << nv) - 1
