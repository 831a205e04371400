"""CPU-side checks of the multilinear-extension entries (no GPU needed): the six entries are public C ABI with the same
arity in the header, `_lib.SYMBOLS`, ark-hip-sys, ark_hip.hpp and the Rust mirror; the fold plan is sane for every
0 <= dim <= num_vars < 64; argument errors come before any device is touched; and the big-integer model of tests/mle_ref.py
reproduces the reference's documented answers.  The kernels are checked on the GPU by tests/test_gpu_mle.py."""
import ctypes as C
import os
import re

import numpy as np

from algebra_amd import _lib
import mle_ref
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ark_hip_mle_fix_variables_device": 6, "ark_hip_mle_evaluate_device": 5, "ark_hip_mle_relabel_device": 7,
         "ark_hip_fr_axpy_device": 6, "ark_hip_mle_fold_plan": 5, "ark_hip_mle_fold_tiles": 3}
ERR_ARG = -1
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
    assert "must not overlap" in hdr[hdr.index("int ark_hip_mle_fix_variables_device") - 1200:hdr.index("int ark_hip_mle_fix_variables_device")]


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
        if name not in ("ark_hip_mle_fold_plan", "ark_hip_mle_fold_tiles"):
            assert "sys::%s(" % name in mle, name
            assert name + "(" in hpp, name
    assert "pub mod mle;" in open(os.path.join(ROOT, "rust", "ark-hip", "src", "lib.rs")).read()
    for method in ("fix_variables", "evaluate", "relabel", "relabel_in_place", "concat", "zero", "is_zero", "num_vars", "to_evaluations"):
        assert re.search(r"\bfn %s\b" % method, mle), method
        assert re.search(r"\b%s\(" % method, hpp[hpp.index("class DenseMultilinearExtension"):]), method


def _plan(num_vars, dim):
    t, ps = C.c_int(), C.c_int()
    widths = (C.c_int * 8)(*([-7] * 8))
    assert _lib.lib().ark_hip_mle_fold_plan(num_vars, dim, C.byref(t), C.byref(ps), widths) == 0, (num_vars, dim)
    return t.value, ps.value, list(widths)


def test_fold_plan():
    W = _plan(0, 0)[0]
    assert 1 <= W <= 16
    for nv in range(64):
        for dim in range(nv + 1):
            t, ps, widths = _plan(nv, dim)
            assert t == W
            assert ps == -(-dim // W), (nv, dim)                  # the minimum: a launch binds at most W variables
            assert sum(widths[:ps]) == dim and all(1 <= w <= W for w in widths[:ps]), (nv, dim, widths)
            assert widths[ps:] == [0] * (8 - ps)
            assert widths[:ps] == sorted(widths[:ps], reverse=True) and (ps == 0 or widths[0] == max(widths[:ps]))
    L = _lib.lib()
    # tiles per wave: 2^gl tiles never outnumber what the launch's bound bits leave as streams (8 per lane), one tile for
    # launches that bind few bits or have few elements, defined wherever the plan is
    for nv in range(64):
        for dim in range(nv + 1):
            _, ps, widths = _plan(nv, dim)
            tiles = (C.c_int * 8)(*([-7] * 8))
            assert L.ark_hip_mle_fold_tiles(nv, dim, tiles) == 0
            tiles, m = list(tiles), nv
            assert tiles[ps:] == [0] * (8 - ps)
            for w, gl in zip(widths[:ps], tiles[:ps]):
                assert 0 <= gl <= 3 and (8 >> max(w - (W - 3), 0)) << gl <= 8, (nv, dim, w, gl)
                assert gl == 0 or m >= W + gl, (nv, dim, w, gl)      # whole tiles only
                m -= w
    assert L.ark_hip_mle_fold_tiles(5, 6, (C.c_int * 8)()) == ERR_ARG
    assert L.ark_hip_mle_fold_tiles(64, 3, (C.c_int * 8)()) == ERR_ARG
    assert L.ark_hip_mle_fold_tiles(5, 3, None) == ERR_ARG
    t, ps, widths = C.c_int(), C.c_int(), (C.c_int * 8)()
    assert L.ark_hip_mle_fold_plan(5, 6, C.byref(t), C.byref(ps), widths) == ERR_ARG
    assert L.ark_hip_mle_fold_plan(64, 3, C.byref(t), C.byref(ps), widths) == ERR_ARG
    assert L.ark_hip_mle_fold_plan(5, 3, None, C.byref(ps), widths) == ERR_ARG
    assert L.ark_hip_mle_fold_plan(5, 3, C.byref(t), None, widths) == ERR_ARG
    assert L.ark_hip_mle_fold_plan(5, 3, C.byref(t), C.byref(ps), None) == ERR_ARG


def test_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    FR = 3                                           # BLS12_381_FR
    d, d2 = C.c_void_p(1 << 20), C.c_void_p(1 << 30)  # non-null "device pointers" that are never dereferenced
    el = (C.c_uint64 * (4 * 16))()
    host = C.cast(el, C.c_void_p)
    # fix_variables
    assert L.ark_hip_mle_fix_variables_device(99, d, 4, host, 2, d2) == ERR_ARG
    assert L.ark_hip_mle_fix_variables_device(0, d, 4, host, 2, d2) == ERR_ARG       # a base field is not served
    assert L.ark_hip_mle_fix_variables_device(FR, None, 4, host, 2, d2) == ERR_ARG
    assert L.ark_hip_mle_fix_variables_device(FR, d, 4, None, 2, d2) == ERR_ARG
    assert L.ark_hip_mle_fix_variables_device(FR, d, 4, host, 2, None) == ERR_ARG
    assert L.ark_hip_mle_fix_variables_device(FR, d, 4, host, 5, d2) == ERR_ARG      # dim > num_vars
    assert L.ark_hip_mle_fix_variables_device(FR, d, 64, host, 2, d2) == ERR_ARG     # num_vars >= 64
    assert L.ark_hip_mle_fix_variables_device(FR, d, 4, host, 2, d) == ERR_ARG       # no in-place form
    assert L.ark_hip_mle_fix_variables_device(FR, d, 4, host, 2, C.c_void_p((1 << 20) + 32 * 15)) == ERR_ARG   # overlap
    # evaluate
    assert L.ark_hip_mle_evaluate_device(99, d, 4, host, host) == ERR_ARG
    assert L.ark_hip_mle_evaluate_device(FR, None, 4, host, host) == ERR_ARG
    assert L.ark_hip_mle_evaluate_device(FR, d, 4, None, host) == ERR_ARG
    assert L.ark_hip_mle_evaluate_device(FR, d, 4, host, None) == ERR_ARG
    assert L.ark_hip_mle_evaluate_device(FR, d, 64, host, host) == ERR_ARG
    # relabel: the reference's two assertions after ordering a <= b
    assert L.ark_hip_mle_relabel_device(99, d, 8, 1, 4, 2, d2) == ERR_ARG
    assert L.ark_hip_mle_relabel_device(FR, None, 8, 1, 4, 2, d2) == ERR_ARG
    assert L.ark_hip_mle_relabel_device(FR, d, 8, 1, 4, 2, None) == ERR_ARG
    assert L.ark_hip_mle_relabel_device(FR, d, 64, 1, 4, 2, d2) == ERR_ARG
    assert L.ark_hip_mle_relabel_device(FR, d, 8, 1, 7, 2, d2) == ERR_ARG            # b + k > num_vars
    assert L.ark_hip_mle_relabel_device(FR, d, 8, 7, 1, 2, d2) == ERR_ARG            # the same, a and b exchanged
    assert L.ark_hip_mle_relabel_device(FR, d, 8, 2, 3, 2, d2) == ERR_ARG            # overlapping windows
    assert L.ark_hip_mle_relabel_device(FR, d, 8, 3, 2, 2, d) == ERR_ARG
    assert L.ark_hip_mle_relabel_device(FR, d, 8, 1, 4, 2, C.c_void_p((1 << 20) + 32)) == ERR_ARG   # partial overlap of the buffers
    # axpy
    assert L.ark_hip_fr_axpy_device(99, d, host, d, d, 4) == ERR_ARG
    assert L.ark_hip_fr_axpy_device(FR, None, host, d, d, 4) == ERR_ARG
    assert L.ark_hip_fr_axpy_device(FR, d, None, d, d, 4) == ERR_ARG
    assert L.ark_hip_fr_axpy_device(FR, d, host, None, d, 4) == ERR_ARG
    assert L.ark_hip_fr_axpy_device(FR, d, host, d, None, 4) == ERR_ARG
    if L.ark_hip_device_count() == 0:                # well-formed calls: loud refusal, no CPU fallback
        assert L.ark_hip_mle_fix_variables_device(FR, d, 4, host, 2, d2) == -5
        assert L.ark_hip_mle_evaluate_device(FR, d, 4, host, host) == -5
        assert L.ark_hip_mle_relabel_device(FR, d, 8, 1, 4, 2, d2) == -5
        assert L.ark_hip_mle_relabel_device(FR, d, 8, 1, 4, 2, d) == -5
        assert L.ark_hip_fr_axpy_device(FR, d, host, d, d, 4) == -5


def test_the_model_reproduces_the_references_documented_answers():
    assert mle_ref.evaluate([0, 0, 1, 0], [(-2) % P, 17], P) == 51                   # dense.rs:49-56
    assert mle_ref.fix_variables([0, 1, 2, 6], [5], P) == [5, 22]                    # dense.rs:211-221
    assert mle_ref.evaluate([2, 3, 2, 6], [1, 17], P) == 54                          # dense.rs:448-458
    # concat (dense.rs:113-132): f3 = (1 - x_2) f1 + x_2 f2 at (1, 17, 3)
    f1, f2, pt = [2, 3, 2, 6], [0, 0, 0, 1], [1, 17, 3]
    want = ((1 - pt[2]) * mle_ref.evaluate(f1, pt[:2], P) + pt[2] * mle_ref.evaluate(f2, pt[:2], P)) % P
    assert mle_ref.evaluate(f1 + f2, pt, P) == want


def test_the_model_agrees_with_the_references_test_helper():
    rng = np.random.default_rng(5)
    for nv in range(0, 9):
        table = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(1 << nv)]
        point = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(nv)]
        want = mle_ref.evaluate_data_array(table, point, P)                          # dense.rs:476-492
        assert mle_ref.evaluate(table, point, P) == want
        assert sum(v * mle_ref.eq(i, point, P) for i, v in enumerate(table)) % P == want
        for dim in range(nv + 1):                                                    # binding in two steps is binding in one
            part = mle_ref.fix_variables(table, point[:dim], P)
            assert len(part) == 1 << (nv - dim) and mle_ref.evaluate(part, point[dim:], P) == want
    # relabel: the reference's own windows (dense.rs:516-529); evaluating with the point swapped the same way
    nv = 10
    table = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(1 << nv)]
    point = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(nv)]
    for a, b, k in ((2, 2, 1), (3, 4, 1), (7, 5, 1), (2, 5, 3), (0, 5, 5)):
        moved = mle_ref.relabel(table, a, b, k)
        pt = list(point)
        for t in range(k if a != b else 0):
            pt[a + t], pt[b + t] = pt[b + t], pt[a + t]
        assert mle_ref.evaluate(moved, pt, P) == mle_ref.evaluate(table, point, P)
        assert mle_ref.relabel(moved, a, b, k) == table
    assert mle_ref.swap_bits(0b1011, 0, 2, 2) == 0b1110
