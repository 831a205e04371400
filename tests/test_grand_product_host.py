"""CPU-side checks of the grand-product entries (no GPU needed): the three entries are public C ABI with the same arity in the
header, `_lib.SYMBOLS`, ark-hip-sys, and are called by ark_hip.hpp and the Rust mirror; the plan answers for every
num_vars < 64 without a device and its launches tile the tree exactly once; argument errors come before any device is
touched; and the big-integer model of tests/grand_product_ref.py proves to its own verifier and that verifier rejects altered
proofs.  The kernels are checked on the GPU by tests/test_gpu_grand_product.py."""
import ctypes as C
import os
import re

import numpy as np

from algebra_amd import _lib
import grand_product_ref as R
import mle_ref
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ark_hip_mle_product_tree_device": 5, "ark_hip_mle_product_tree_plan": 4, "ark_hip_fr_lincomb_device": 7}
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
    at = hdr.index("int ark_hip_mle_product_tree_device")
    assert "must not overlap" in hdr[at - 2000:at]
    assert int(re.search(r"#define ARK_HIP_PRODUCT_TREE_LEVELS (\d+)", hdr).group(1)) == LEVELS


def test_rust_and_cpp_mirrors_have_the_entries():
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    found = dict((n, len([a for a in args.split(",") if a.strip()]))
                 for n, args in re.findall(r"pub fn (ark_hip_\w+)\s*\(([^;]*?)\)\s*(?:->\s*[^;]+)?;", ext, flags=re.S))
    for name, arity in NAMES.items():
        assert found.get(name) == arity, name
    rust = open(os.path.join(ROOT, "rust", "ark-hip", "src", "mle.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for name in NAMES:
        assert "sys::%s(" % name in rust, name
        assert name + "(" in hpp, name
    for method in ("product_tree", "linear_combination"):
        assert re.search(r"\bfn %s\b" % method, rust), method
        assert re.search(r"\b%s\(" % method, hpp[hpp.index("class DenseMultilinearExtension"):]), method
    gp = open(os.path.join(ROOT, "rust", "ark-hip", "src", "grand_product.rs")).read()
    assert re.search(r"\bfn prove\b", gp) and "struct GrandProductProof" in gp
    assert "class GrandProduct" in hpp and "struct GrandProductProof" in hpp


LEVELS = 3      # ARK_HIP_PRODUCT_TREE_LEVELS


def _plan(num_vars):
    ps = C.c_int()
    widths, groups = (C.c_int * 8)(*([-7] * 8)), (C.c_int * 8)(*([-7] * 8))
    assert _lib.lib().ark_hip_mle_product_tree_plan(num_vars, C.byref(ps), widths, groups) == 0, num_vars
    return ps.value, list(widths), list(groups)


def _launches(num_vars):
    """the runs of the plan spelled out launch by launch: [(levels, group_log)]"""
    ps, widths, groups = _plan(num_vars)
    out = []
    for w, g in zip(widths[:ps], groups[:ps]):
        out += [(LEVELS, g)] * (w // LEVELS) if w >= LEVELS else [(w, g)]
    return out


def test_the_plan_answers_for_every_size_without_a_device():
    L = _lib.lib()
    last_launches = 0
    for nv in range(64):
        ps, widths, groups = _plan(nv)
        assert 0 <= ps <= 2 and (ps > 0) == (nv > 0), (nv, ps)
        assert sum(widths[:ps]) == nv and all(w >= 1 for w in widths[:ps]), (nv, widths)
        assert widths[ps:] == [0] * (8 - ps) and groups[ps:] == [0] * (8 - ps)
        assert all(g == 0 for g in groups[:ps])                  # one chunk of 64 outputs per wave, always
        # a run is whole launches of LEVELS levels, or it is the one remainder launch, which comes last
        assert all(w % LEVELS == 0 for w in widths[:max(ps - 1, 0)]), (nv, widths)
        assert ps == 0 or widths[ps - 1] % LEVELS == 0 or widths[ps - 1] < LEVELS
        la = _launches(nv)
        assert sum(w for w, _ in la) == nv and len(la) == -(-nv // LEVELS), (nv, la)   # the fewest launches of <= LEVELS levels
        assert len(la) >= last_launches                                                  # monotone
        last_launches = len(la)
        # the offsets the launches imply tile the 2^nv - 1 elements exactly once, in order
        at, m = 0, nv
        for w, _ in la:
            for a in range(w):
                j = nv - (m - 1 - a)                              # the level that holds L_(m-1-a)
                assert R.level_offset(nv, j) == at and R.level_len(nv, j) == 1 << (m - 1 - a)
                at += R.level_len(nv, j)
            m -= w
        assert m == 0 and at == (1 << nv) - 1
    ps, widths, groups = C.c_int(), (C.c_int * 8)(), (C.c_int * 8)()
    f = L.ark_hip_mle_product_tree_plan
    assert f(64, C.byref(ps), widths, groups) == ERR_ARG
    assert f(5, None, widths, groups) == ERR_ARG
    assert f(5, C.byref(ps), None, groups) == ERR_ARG
    assert f(5, C.byref(ps), widths, None) == ERR_ARG


def test_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    FR = 3                                           # BLS12_381_FR
    d, d2 = C.c_void_p(1 << 20), C.c_void_p(1 << 30)  # non-null "device pointers" that are never dereferenced
    el = (C.c_uint64 * (4 * 64))()
    host = C.cast(el, C.c_void_p)
    tree, lin = L.ark_hip_mle_product_tree_device, L.ark_hip_fr_lincomb_device

    def tabs(*ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)
    for field in (99, -1, 0, 2, 4):                  # unknown ids and the base fields
        assert tree(field, d, 4, d2, host) == ERR_ARG
        assert lin(field, tabs(d.value), 1, host, host, d2, 16) == ERR_ARG
    assert tree(FR, None, 4, d2, host) == ERR_ARG
    assert tree(FR, d, 4, None, host) == ERR_ARG     # a tree is needed once there are variables
    assert tree(FR, None, 0, None, host) == ERR_ARG
    assert tree(FR, d, 64, d2, host) == ERR_ARG      # num_vars >= 64
    assert tree(FR, d, 59, d2, None) == ERR_ARG      # a table whose bytes a size_t cannot count
    assert tree(FR, d, 63, d2, host) == ERR_ARG
    assert tree(FR, d, 4, d, host) == ERR_ARG                                           # no in-place form
    assert tree(FR, d, 4, C.c_void_p((1 << 20) + 32 * 15), None) == ERR_ARG            # the table's last element
    assert tree(FR, d, 4, C.c_void_p((1 << 20) - 32 * 14), host) == ERR_ARG            # the tree's last element
    assert lin(FR, None, 1, host, host, d2, 16) == ERR_ARG
    assert lin(FR, tabs(d.value), 1, None, host, d2, 16) == ERR_ARG
    assert lin(FR, tabs(d.value), 1, host, host, None, 16) == ERR_ARG
    assert lin(FR, tabs(d.value), 0, host, host, d2, 16) == ERR_ARG                     # 1 <= ntables <= 8
    assert lin(FR, tabs(*([d.value] * 9)), 9, host, host, d2, 16) == ERR_ARG
    assert lin(FR, tabs(d.value, None), 2, host, host, d2, 16) == ERR_ARG               # a null table
    assert lin(FR, tabs(d.value), 1, host, None, d2, (1 << 64) // 32) == ERR_ARG        # bytes a size_t cannot count
    assert lin(FR, tabs(d.value, d2.value), 2, host, host, C.c_void_p((1 << 30) + 32), 16) == ERR_ARG    # partial overlap
    assert lin(FR, tabs(d.value, d2.value), 2, host, None, C.c_void_p((1 << 20) - 32 * 15), 16) == ERR_ARG
    if L.ark_hip_device_count() == 0:                # well-formed calls: loud refusal, no CPU fallback
        for fid in (1, 3, 5):
            assert tree(fid, d, 4, d2, host) == ERR_NO_DEVICE
            assert tree(fid, d, 4, d2, None) == ERR_NO_DEVICE
            assert tree(fid, d, 0, None, host) == ERR_NO_DEVICE
            assert tree(fid, d, 4, C.c_void_p((1 << 20) + 32 * 16), host) == ERR_NO_DEVICE     # adjacent, not overlapping
            assert tree(fid, d, 4, C.c_void_p((1 << 20) - 32 * 15), host) == ERR_NO_DEVICE
            assert lin(fid, tabs(d.value, d2.value), 2, host, host, d2, 16) == ERR_NO_DEVICE   # d_out is table 1
            assert lin(fid, tabs(d.value, d2.value), 2, host, None, d, 16) == ERR_NO_DEVICE    # d_out is table 0
            assert lin(fid, tabs(d.value), 1, host, None, C.c_void_p((1 << 20) + 32 * 16), 16) == ERR_NO_DEVICE


def _rand(rng, count):
    return [int.from_bytes(rng.bytes(40), "little") % P for _ in range(count)]


def test_the_tree_model():
    rng = np.random.default_rng(21)
    assert R.tree([9], P) == (9, [])
    assert R.tree([2, 3, 5, 7], P) == (210, [2 * 5, 3 * 7, 210])       # pairs over the top index bit
    for nv in range(1, 9):
        f = _rand(rng, 1 << nv)
        prod, flat = R.tree(f, P)
        want = 1
        for v in f:
            want = want * v % P
        assert prod == want and flat[-1] == prod and len(flat) == (1 << nv) - 1
        lv = R.levels(f, P)
        for j in range(1, nv + 1):
            seg = flat[R.level_offset(nv, j):R.level_offset(nv, j) + R.level_len(nv, j)]
            assert seg == lv[j]
            # L_k(r) = sum_x eq(r, x) L_{k+1}(x, 0) L_{k+1}(x, 1) at a random r
            k = nv - j
            r = _rand(rng, k)
            h = 1 << k
            assert mle_ref.evaluate(seg, r, P) == sum(mle_ref.eq(x, r, P) * lv[j - 1][x] * lv[j - 1][x + h] for x in range(h)) % P
        z = list(f)
        z[-1] = 0                                                      # a zero in the last cell reaches every level's last cell
        assert all(level[-1] == 0 for level in R.levels(z, P)[1:]) and R.tree(z, P)[0] == 0
    assert R.lincomb([[1, 2], [3, 4]], [10, 100], 7, P) == [317, 427]


def _tamper(layers, k, what):
    out = [(None if sc is None else ([list(g) for g in sc[0]], list(sc[1])), tuple(pair)) for sc, pair in layers]
    sc, pair = out[k]
    if what == "round":
        sc[0][len(sc[0]) // 2][1] = (sc[0][len(sc[0]) // 2][1] + 1) % P
    else:
        out[k] = (sc, (pair[0], (pair[1] + 1) % P))
    return out


def test_the_verifier_accepts_the_model_and_rejects_altered_proofs():
    rng = np.random.default_rng(22)
    _, ch = R.hash_challenge(P)
    for nv in range(0, 7):
        f = _rand(rng, 1 << nv)
        product, layers, point = R.prove(f, ch, P)
        assert product == R.tree(f, P)[0] and len(layers) == nv and len(point) == nv
        ok, vpoint, claim = R.verify(nv, product, layers, ch, P)
        assert ok and vpoint == point and claim == mle_ref.evaluate(f, point, P), nv
        if nv == 0:
            continue
        # an altered product is caught at the first layer; an altered round or pair by that layer's sumcheck, or it moves
        # the last claim away from f(point)
        assert not R.verify(nv, (product + 1) % P, layers, ch, P)[0]
        assert not R.verify(nv, product, layers[:-1], ch, P)[0]
        for k in range(nv):
            ok, vpoint, claim = R.verify(nv, product, _tamper(layers, k, "pair"), ch, P)
            assert not ok or claim != mle_ref.evaluate(f, vpoint, P), (nv, k, "pair")
            if k:
                ok, vpoint, claim = R.verify(nv, product, _tamper(layers, k, "round"), ch, P)
                assert not ok, (nv, k, "round")
        assert not R.verify(nv, product, _tamper(layers, 0, "pair"), ch, P)[0]
