"""CPU-side checks of the fractional-sum entries (no GPU needed): the three entries are public C ABI with the same arity in the
header, `_lib.SYMBOLS`, ark-hip-sys, and are called by ark_hip.hpp and the Rust mirror; the plan answers for every
num_vars < 64 without a device and its launches tile each tree exactly once; argument errors come before any device is
touched; and the big-integer model of tests/fraction_sum_ref.py proves to its own verifier and that verifier rejects altered
proofs.  The kernels are checked on the GPU by tests/test_gpu_fraction_sum.py."""
import ctypes as C
import os
import re

import numpy as np

from algebra_amd import _lib
import algebra_amd as A
import fraction_sum_ref as R
import mle_ref
import pyref
from test_grand_product_host import _decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ark_hip_mle_fraction_tree_device": 7, "ark_hip_mle_fraction_tree_plan": 5, "ark_hip_fr_count_indices_device": 5}
ERR_ARG, ERR_NO_DEVICE = -1, -5
P = pyref.MODULI["BLS12_381_FR"][0]


def _levels():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    return int(re.search(r"#define ARK_HIP_FRACTION_TREE_LEVELS (\d+)", hdr).group(1))


LEVELS = _levels()


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
    at = hdr.index("int ark_hip_mle_fraction_tree_device")
    assert "must not overlap" in hdr[at - 2600:at]
    at = hdr.index("int ark_hip_fr_count_indices_device")
    doc = " ".join(hdr[at - 1200:at].split())
    assert "SKIPPED and not reported" in doc and "exactly when none was skipped" in doc
    assert 1 <= LEVELS <= 3 and A.mle.FRACTION_TREE_LEVELS == LEVELS


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
    for method in ("fraction_tree", "count_indices"):
        assert re.search(r"\bfn %s\b" % method, rust), method
        assert re.search(r"\b%s\(" % method, hpp[hpp.index("class DenseMultilinearExtension"):]), method
    fs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "fraction_sum.rs")).read()
    lib_rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "lib.rs")).read()
    assert re.search(r"\bfn prove\b", fs) and "struct FractionalSumProof" in fs and "struct FractionalSum<" in fs
    assert "pub mod fraction_sum;" in lib_rs and "FractionalSum" in lib_rs[lib_rs.index("pub use"):]
    assert "class FractionalSum" in hpp and "struct FractionalSumProof" in hpp
    # the ask for lambda has a name in every mirror
    assert re.search(r"LAMBDA_ROUND\s*=\s*-2", hpp) and re.search(r"LAMBDA_ROUND: i32 = -2", fs)
    assert A.fraction_sum.LAMBDA == "lambda" == R.LAMBDA
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "`%s`" % name in integ, name


def _plan(num_vars, has_num):
    ps = C.c_int()
    widths, groups = (C.c_int * 8)(*([-7] * 8)), (C.c_int * 8)(*([-7] * 8))
    assert _lib.lib().ark_hip_mle_fraction_tree_plan(num_vars, has_num, C.byref(ps), widths, groups) == 0, num_vars
    return ps.value, list(widths), list(groups)


def test_the_plan_answers_for_every_size_without_a_device():
    L = _lib.lib()
    for has_num in (1, 0):
        last_launches = 0
        for nv in range(64):
            ps, widths, groups = _plan(nv, has_num)
            assert 0 <= ps <= 2 and (ps > 0) == (nv > 0), (nv, ps)
            assert sum(widths[:ps]) == nv and all(w >= 1 for w in widths[:ps]), (nv, widths)
            assert widths[ps:] == [0] * (8 - ps) and groups == [0] * 8
            # a run is whole launches of LEVELS levels, or it is the one remainder launch, which comes last
            assert all(w % LEVELS == 0 for w in widths[:max(ps - 1, 0)]), (nv, widths)
            assert ps == 0 or widths[ps - 1] % LEVELS == 0 or widths[ps - 1] < LEVELS
            la = A.mle_fraction_tree_launches(nv, bool(has_num))
            assert sum(w for w, _ in la) == nv == sum(A.mle_fraction_tree_plan(nv, bool(has_num))[0])
            assert len(la) == -(-nv // LEVELS), (nv, la)              # the fewest launches of <= LEVELS levels
            assert [reads for _, reads in la] == [bool(has_num)] + [True] * (len(la) - 1) or not la
            assert len(la) >= last_launches
            last_launches = len(la)
            # the offsets the launches imply tile the 2^nv - 1 elements of a tree exactly once, in order
            at, m = 0, nv
            for w, _ in la:
                for a in range(w):
                    j = nv - (m - 1 - a)                              # the level that holds level m-1-a
                    assert R.level_offset(nv, j) == at and R.level_len(nv, j) == 1 << (m - 1 - a)
                    at += R.level_len(nv, j)
                m -= w
            assert m == 0 and at == (1 << nv) - 1
    ps, widths, groups = C.c_int(), (C.c_int * 8)(), (C.c_int * 8)()
    f = L.ark_hip_mle_fraction_tree_plan
    assert f(64, 1, C.byref(ps), widths, groups) == ERR_ARG
    assert f(5, 1, None, widths, groups) == ERR_ARG
    assert f(5, 0, C.byref(ps), None, groups) == ERR_ARG
    assert f(5, 1, C.byref(ps), widths, None) == ERR_ARG


def test_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    FR = 3                                           # BLS12_381_FR
    B = 1 << 20                                      # non-null "device pointers" that are never dereferenced
    p = C.c_void_p
    num, den, nt, dt = p(B), p(2 * B), p(3 * B), p(4 * B)
    el = (C.c_uint64 * 8)()
    host = C.cast(el, C.c_void_p)
    tree, cnt = L.ark_hip_mle_fraction_tree_device, L.ark_hip_fr_count_indices_device
    for field in (99, -1, 0, 2, 4):                  # unknown ids and the base fields
        assert tree(field, num, den, 4, nt, dt, host) == ERR_ARG
        assert cnt(field, num, 16, den, 16) == ERR_ARG
    for nm in (num, None):
        assert tree(FR, nm, None, 4, nt, dt, host) == ERR_ARG
        assert tree(FR, nm, None, 0, None, None, host) == ERR_ARG
        assert tree(FR, nm, den, 4, None, dt, host) == ERR_ARG       # both trees are needed once there are variables
        assert tree(FR, nm, den, 4, nt, None, None) == ERR_ARG
        assert tree(FR, nm, den, 64, nt, dt, host) == ERR_ARG        # num_vars >= 64
        assert tree(FR, nm, den, 63, nt, dt, host) == ERR_ARG
        assert tree(FR, nm, den, 59, nt, dt, None) == ERR_ARG        # more than 2^58 elements
        assert tree(FR, nm, den, 4, nt, nt, host) == ERR_ARG         # the two trees overlap
        assert tree(FR, nm, den, 4, nt, p(3 * B + 32 * 14), None) == ERR_ARG     # ... in one element
        assert tree(FR, nm, den, 4, nt, p(3 * B - 32 * 14), host) == ERR_ARG
        assert tree(FR, nm, den, 4, den, dt, host) == ERR_ARG        # a tree on the denominators
        assert tree(FR, nm, den, 4, nt, p(2 * B + 32 * 15), host) == ERR_ARG     # ... on their last element
        assert tree(FR, nm, den, 4, p(2 * B - 32 * 14), dt, None) == ERR_ARG     # a tree's last element on their first
    assert tree(FR, num, den, 4, num, dt, host) == ERR_ARG           # a tree on the numerators
    assert tree(FR, num, den, 4, nt, p(B + 32 * 15), host) == ERR_ARG
    assert tree(FR, num, den, 4, p(B - 32 * 14), dt, None) == ERR_ARG
    # counts
    assert cnt(FR, None, 16, den, 16) == ERR_ARG
    assert cnt(FR, num, 16, None, 16) == ERR_ARG
    assert cnt(FR, None, 0, None, 16) == ERR_ARG
    assert cnt(FR, num, 16, den, 0) == ERR_ARG
    assert cnt(FR, num, 1 << 32, p(1 << 50), 16) == ERR_ARG          # n >= 2^32
    assert cnt(FR, num, 16, den, (1 << 58) + 1) == ERR_ARG
    assert cnt(FR, num, 16, p(B + 4 * 15), 16) == ERR_ARG            # the output on the last index
    assert cnt(FR, num, 16, p(B - 32 * 16 + 1), 16) == ERR_ARG       # the output's last byte on the first index
    assert cnt(FR, p(2 * B + 32 * 999), 16, den, 1000) == ERR_ARG
    if L.ark_hip_device_count() == 0:                # well-formed calls: loud refusal, no CPU fallback
        for fid in (1, 3, 5):
            for nm in (num, None):
                assert tree(fid, nm, den, 4, nt, dt, host) == ERR_NO_DEVICE
                assert tree(fid, nm, den, 4, nt, dt, None) == ERR_NO_DEVICE
                assert tree(fid, nm, den, 0, None, None, host) == ERR_NO_DEVICE
                assert tree(fid, nm, den, 4, nt, p(3 * B + 32 * 15), host) == ERR_NO_DEVICE      # adjacent, not overlapping
                assert tree(fid, nm, den, 4, p(2 * B + 32 * 16), p(2 * B - 32 * 15), host) == ERR_NO_DEVICE
            assert tree(fid, None, den, 4, num, dt, host) == ERR_NO_DEVICE
            assert cnt(fid, num, 16, den, 16) == ERR_NO_DEVICE
            assert cnt(fid, None, 0, den, 1000) == ERR_NO_DEVICE      # no indices: d_indices may be null
            assert cnt(fid, num, 16, p(B + 4 * 16), 16) == ERR_NO_DEVICE
            assert cnt(fid, num, (1 << 32) - 1, p(1 << 50), 1 << 58) == ERR_NO_DEVICE


def _rand(rng, count):
    return [int.from_bytes(rng.bytes(40), "little") % P for _ in range(count)]


def test_the_tree_and_count_models():
    rng = np.random.default_rng(31)
    assert R.tree([5], [9], P) == ((5, 9), [], [])
    assert R.tree(None, [9], P) == ((1, 9), [], [])
    # 1/2 + 1/3 + 1/5 + 1/7 pairs over the top index bit: (2, 5) and (3, 7)
    assert R.tree(None, [2, 3, 5, 7], P) == ((7 * 21 + 10 * 10, 210), [7, 10, 7 * 21 + 10 * 10], [10, 21, 210])
    for nv in range(1, 9):
        for has_num in (True, False):
            den = _rand(rng, 1 << nv)
            num = _rand(rng, 1 << nv) if has_num else None
            (pp, qq), nflat, dflat = R.tree(num, den, P)
            want = sum((1 if num is None else num[b]) * pow(den[b], -1, P) for b in range(1 << nv)) % P
            assert pp * pow(qq, -1, P) % P == want and (nflat[-1], dflat[-1]) == (pp, qq)
            assert len(nflat) == len(dflat) == (1 << nv) - 1
            assert dflat == R.GP.tree(den, P)[1]
            ns, ds = R.levels(num, den, P)
            for j in range(1, nv + 1):
                k, h = nv - j, 1 << (nv - j)
                seg = nflat[R.level_offset(nv, j):R.level_offset(nv, j) + R.level_len(nv, j)]
                assert seg == ns[j]
                r = _rand(rng, k)
                assert mle_ref.evaluate(seg, r, P) == sum(
                    mle_ref.eq(x, r, P) * (ns[j - 1][x] * ds[j - 1][x + h] + ns[j - 1][x + h] * ds[j - 1][x]) for x in range(h)) % P
        z = _rand(rng, 1 << nv)
        z[-1] = 0                                                      # a zero denominator is just a value
        (pp, qq), _, _ = R.tree(None, z, P)
        prod = 1
        for v in z[:-1]:
            prod = prod * v % P
        assert qq == 0 and pp == prod
    assert R.counts([0, 3, 3, 7, 9, 3], 8) == [1, 0, 0, 3, 0, 0, 0, 1]
    assert R.counts([], 3) == [0, 0, 0] and R.counts([5, 5], 5) == [0] * 5


def _tamper(layers, k, what):
    out = [(None if sc is None else ([list(g) for g in sc[0]], list(sc[1])), tuple(v)) for sc, v in layers]
    sc, v = out[k]
    if what == "round":
        sc[0][len(sc[0]) // 2][1] = (sc[0][len(sc[0]) // 2][1] + 1) % P
    else:
        out[k] = (sc, v[:-1] + ((v[-1] + 1) % P,))
    return out


def test_the_verifier_accepts_the_model_and_rejects_altered_proofs():
    rng = np.random.default_rng(32)
    _, ch = R.hash_challenge(P)

    def swapped(layer, rnd, values):                                   # another lambda than the prover batched with
        return (ch(layer, rnd, values) + 1) % P if rnd == R.LAMBDA else ch(layer, rnd, values)
    for nv in range(0, 7):
        for has_num in (True, False):
            den = _rand(rng, 1 << nv)
            num = _rand(rng, 1 << nv) if has_num else None
            root, layers, point = R.prove(num, den, ch, P)
            assert root == R.tree(num, den, P)[0] and len(layers) == nv and len(point) == nv
            ok, vpoint, cn, cd = R.verify(nv, has_num, root, layers, ch, P)
            assert ok and vpoint == point, (nv, has_num)
            assert cd == mle_ref.evaluate(den, point, P) and cn == (mle_ref.evaluate(num, point, P) if has_num else 1)
            if nv == 0:
                continue

            def caught(result):                                        # rejected, or the last claims no longer hold
                ok, vpoint, cn, cd = result
                return not ok or cd != mle_ref.evaluate(den, vpoint, P) or cn != (mle_ref.evaluate(num, vpoint, P) if has_num else 1)
            assert not R.verify(nv, has_num, ((root[0] + 1) % P, root[1]), layers, ch, P)[0]
            assert not R.verify(nv, has_num, (root[0], (root[1] + 1) % P), layers, ch, P)[0]
            assert not R.verify(nv, has_num, root, layers[:-1], ch, P)[0]
            assert not R.verify(nv, not has_num, root, layers, ch, P)[0]      # the last layer's values have the other shape
            for k in range(nv):
                assert caught(R.verify(nv, has_num, root, _tamper(layers, k, "value"), ch, P)), (nv, k, "value")
                if k:
                    assert not R.verify(nv, has_num, root, _tamper(layers, k, "round"), ch, P)[0], (nv, k, "round")
            assert not R.verify(nv, has_num, root, _tamper(layers, 0, "value"), ch, P)[0]
            if nv > 1:
                assert not R.verify(nv, has_num, root, layers, swapped, P)[0], (nv, "lambda")


def test_the_lookup_seeds_on_the_model():
    """on the CPU model first: with these seeds the honest lookup balances and the altered one does not"""
    p = P
    t, idx, gamma, outside = R.lookup_case(p)
    assert outside not in t and all((gamma + v) % p for v in t + [outside])
    m = R.counts([int(i) for i in idx], 64)
    assert sum(m) == 512
    w = [t[i] for i in idx]
    (pw, qw), _, _ = R.tree(None, [(gamma + v) % p for v in w], p)
    (pt, qt), _, _ = R.tree(m, [(gamma + v) % p for v in t], p)
    assert pw * qt % p == pt * qw % p and qw and qt
    w[77] = outside
    (pw, qw), _, _ = R.tree(None, [(gamma + v) % p for v in w], p)
    assert pw * qt % p != pt * qw % p
