"""Host-side checks of the extension fields and of FRI over the one-word fields (no GPU): the model of
tests/fri_ref.py against itself, and the host entries of the library (ark_hip_xfp_info / _mul / _inverse / _pow,
ark_hip_fri_fold_row / _folded_domain / _plan and every argument error) against the model."""
import ctypes as C
import os
import re

import pytest

import algebra_amd as A
from algebra_amd import _lib, fri
import fri_ref as X
import smallfp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = list(X.FIELDS)
ERR_ARG, ERR_SIZE, ERR_NO_DEVICE = -1, -2, -5
NAMES = {"ark_hip_xfp_" + s for s in ("info", "mul", "inverse", "pow", "vec_mul", "vec_inverse", "vec_mul_const", "vec_mul_base",
                                      "combine_columns")} | \
        {"ark_hip_fri_" + s for s in ("fold_row", "folded_domain", "plan", "fold", "commit_phase")}


def edge_elements(x):
    vals = (0, 1, x.p - 1)
    if x.d == 2:
        return [(a, b) for a in vals for b in vals]
    return [(a, b, c, e) for a in vals for b in vals for c in vals for e in vals]


def dom_struct(f, k, h_stored=None):
    d = A.SmallRadix2EvaluationDomain.new(f.name, 1 << k)
    return d if h_stored is None else d.get_coset(h_stored)


# ---- the model against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIELDS)
def test_model_w_is_a_non_residue_and_the_tower_is_a_field(name):
    x = X.FIELDS[name]
    assert x.w_is_irreducible()
    assert (x.d, x.w) == {"GOLDILOCKS": (2, 7), "BABYBEAR": (4, 11), "KOALABEAR": (4, 3)}[name]
    assert pow(x.w, (x.p - 1) // 2, x.p) == x.p - 1 and x.p % 4 == 1
    # the upper level's non-residue is u = (0, 1): v^2 = u
    if x.d == 4:
        v = (0, 0, 1, 0)
        assert x.mul(v, v) == (0, 1, 0, 0) and x.mul((0, 1, 0, 0), (0, 1, 0, 0)) == (x.w, 0, 0, 0)
        assert x.expo == (0, 2, 1, 3)
    else:
        assert x.mul((0, 1), (0, 1)) == (x.w, 0)


@pytest.mark.parametrize("name", FIELDS)
def test_model_tower_product_is_the_schoolbook_product_modulo_x_d_minus_w(name):
    x = X.FIELDS[name]
    rng = X.rng(30)
    edges = edge_elements(x)
    pairs = [(a, b) for a in edges[:9] for b in edges] + [(x.random_element(rng), x.random_element(rng)) for _ in range(3000)]
    pairs += [(a, x.random_element(rng)) for a in edges]
    for a, b in pairs:
        assert x.mul(a, b) == x.mul_poly(a, b), (a, b)
    for a in edges:   # the basis map (a0, a1, b0, b1) <-> (x0, x2, x1, x3) is its own inverse on the tuple
        assert x.from_poly(x.to_poly(a)) == a


@pytest.mark.parametrize("name", FIELDS)
def test_model_inverse(name):
    x = X.FIELDS[name]
    rng = X.rng(31)
    for a in edge_elements(x) + [x.random_element(rng) for _ in range(10000)]:
        if a == x.zero():
            assert x.inv(a) == x.zero()
        else:
            assert x.mul(a, x.inv(a)) == x.one(), a


@pytest.mark.parametrize("name", FIELDS)
def test_model_fold_definitions_agree(name):
    x = X.FIELDS[name]
    rng = X.rng(32)
    for k in range(1, 7):
        for a in (1, 2, 3):
            if a > k:
                continue
            for h in (1, x.gen):
                f = [x.random_element(rng) for _ in range(1 << k)]
                beta = x.random_element(rng)
                by_eval = x.fold_eval(f, k, h, a, beta)
                assert by_eval == x.fold_coeff(f, k, h, a, beta), (k, a, h)
                # arity 2^a is a 2-folds with beta^(2^j): spelled out once more, step by step
                g, kk, hh, bb = f, k, h, beta
                for _ in range(a):
                    g, kk, hh, bb = x.fold2(g, kk, hh, bb), kk - 1, hh * hh % x.p, x.mul(bb, bb)
                assert g == by_eval
                # and a row folded on its own is the fold's value at that row
                m = 1 << (k - a)
                for i in {0, m - 1, rng.randrange(m)}:
                    row = [f[i + j * m] for j in range(1 << a)]
                    assert x._fold_small(row, a, h * pow(x.omega(k), i, x.p) % x.p, beta) == by_eval[i]


# ---- the C ABI against the model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIELDS)
def test_info_mul_inverse_pow(name):
    x = X.FIELDS[name]
    info = A.small_ext_info(name)
    assert info == dict(degree=x.d, w=x.w, w_stored=x.st(x.w), exponents=list(x.expo))
    rng = X.rng(33)
    edges = edge_elements(x)   # as STORED words: 0, 1, p - 1 in every component
    pairs = [(a, b) for a in edges[:9] for b in edges] + [(x.random_element(rng), x.random_element(rng)) for _ in range(2000)]
    for a, b in pairs:
        assert A.ext_mul(name, a, b) == x.stored(x.mul(x.plain(a), x.plain(b))), (a, b)
    for a in edges + [x.random_element(rng) for _ in range(500)]:
        assert A.ext_inverse(name, a) == x.stored(x.inv(x.plain(a))), a
        for e in (0, 1, 2, 5, x.p, (1 << 64) - 1):
            assert A.ext_pow(name, a, e) == x.stored(x.pow(x.plain(a), e)), (a, e)


@pytest.mark.parametrize("name", FIELDS)
def test_fold_row_and_folded_domain(name):
    x, f = X.FIELDS[name], R.FIELDS[name]
    rng = X.rng(34)
    for k in range(1, 8):
        for a in (1, 2, 3):
            if a > k:
                continue
            for h in (1, x.gen, rng.randrange(1, x.p)):
                dom = dom_struct(f, k, x.st(h))
                layer = [x.random_element(rng) for _ in range(1 << k)]
                betas = [x.zero(), x.one(), x.base(rng.randrange(x.p)), x.random_element(rng)]
                beta = betas[(k + a) % 4]
                want = x.fold_eval(layer, k, h, a, beta)
                m = 1 << (k - a)
                for i in sorted({0, m - 1, rng.randrange(m)}):
                    row = [x.st(layer[i + j * m][c]) for c in range(x.d) for j in range(1 << a)]
                    assert A.fri_fold_row(dom, a, i, row, x.stored(beta)) == x.stored(want[i]), (k, a, h, i)
                fd = A.fri_folded_domain(dom, a)
                ref = f.get_coset(f.domain_new(1 << (k - a)), x.st(pow(h, 1 << a, x.p)))
                assert {key: getattr(fd._s, key) for key in R.DOMAIN_KEYS} == ref, (k, a, h)


@pytest.mark.parametrize("name", FIELDS)
def test_plan_closed_forms(name):
    x, f = X.FIELDS[name], R.FIELDS[name]
    for log_n in range(f.two_adicity + 1):
        for a in (1, 2, 3):
            for num_folds in sorted({0, 1, log_n // a, -(-log_n // a)}):
                if num_folds and (num_folds - 1) * a >= log_n:
                    continue
                pl = A.fri_plan(name, log_n, a, num_folds)
                ar = x.layer_arities(log_n, a, num_folds)
                logs = [log_n - sum(ar[:l]) for l in range(num_folds + 1)]
                assert pl["degree"] == x.d and len(pl["layers"]) == num_folds + 1 and pl["launches_per_fold"] == 1
                assert [l["log_size"] for l in pl["layers"]] == logs
                assert [l["log_arity"] for l in pl["layers"]] == ar + [0]
                assert [l["lo_bits"] for l in pl["layers"]] == [(k + 1) // 2 for k in logs[:-1]] + [0]
                off, toff = 0, 0
                for l, lay in enumerate(pl["layers"]):
                    if l:
                        assert lay["layer_offset"] == off
                        off += x.d << logs[l]
                    if l < num_folds:
                        assert lay["tree_offset"] == toff
                        toff += (2 * (1 << (logs[l] - ar[l])) - 1) * 32
                assert pl["final_copy_offset"] == off and pl["final_size"] == 1 << logs[-1]
                assert pl["layer_words"] == off + (x.d << logs[-1]) and pl["tree_bytes"] == toff
                assert all(lay["layer_offset"] * f.bytes % 16 == 0 and lay["tree_offset"] % 32 == 0 for lay in pl["layers"])


@pytest.mark.parametrize("name", FIELDS)
def test_verifier_accepts_the_models_commit_phase_and_rejects_tampering(name):
    """fri_verify_query needs no GPU: openings built from the model's layers and trees"""
    import numpy as np
    import merkle_ref as MR
    x, f = X.FIELDS[name], R.FIELDS[name]
    rng = X.rng(35)
    for k, a, num_folds in ((6, 1, 4), (7, 2, 3), (7, 3, 3)):
        layer = [x.random_element(rng) for _ in range(1 << k)]
        cols = [[e[c] for e in layer] for c in range(x.d)]
        cp = x.commit_phase(cols, k, x.gen, a, num_folds, X.shake_challenge(x, []))
        dom = dom_struct(f, k, x.st(x.gen))
        final = np.array(cp["final"], dtype=np.uint64)
        for index in (0, (1 << k) - 1, rng.randrange(1 << k)):
            openings, pos, kk = [], index, k
            for l, al in enumerate(cp["arities"]):
                m = 1 << (kk - al)
                r = pos % m
                view = x.row_view(cp["layers"][l], al)
                row = np.array([c[r] for c in view], dtype=np.uint64)
                path = np.frombuffer(b"".join(MR.path(cp["trees"][l], r)), dtype=np.uint8).reshape(-1, 32)
                openings.append((row, path))
                pos, kk = r, kk - al
            args = (dom, a, num_folds, cp["roots"], cp["betas"])
            assert A.fri_verify_query(*args, final, index, openings), (name, k, a, index)
            assert x.verify_query(k, x.gen, a, num_folds, cp["roots"], cp["betas"], cp["final"], index,
                                  [(r_.tolist(), [bytes(p_) for p_ in pa]) for r_, pa in openings])
            for l in range(num_folds):
                row, path = openings[l]
                bad = row.copy()
                bad[l % bad.size] ^= 1
                assert not A.fri_verify_query(*args, final, index, openings[:l] + [(bad, path)] + openings[l + 1:])
            bad_final = final.copy()
            bad_final[0, 0] ^= 1
            assert not A.fri_verify_query(*args, bad_final, index, openings)
            assert not A.fri_verify_query(dom, a, num_folds, cp["roots"], cp["betas"][::-1], final, index, openings)


def test_argument_errors_come_before_any_device():
    L = _lib.lib()
    out4, out8, plan = (C.c_uint64 * 4)(), (C.c_uint64 * 8)(), (C.c_uint64 * 64)()
    fake, fake2, fake3 = C.c_void_p(0x100000), C.c_void_p(0x800000), C.c_void_p(0xC00000)
    one = (C.c_uint64 * 4)(1, 0, 0, 0)
    row = (C.c_uint64 * 32)()
    roots = (C.c_uint8 * 1024)()
    cb = _lib.FriNextBeta(lambda u, r, b: 0)
    cbp = C.cast(cb, C.c_void_p)
    dom = _lib.SmallRadix2DomainStruct()
    for bad in (-1, 3, 5, 99):
        assert L.ark_hip_xfp_info(bad, out8) == ERR_ARG
        assert L.ark_hip_xfp_mul(bad, one, one, out4) == ERR_ARG
        assert L.ark_hip_xfp_inverse(bad, one, out4) == ERR_ARG
        assert L.ark_hip_xfp_pow(bad, one, 1, out4) == ERR_ARG
        assert L.ark_hip_fri_plan(bad, 4, 1, 1, plan) == ERR_ARG
        assert L.ark_hip_xfp_vec_mul(bad, fake, 4, fake, 4, fake, 4, 4) == ERR_ARG
        assert L.ark_hip_xfp_vec_inverse(bad, fake, 4, fake, 4, 4) == ERR_ARG
        assert L.ark_hip_xfp_vec_mul_const(bad, fake, 4, one, fake, 4, 4) == ERR_ARG
        assert L.ark_hip_xfp_vec_mul_base(bad, fake, 4, fake, fake, 4, 4) == ERR_ARG
        assert L.ark_hip_xfp_combine_columns(bad, fake, 1, 4, 4, one, 0, fake2, 4, 0) == ERR_ARG
    for name in FIELDS:
        x, f = X.FIELDS[name], R.FIELDS[name]
        sid = f.sid
        assert L.ark_hip_sfp_radix2_domain_new(sid, 16, C.byref(dom)) == 0
        D = C.byref(dom)
        big = (C.c_uint64 * 4)(x.p, 0, 0, 0)
        hi = (C.c_uint64 * 4)(1, 0, 1, 0) if x.d == 2 else (C.c_uint64 * 4)(1, 0, 0, x.p)
        assert L.ark_hip_xfp_info(sid, None) == ERR_ARG
        for k in (big, hi, None):   # a component >= p, a non-zero word behind the degree, a null element
            assert L.ark_hip_xfp_mul(sid, k, one, out4) == L.ark_hip_xfp_mul(sid, one, k, out4) == ERR_ARG
            assert L.ark_hip_xfp_inverse(sid, k, out4) == L.ark_hip_xfp_pow(sid, k, 3, out4) == ERR_ARG
            assert L.ark_hip_xfp_vec_mul_const(sid, fake, 4, k, fake, 4, 4) == ERR_ARG
            assert L.ark_hip_xfp_combine_columns(sid, fake, 1, 4, 4, k, 0, fake2, 4, 0) == ERR_ARG
            assert L.ark_hip_fri_fold_row(sid, D, 1, 0, row, k, out4) == ERR_ARG
            assert L.ark_hip_fri_fold(sid, D, 1, k, fake, 16, fake2, 8) == ERR_ARG
        assert L.ark_hip_xfp_mul(sid, one, one, None) == L.ark_hip_xfp_inverse(sid, one, None) == L.ark_hip_xfp_pow(sid, one, 1, None) == ERR_ARG
        # pointwise: null pointers with n > 0, stride < n
        assert L.ark_hip_xfp_vec_mul(sid, None, 4, fake, 4, fake, 4, 4) == L.ark_hip_xfp_vec_mul(sid, fake, 4, None, 4, fake, 4, 4) == ERR_ARG
        assert L.ark_hip_xfp_vec_mul(sid, fake, 4, fake, 4, None, 4, 4) == ERR_ARG
        assert L.ark_hip_xfp_vec_mul(sid, fake, 3, fake, 4, fake, 4, 4) == L.ark_hip_xfp_vec_mul(sid, fake, 4, fake, 3, fake, 4, 4) == ERR_ARG
        assert L.ark_hip_xfp_vec_mul(sid, fake, 4, fake, 4, fake, 3, 4) == ERR_ARG
        assert L.ark_hip_xfp_vec_inverse(sid, None, 4, fake, 4, 4) == L.ark_hip_xfp_vec_inverse(sid, fake, 4, None, 4, 4) == ERR_ARG
        assert L.ark_hip_xfp_vec_inverse(sid, fake, 3, fake, 4, 4) == L.ark_hip_xfp_vec_inverse(sid, fake, 4, fake, 3, 4) == ERR_ARG
        assert L.ark_hip_xfp_vec_mul_const(sid, None, 4, one, fake, 4, 4) == L.ark_hip_xfp_vec_mul_const(sid, fake, 4, one, None, 4, 4) == ERR_ARG
        assert L.ark_hip_xfp_vec_mul_base(sid, fake, 4, None, fake, 4, 4) == L.ark_hip_xfp_vec_mul_base(sid, fake, 3, fake, fake, 4, 4) == ERR_ARG
        # combine: null pointers, no column, stride < rows, out inside the matrix
        cc = L.ark_hip_xfp_combine_columns
        assert cc(sid, None, 1, 4, 4, one, 0, fake2, 4, 0) == cc(sid, fake, 1, 4, 4, one, 0, None, 4, 0) == ERR_ARG
        assert cc(sid, fake, 0, 4, 4, one, 0, fake2, 4, 0) == cc(sid, fake, 1, 3, 4, one, 0, fake2, 4, 0) == ERR_ARG
        assert cc(sid, fake, 1, 4, 4, one, 0, fake2, 3, 0) == ERR_ARG
        assert cc(sid, fake, 3, 8, 8, one, 0, C.c_void_p(0x100000 + 16 * f.bytes), 8, 0) == ERR_ARG
        # fold_row / folded_domain / fold: the domain, the arity, the index
        broken = _lib.SmallRadix2DomainStruct.from_buffer_copy(dom)
        broken.size = 24
        toobig = _lib.SmallRadix2DomainStruct.from_buffer_copy(dom)
        toobig.group_gen_inv = x.p
        for bd in (None, C.byref(broken), C.byref(toobig)):
            assert L.ark_hip_fri_fold_row(sid, bd, 1, 0, row, one, out4) == ERR_ARG
            assert L.ark_hip_fri_folded_domain(sid, bd, 1, C.byref(_lib.SmallRadix2DomainStruct())) == ERR_ARG
            assert L.ark_hip_fri_fold(sid, bd, 1, one, fake, 16, fake2, 8) == ERR_ARG
            assert L.ark_hip_fri_commit_phase(sid, bd, 1, 1, fake, fake2, fake3, cbp, None, roots, roots) == ERR_ARG
        for a in (0, 4, 5):
            assert L.ark_hip_fri_fold_row(sid, D, a, 0, row, one, out4) == ERR_ARG
            assert L.ark_hip_fri_folded_domain(sid, D, a, C.byref(_lib.SmallRadix2DomainStruct())) == ERR_ARG
            assert L.ark_hip_fri_fold(sid, D, a, one, fake, 16, fake2, 8) == ERR_ARG
            assert L.ark_hip_fri_plan(sid, 4, a, 1, plan) == ERR_ARG
            assert L.ark_hip_fri_commit_phase(sid, D, a, 1, fake, fake2, fake3, cbp, None, roots, roots) == ERR_ARG
        assert L.ark_hip_fri_fold_row(sid, D, 1, 8, row, one, out4) == ERR_ARG, "an index >= n / 2^a"
        assert L.ark_hip_fri_fold_row(sid, D, 1, 0, None, one, out4) == L.ark_hip_fri_fold_row(sid, D, 1, 0, row, one, None) == ERR_ARG
        bad_row = (C.c_uint64 * 32)()
        bad_row[1] = x.p
        assert L.ark_hip_fri_fold_row(sid, D, 1, 0, bad_row, one, out4) == ERR_ARG
        assert L.ark_hip_fri_folded_domain(sid, D, 1, None) == ERR_ARG
        small = _lib.SmallRadix2DomainStruct()
        assert L.ark_hip_sfp_radix2_domain_new(sid, 2, C.byref(small)) == 0
        assert L.ark_hip_fri_folded_domain(sid, C.byref(small), 2, C.byref(_lib.SmallRadix2DomainStruct())) == ERR_ARG, "arity beyond the size"
        assert L.ark_hip_fri_fold(sid, D, 1, one, None, 16, fake2, 8) == L.ark_hip_fri_fold(sid, D, 1, one, fake, 16, None, 8) == ERR_ARG
        assert L.ark_hip_fri_fold(sid, D, 1, one, fake, 15, fake2, 8) == L.ark_hip_fri_fold(sid, D, 1, one, fake, 16, fake2, 7) == ERR_ARG
        ext_in = (x.d - 1) * 16 + 16   # words of the input's extent at stride 16
        for o in (0x100000, 0x100000 + (ext_in - 1) * f.bytes, 0x100000 - ((x.d - 1) * 8 + 8 - 1) * f.bytes):
            assert L.ark_hip_fri_fold(sid, D, 1, one, fake, 16, C.c_void_p(o), 8) == ERR_ARG, ("in and out overlap", hex(o))
        # plan: num_folds * a beyond log n, except a short last fold
        assert L.ark_hip_fri_plan(sid, 4, 1, 1, None) == ERR_ARG
        assert L.ark_hip_fri_plan(sid, 4, 2, 3, plan) == ERR_ARG and L.ark_hip_fri_plan(sid, 4, 1, 5, plan) == ERR_ARG
        assert L.ark_hip_fri_plan(sid, 4, 3, 2, plan) == 0 and L.ark_hip_fri_plan(sid, 4, 3, 3, plan) == ERR_ARG
        assert L.ark_hip_fri_plan(sid, f.two_adicity + 1, 1, 1, plan) == ERR_SIZE
        # commit phase: null pointers, too many folds, workspaces over layer 0 or over each other
        cp = L.ark_hip_fri_commit_phase
        assert cp(sid, D, 1, 2, None, fake2, fake3, cbp, None, roots, roots) == cp(sid, D, 1, 2, fake, None, fake3, cbp, None, roots, roots) == ERR_ARG
        assert cp(sid, D, 1, 2, fake, fake2, None, cbp, None, roots, roots) == cp(sid, D, 1, 2, fake, fake2, fake3, None, None, roots, roots) == ERR_ARG
        assert cp(sid, D, 1, 2, fake, fake2, fake3, cbp, None, None, roots) == cp(sid, D, 1, 2, fake, fake2, fake3, cbp, None, roots, None) == ERR_ARG
        assert cp(sid, D, 2, 3, fake, fake2, fake3, cbp, None, roots, roots) == cp(sid, D, 1, 5, fake, fake2, fake3, cbp, None, roots, roots) == ERR_ARG
        last0 = 0x100000 + (x.d * 16 - 1) * f.bytes & ~15
        assert cp(sid, D, 1, 2, fake, C.c_void_p(last0), fake3, cbp, None, roots, roots) == ERR_ARG, "layers over layer 0"
        assert cp(sid, D, 1, 2, fake, fake2, C.c_void_p(last0), cbp, None, roots, roots) == ERR_ARG, "trees over layer 0"
        assert cp(sid, D, 1, 2, fake, fake2, C.c_void_p(0x800000 + 16), cbp, None, roots, roots) == ERR_ARG, "trees over layers"
        assert cp(sid, D, 1, 2, fake, C.c_void_p(0x800008), fake3, cbp, None, roots, roots) == ERR_ARG, "a misaligned workspace"


def test_without_a_gpu_the_device_entries_say_so():
    L = _lib.lib()
    if L.ark_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    dom = _lib.SmallRadix2DomainStruct()
    assert L.ark_hip_sfp_radix2_domain_new(1, 16, C.byref(dom)) == 0
    fake, fake2, fake3 = C.c_void_p(0x100000), C.c_void_p(0x800000), C.c_void_p(0xC00000)
    one = (C.c_uint64 * 4)(1, 0, 0, 0)
    out = (C.c_uint8 * 1024)()
    cb = _lib.FriNextBeta(lambda u, r, b: 0)
    assert L.ark_hip_xfp_vec_mul(1, fake, 4, fake, 4, fake, 4, 4) == ERR_NO_DEVICE
    assert L.ark_hip_xfp_vec_inverse(1, fake, 4, fake, 4, 0) == ERR_NO_DEVICE
    assert L.ark_hip_xfp_vec_mul_const(1, fake, 4, one, fake, 4, 4) == ERR_NO_DEVICE
    assert L.ark_hip_xfp_vec_mul_base(1, fake, 4, fake2, fake, 4, 4) == ERR_NO_DEVICE
    assert L.ark_hip_xfp_combine_columns(1, fake, 2, 4, 4, one, 0, fake2, 4, 0) == ERR_NO_DEVICE
    assert L.ark_hip_fri_fold(1, C.byref(dom), 1, one, fake, 16, fake2, 8) == ERR_NO_DEVICE
    assert L.ark_hip_fri_commit_phase(1, C.byref(dom), 1, 2, fake, fake2, fake3, C.cast(cb, C.c_void_p), None, out, out) == ERR_NO_DEVICE


def test_header_bindings_and_mirrors_name_the_same_entries():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    pat = r"\b(ark_hip_(?:xfp|fri)_[a-z0-9_]+)\s*\("
    declared = set(re.findall(pat, hdr))
    assert declared == NAMES, declared ^ NAMES
    bound = {s for s in _lib.SYMBOLS if s.startswith(("ark_hip_xfp_", "ark_hip_fri_"))}
    assert bound == declared, bound ^ declared
    for name in declared:
        assert not name.startswith("ark_hip_sfp_") and not name.endswith("_device"), name
        arity = len(re.search(r"\b%s\s*\(([^;]*?)\);" % name, hdr, re.S).group(1).split(","))
        assert len(_lib.SYMBOLS[name][1]) == arity, name
        assert hasattr(_lib.lib(), name), name
    assert "ark_hip_*" in open(os.path.join(ROOT, "algebra_amd", "csrc", "exports.map")).read()
    py = open(os.path.join(ROOT, "algebra_amd", "fri.py")).read()
    cpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for mirror, text in (("fri.py", py), ("ark_hip.hpp", cpp)):
        used = set(re.findall(pat, text))
        assert used == declared, (mirror, used ^ declared)
        for cls in ("SmallExtVec", "FriProver"):
            assert ("class " + cls) in text, (mirror, cls)
    assert "def combine_columns" in py and "def fri_verify_query" in py
    assert fri.small_ext_degree("GOLDILOCKS") == 2 and fri.small_ext_degree("BABYBEAR") == fri.small_ext_degree("KOALABEAR") == 4
