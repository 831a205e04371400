"""The extension-field vectors, the combination of columns, the FRI fold and the commit phase on the GPU, limb for limb against
the model of tests/fri_ref.py.  Outputs go into 0xFF-filled buffers with guard regions and gaps; inputs are
checked unchanged."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd import _lib
import fri_ref as X
import merkle_ref as MR
import smallfp_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = list(X.FIELDS)
GUARD = 8
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000)
SEAMS = (0, 1, 2, 3, 4, 5, 7, 8, 62, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512)


def dtype(x):
    return np.uint64 if x.bytes == 8 else np.uint32


def elem4(e):
    a = (C.c_uint64 * 4)()
    for k, v in enumerate(e):
        a[k] = int(v)
    return a


def edge_at(x, i):
    """a stored element whose components run through 0, 1, p - 1 as i grows"""
    vals = (0, 1, x.p - 1)
    return tuple(vals[(i // 3 ** k) % 3] for k in range(x.d))


def ext_inputs(x, n, seed, zeros=False):
    """n stored elements: random, with the edge components planted at every chunk, wave and block seam (zeros=True: zero
    elements at and around the seams instead, and one whole chunk of them)"""
    rng = X.rng(seed)
    v = [x.random_element(rng) for _ in range(n)]
    for t, i in enumerate(SEAMS + (n - 2, n - 1)):
        if 0 <= i < n:
            v[i] = x.zero() if zeros and t % 3 != 1 else edge_at(x, 7 * t + 1 + i)
    if zeros:
        for i in range(16, min(20, n)):
            v[i] = x.zero()
    return v


class Arena:
    """one device allocation of 0xFF words; vectors are carved out of it with guards between them.  add(): d (or 1) columns of n
    words `stride` apart, the first on a 16-byte boundary plus `shift` words"""

    def __init__(self, x, words):
        self.x, self.dt = x, dtype(x)
        self.host = np.full(words, np.iinfo(self.dt).max, dtype=self.dt)
        self.next = GUARD + (-GUARD) % 4
        self.regions = {}

    def add(self, name, n, stride, cols, shift=0, data=None):
        at = self.next + shift
        self.regions[name] = (at, n, stride, cols)
        self.next = at + cols * max(stride, 1) + GUARD
        self.next += (-self.next) % 4
        assert self.next <= self.host.size
        if data is not None:      # data: n elements (tuples of `cols` words), or n words for cols = 1
            for k in range(cols):
                self.host[at + k * stride:at + k * stride + n] = [e[k] for e in data] if cols > 1 else list(data)
        return at

    def upload(self):
        self.vec = A.SmallDeviceVec.from_host(self.x.name, self.host)
        return self

    def ptr(self, name):
        return C.c_void_p(self.vec.ptr + self.regions[name][0] * self.x.bytes)

    def stride(self, name):
        return self.regions[name][2]

    def check_outside(self, written, what):
        """every word outside region `written`'s elements is as uploaded; returns the downloaded arena"""
        out = self.vec.to_host()
        at, n, stride, cols = self.regions[written]
        mask = np.ones(out.size, dtype=bool)
        for k in range(cols):
            mask[at + k * stride:at + k * stride + n] = False
        assert np.array_equal(out[mask], self.host[mask]), (what, "wrote outside its output, or changed an input")
        return out

    def check(self, written, want, what):
        """region `written` holds `want` (n elements); every other word of the arena is as uploaded"""
        out = self.check_outside(written, what)
        at, n, stride, cols = self.regions[written]
        got = [out[at + k * stride:at + k * stride + n].tolist() for k in range(cols)]
        got = [tuple(g[i] for g in got) for i in range(n)]
        bad = [i for i in range(n) if got[i] != tuple(want[i])]
        assert not bad, (what, "first differing elements", bad[:8])


def layouts(x, n):
    """(shift, stride): compact and aligned, compact off alignment, gaps of three words, gaps on 16-byte multiples"""
    wide = 16 // x.bytes
    return ((0, n), (1, n), (0, n + 3), (0, (n + wide - 1) // wide * wide + wide), (1, n + 3))


# ---- pointwise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["mul", "inverse", "mul_const", "mul_base"])
@pytest.mark.parametrize("name", FIELDS)
def test_pointwise(name, op):
    x = X.FIELDS[name]
    L = _lib.lib()
    rng = X.rng(40)
    consts = [x.zero(), x.one(), x.stored(x.base(5)), x.random_element(rng), edge_at(x, 2 + 3 + 9 + 27)]
    for n in LENGTHS:
        a = ext_inputs(x, n, 41 + n, zeros=op == "inverse")
        b = ext_inputs(x, n, 43 + n)
        bb = [e[0] for e in b]
        pa, pb = [x.plain(e) for e in a], [x.plain(e) for e in b]
        if op == "mul":
            wants = [[x.stored(x.mul(u, v)) for u, v in zip(pa, pb)]]
        elif op == "inverse":
            wants = [[x.stored(x.inv(u)) for u in pa]]
            assert all((w == x.zero()) == (u == x.zero()) for u, w in zip(a, wants[0]))
        elif op == "mul_const":
            wants = [[x.stored(x.mul(u, x.plain(k))) for u in pa] for k in consts]
        else:
            wants = [[x.stored(x.scale(u, x.pl(s))) for u, s in zip(pa, bb)]]
        for shift, stride in layouts(x, n):
            for dst in (("r", "a", "b") if op == "mul" else ("r", "a")):
                for ci, want in enumerate(wants):
                    ar = Arena(x, 3 * (x.d * max(stride, 1) + 2 * GUARD + 8) + 16)
                    ar.add("a", n, stride, x.d, shift, a)
                    if op == "mul_base":
                        ar.add("b", n, n, 1, shift, bb)
                    else:
                        ar.add("b", n, stride, x.d, shift, b)
                    ar.add("r", n, stride, x.d, shift)
                    ar.upload()
                    s = stride
                    if op == "mul":
                        rc = L.ark_hip_xfp_vec_mul(x.sid, ar.ptr("a"), s, ar.ptr("b"), s, ar.ptr(dst), s, n)
                    elif op == "inverse":
                        rc = L.ark_hip_xfp_vec_inverse(x.sid, ar.ptr("a"), s, ar.ptr(dst), s, n)
                    elif op == "mul_const":
                        rc = L.ark_hip_xfp_vec_mul_const(x.sid, ar.ptr("a"), s, elem4(consts[ci]), ar.ptr(dst), s, n)
                    else:
                        rc = L.ark_hip_xfp_vec_mul_base(x.sid, ar.ptr("a"), s, ar.ptr("b"), ar.ptr(dst), s, n)
                    assert rc == 0, (name, op, n, rc)
                    ar.check(dst, want, (name, op, n, shift, stride, dst, ci))   # dst = a or b: the output aliases that input


@pytest.mark.parametrize("name", FIELDS)
def test_ext_vec_mirror(name):
    x = X.FIELDS[name]
    rng = X.rng(44)
    n = 300
    a, b = [x.random_element(rng) for _ in range(n)], [x.random_element(rng) for _ in range(n)]
    a[7] = x.zero()
    va = A.SmallExtVec.from_host(name, np.array(x_cols(x, a), dtype=dtype(x)))
    vb = A.SmallExtVec.from_host(name, np.array(x_cols(x, b), dtype=dtype(x)), stride=n + 4)
    k = x.random_element(rng)
    base = [rng.randrange(x.p) for _ in range(n)]
    va *= vb
    va.mul_const(k).mul_base(A.SmallDeviceVec.from_host(name, np.array(base, dtype=dtype(x)))).batch_inverse()
    want = []
    for u, v, s in zip(a, b, base):
        t = x.scale(x.mul(x.mul(x.plain(u), x.plain(v)), x.plain(k)), x.pl(s))
        want.append(x.stored(x.inv(t)))
    assert cols_x(va.to_host()) == want
    assert cols_x(vb.to_host()) == b
    # the Merkle commit of the d columns hashes header | serialize_compressed(element)
    small = A.SmallExtVec.from_host(name, np.array(x_cols(x, b[:8]), dtype=dtype(x)))
    assert small.commit().root == MR.tree(name, x_cols(x, b[:8]))[0]


def x_cols(x, elems):
    return [[e[k] for e in elems] for k in range(x.d)]


def cols_x(arr):
    return [tuple(int(v) for v in arr[:, i]) for i in range(arr.shape[1])]


# ---- combine --------------------------------------------------------------------------------------------------------------------
def combine_model(x, plain_cols, rows, alpha, first_power, acc):
    """x.combine on object arrays (one big-integer product per column and component); plain_cols: [count, >= rows] plain
    residues, alpha and acc stored, stored out"""
    pa = x.plain(alpha)
    pws = [x.pow(pa, first_power)]
    for _ in range(plain_cols.shape[0] - 1):
        pws.append(x.mul(pws[-1], pa))
    m = plain_cols[:, :rows]
    out = []
    for k in range(x.d):
        w = np.array([pw[k] for pw in pws], dtype=object)
        out.append((w[:, None] * m).sum(axis=0) % x.p)
    res = [tuple(x.st(int(out[k][i])) for k in range(x.d)) for i in range(rows)]
    if acc is not None:
        res = [x.stored(x.add(x.plain(r), x.plain(a))) for r, a in zip(res, acc)]
    return res


@pytest.mark.parametrize("count", [1, 2, 3, 64, 65])
@pytest.mark.parametrize("name", FIELDS)
def test_combine_columns(name, count):
    x = X.FIELDS[name]
    L = _lib.lib()
    rng = X.rng(50 + count)
    big = 1 << 13
    cols = [[rng.randrange(x.p) for _ in range(big)] for _ in range(count)]
    for c in cols:
        c[0], c[1], c[2] = 0, x.p - 1, x.st(1)
    alpha = x.random_element(rng)
    old = [x.random_element(rng) for _ in range(big)]
    # the numpy model is the model of fri_ref.py
    pc = np.array([[x.pl(v) for v in c] for c in cols], dtype=object)
    ref = x.combine([[x.pl(v) for v in c[:9]] for c in cols], x.plain(alpha), 5, [x.plain(e) for e in old[:9]])
    assert combine_model(x, pc, 9, alpha, 5, old[:9]) == [x.stored(e) for e in ref]
    for first_power in (0, 5):
        for accumulate in (0, 1):
            full = combine_model(x, pc, 300, alpha, first_power, old[:300] if accumulate else None)
            for rows in list(range(1, 301)) + [big]:
                want = full[:rows] if rows <= 300 else combine_model(x, pc, rows, alpha, first_power, old[:rows] if accumulate else None)
                variant = (rows + count) % 3     # compact and aligned, columns with gaps of three words, everything off alignment
                stride = rows if variant != 1 else rows + 3
                shift = 1 if variant == 2 else 0
                ar = Arena(x, (count + x.d) * (stride + 3) + 4 * GUARD + 32)
                at = ar.add("cols", rows, stride, count, shift)
                for j in range(count):
                    ar.host[at + j * stride:at + j * stride + rows] = cols[j][:rows]
                ar.add("out", rows, stride, x.d, shift, old[:rows] if accumulate else None)
                ar.upload()
                rc = L.ark_hip_xfp_combine_columns(x.sid, ar.ptr("cols"), count, stride, rows, elem4(alpha), first_power, ar.ptr("out"), stride,
                                                   accumulate)
                assert rc == 0, (name, count, rows, rc)
                ar.check("out", want, (name, count, rows, first_power, accumulate, variant))


# ---- fold -----------------------------------------------------------------------------------------------------------------------
def fold_betas(x, rng):
    return [x.zero(), x.one(), x.stored(x.base(rng.randrange(2, x.p))), x.random_element(rng)]


def run_fold(x, dom, a, beta, layer, shift, stride_in, stride_out):
    n, m = len(layer), len(layer) >> a
    ar = Arena(x, x.d * (stride_in + stride_out) + 4 * GUARD + 32)
    ar.add("in", n, stride_in, x.d, shift, layer)
    ar.add("out", m, stride_out, x.d, shift)
    ar.upload()
    rc = _lib.lib().ark_hip_fri_fold(x.sid, C.byref(dom._s), a, elem4(beta), ar.ptr("in"), stride_in, ar.ptr("out"), stride_out)
    assert rc == 0, (x.name, n, a, rc)
    return ar


@pytest.mark.parametrize("a", [1, 2, 3])
@pytest.mark.parametrize("name", FIELDS)
def test_fold(name, a):
    x, f = X.FIELDS[name], R.FIELDS[name]
    rng = X.rng(60 + a)
    for k in range(a, 15):
        n, m = 1 << k, 1 << (k - a)
        layer = ext_inputs(x, n, 61 + k)
        plain = [x.plain(e) for e in layer]
        for hi, h in enumerate((1, x.gen)):
            dom = A.SmallRadix2EvaluationDomain.new(name, n).get_coset(x.st(h))
            betas = fold_betas(x, rng)
            variants = [(0, n, m), (0, n + 3, m + 3), (1, n, m), (0, n + 16 // x.bytes, m + 16 // x.bytes)]
            full = (k + hi) % 4     # k <= 10: every beta at every position; above: one beta whole, the others at the seams and samples
            for bi, beta in enumerate(betas):
                shift, s_in, s_out = variants[(k + a + hi + bi) % 4]
                ar = run_fold(x, dom, a, beta, layer, shift, s_in, s_out)
                if k <= 10 or bi == full:
                    want = [x.stored(e) for e in x.fold_eval(plain, k, h, a, x.plain(beta))]
                    ar.check("out", want, (name, k, a, h, bi, shift, s_in))
                else:
                    out = ar.check_outside("out", (name, k, a, h, bi, shift, s_in))
                    at = ar.regions["out"][0]
                    pos = sorted({i for i in SEAMS + (m - 1, m - 2, m // 2, m // 2 - 1) if 0 <= i < m} | {rng.randrange(m) for _ in range(48)})
                    w = x.omega(k)
                    for i in pos:
                        row = [plain[i + j * m] for j in range(1 << a)]
                        want = x.stored(x._fold_small(row, a, h * pow(w, i, x.p) % x.p, x.plain(beta)))
                        got = tuple(int(out[at + c * s_out + i]) for c in range(x.d))
                        assert got == want, (name, k, a, h, bi, i)
            fd = A.fri_folded_domain(dom, a)
            ref = A.SmallRadix2EvaluationDomain.new(name, m).get_coset(x.st(pow(h, 1 << a, x.p)))
            assert bytes(fd._s) == bytes(ref._s), (name, k, a, h)


@pytest.mark.parametrize("name", FIELDS)
def test_fold_is_the_coefficient_definition_on_the_device_transforms(name):
    """k <= 8: the device's inverse transform of the input, split by residue mod 2^a and recombined with powers of beta on the host,
    then the device's forward transform over the folded domain, equals the device's fold"""
    x = X.FIELDS[name]
    rng = X.rng(70)
    dt = dtype(x)
    for k in range(1, 9):
        for a in (1, 2, 3):
            if a > k:
                continue
            n, m = 1 << k, 1 << (k - a)
            for h in (1, x.gen):
                dom = A.SmallRadix2EvaluationDomain.new(name, n).get_coset(x.st(h))
                layer = [x.random_element(rng) for _ in range(n)]
                beta = x.random_element(rng)
                vec = A.SmallExtVec.from_host(name, np.array(x_cols(x, layer), dtype=dt))
                folded = A.fri_fold(vec, dom, a, beta)
                coeffs = A.SmallExtVec.from_host(name, np.array(x_cols(x, layer), dtype=dt))
                coeffs.matrix.fft_in_place(dom, inverse=True)
                c = [x.plain(e) for e in cols_x(coeffs.to_host())]
                g = []
                for t in range(m):
                    acc, bp = x.zero(), x.one()
                    for j in range(1 << a):
                        acc = x.add(acc, x.mul(bp, c[(t << a) + j]))
                        bp = x.mul(bp, x.plain(beta))
                    g.append(x.stored(acc))
                gv = A.SmallExtVec.from_host(name, np.array(x_cols(x, g), dtype=dt))
                gv.matrix.fft_in_place(A.fri_folded_domain(dom, a))
                assert np.array_equal(gv.to_host(), folded.to_host()), (name, k, a, h)
                assert cols_x(vec.to_host()) == layer


# ---- commit phase ---------------------------------------------------------------------------------------------------------------
def fold_counts(k, a):
    """numbers of folds with num_folds * a = k, with a short last fold, and with levels left over"""
    out = {-(-k // a), max(1, k // a - 1), 1}
    if k % a == 0:
        out.add(k // a)
    return sorted(out)


def run_commit_phase(x, k, h, a, num_folds, layer):
    dom = A.SmallRadix2EvaluationDomain.new(x.name, 1 << k).get_coset(x.st(h))
    vec = A.SmallExtVec.from_host(x.name, np.array(x_cols(x, layer), dtype=dtype(x)))
    prover = A.FriProver(vec, dom, a, num_folds)
    prover.commit_phase(X.shake_challenge(x, []))
    return dom, vec, prover


@pytest.mark.parametrize("a", [1, 2, 3])
@pytest.mark.parametrize("name", FIELDS)
def test_commit_phase_is_the_model_byte_for_byte(name, a):
    x = X.FIELDS[name]
    rng = X.rng(80 + a)
    for k in range(4, 13):
        layer = [x.random_element(rng) for _ in range(1 << k)]
        for num_folds in fold_counts(k, a):
            h = x.gen if (k + num_folds) % 2 else 1
            want = x.commit_phase(x_cols(x, layer), k, h, a, num_folds, X.shake_challenge(x, []))
            dom, vec, prover = run_commit_phase(x, k, h, a, num_folds, layer)
            what = (name, k, a, num_folds)
            assert prover.roots == want["roots"], what
            assert prover.betas == want["betas"], what
            assert prover.final_poly.tolist() == want["final"], what
            assert [l["log_arity"] for l in prover.plan["layers"]][:-1] == want["arities"], what
            for l in range(num_folds + 1):
                assert prover.layer_to_host(l).tolist() == want["layers"][l], what + (l,)
            for l in range(num_folds):
                assert [bytes(t) for t in prover.trees[l].to_host()] == want["trees"][l], what + (l,)
            assert cols_x(vec.to_host()) == layer, "layer 0 is the caller's and stays"
            prover.free()


@pytest.mark.parametrize("name", FIELDS)
def test_low_degree_codeword_folds_to_a_short_final_polynomial(name):
    """a codeword of degree < n / 4 on n = 2^10: after folds of total 2^s the final polynomial has degree < n / 2^(s + 2); one
    flipped component of one evaluation fills the coefficients above that bound"""
    x = X.FIELDS[name]
    rng = X.rng(90)
    k, h = 10, x.gen
    n = 1 << k
    dom = A.SmallRadix2EvaluationDomain.new(name, n).get_coset(x.st(h))
    coeffs = [x.random_element(rng) if i < n // 4 else x.zero() for i in range(n)]
    code = A.SmallExtVec.from_host(name, np.array(x_cols(x, coeffs), dtype=dtype(x)))
    code.matrix.fft_in_place(dom)
    host = code.to_host()
    for a, num_folds in ((1, 4), (2, 2), (3, 2)):
        s = sum(x.layer_arities(k, a, num_folds))
        bound = (n // 4) >> s
        prover = A.FriProver(code, dom, a, num_folds)
        prover.commit_phase(X.shake_challenge(x, []))
        assert prover.final_poly.shape == (x.d, n >> s)
        assert not prover.final_poly[:, bound:].any(), (name, a, num_folds)
        assert prover.final_poly[:, :bound].any()
        bad = host.copy()
        bad[1, 77] = (int(bad[1, 77]) + 1) % x.p
        bad_vec = A.SmallExtVec.from_host(name, bad)
        p2 = A.FriProver(bad_vec, dom, a, num_folds)
        p2.commit_phase(X.shake_challenge(x, []))
        assert p2.final_poly[:, bound:].any(), (name, a, num_folds)
        prover.free()
        p2.free()


@pytest.mark.parametrize("name", FIELDS)
def test_queries_verify_and_tampering_is_caught(name):
    x = X.FIELDS[name]
    rng = X.rng(91)
    for k, a, num_folds in ((9, 1, 5), (10, 2, 4), (11, 3, 4)):
        layer = [x.random_element(rng) for _ in range(1 << k)]
        transcript = []
        dom = A.SmallRadix2EvaluationDomain.new(name, 1 << k).get_coset(x.st(x.gen))
        vec = A.SmallExtVec.from_host(name, np.array(x_cols(x, layer), dtype=dtype(x)))
        prover = A.FriProver(vec, dom, a, num_folds)
        prover.commit_phase(X.shake_challenge(x, transcript))
        seed = hashlib.shake_256(b"".join(transcript) + prover.final_poly.tobytes()).digest(16 * 8)
        indices = [int.from_bytes(seed[8 * i:8 * i + 8], "little") % (1 << k) for i in range(16)]
        per_layer = prover.query(indices)
        final = prover.final_poly
        for q, index in enumerate(indices):
            openings = [(rows[q], paths[q]) for _, rows, paths in per_layer]
            args = (dom, a, num_folds, prover.roots, prover.betas)
            assert A.fri_verify_query(*args, final, index, openings), (name, k, a, q)
            # the model's verifier agrees
            mo = [(rows[q].tolist(), [bytes(pp) for pp in paths[q]]) for _, rows, paths in per_layer]
            assert x.verify_query(k, x.gen, a, num_folds, prover.roots, prover.betas, final.tolist(), index, mo), (name, k, a, q)
            if q >= 3:
                continue
            for l in (0, num_folds - 1):      # a flipped bit in a row, in a path, in a final coefficient
                row, path = openings[l]
                bad_row = row.copy()
                bad_row[(q + l) % bad_row.size] ^= 1
                assert not A.fri_verify_query(*args, final, index, openings[:l] + [(bad_row, path)] + openings[l + 1:])
                if path.size:
                    bad_path = path.copy()
                    bad_path[(q + l) % bad_path.shape[0], 5] ^= 0x10
                    assert not A.fri_verify_query(*args, final, index, openings[:l] + [(row, bad_path)] + openings[l + 1:])
            bad_final = final.copy()
            bad_final[x.d - 1, q % final.shape[1]] ^= 1
            assert not A.fri_verify_query(*args, bad_final, index, openings)
        prover.free()


def test_end_to_end_extend_commit_combine_fold_query():
    """8 BabyBear columns of 2^8 evaluations extended 4x on the device and committed; alpha from the root; the combination folded;
    queries check the combined value against the opened matrix row without downloading the matrix"""
    name = "BABYBEAR"
    x, f = X.FIELDS[name], R.FIELDS[name]
    rng = X.rng(95)
    count, small, big = 8, 1 << 8, 1 << 10
    cols = [[rng.randrange(x.p) for _ in range(small)] for _ in range(count)]
    mat = A.SmallDeviceMatrix.from_host(name, np.array(cols, dtype=np.uint32), stride=big)
    d0 = A.SmallRadix2EvaluationDomain.new(name, small)
    d1 = A.SmallRadix2EvaluationDomain.new(name, big).get_coset(x.st(x.gen))
    mat.low_degree_extend(d0, d1)
    tree = mat.commit(n=big)
    alpha = X.shake_challenge(x, [])(tree.root)
    combined = A.combine_columns(mat, big, alpha)
    transcript = [tree.root]
    prover = A.FriProver(combined, d1, 2, 3)
    prover.commit_phase(X.shake_challenge(x, transcript))
    assert not prover.final_poly[:, small >> 6:].any(), "the combination of degree < 2^8 polynomials folds to degree < 2^8 / 2^6"
    seed = hashlib.shake_256(b"".join(transcript)).digest(8 * 16)
    indices = [int.from_bytes(seed[8 * i:8 * i + 8], "little") % big for i in range(16)]
    mrows, mpaths = tree.open(indices)
    per_layer = prover.query(indices)
    rows0 = big >> 2
    pa = x.plain(alpha)
    for q, index in enumerate(indices):
        assert A.MerkleTree.verify(name, tree.root, big, index, mrows[q], mpaths[q])
        want = x.stored(x.combine([[x.pl(int(v))] for v in mrows[q]], pa)[0])
        row = per_layer[0][1][q]
        j = index // rows0
        assert tuple(int(row[(c << 2) + j]) for c in range(x.d)) == want, "layer 0 at the query is the combination of the opened row"
        openings = [(rows[q], paths[q]) for _, rows, paths in per_layer]
        assert A.fri_verify_query(d1, 2, 3, prover.roots, prover.betas, prover.final_poly, index, openings)
    prover.free()


# ---- asynchrony -----------------------------------------------------------------------------------------------------------------
def test_entries_are_asynchronous_and_read_their_constants_before_they_return():
    """tests/fri_async_child.py: fold, combine_columns and vec_mul_const behind a busy context stream, the host copies of their
    challenges overwritten at once; two folds with different challenges and one wait"""
    env = dict(os.environ, ARK_HIP_LIB=_lib.TEST_LIB_PATH)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fri_async_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "fri async: 0 failed" in r.stdout, r.stdout[-3000:]
