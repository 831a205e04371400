"""Sparse matrices on the device (ark_hip_fr_csr_create, _mul_device) through the Python mirror, limb for limb against the
big-integer model of tests/csr_ref.py -- never against the code under test.  Outputs are canonical Montgomery residues: no
tolerance anywhere.

Every shape is the smallest at which a path of csrc/spmv.cuh can go wrong (tile = max_rows = 2048 from the plan): block and
chunk seams, rows around the tile, long rows in every position, empty rows, the dense column whose transpose is a long row.
Each matrix is multiplied as M (a handle without the transpose), as M^T through a handle with it, and as the model's own
stable transposition handed over as a third handle: the transposed structure the library builds gives the same vector as
the model's arrays do."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd._lib import lib
import csr_ref as R
import mle_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1

FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
T, MR = A.csr_plan(0, [0])[:2]


@functools.lru_cache(maxsize=None)
def field(fname):
    return R.Field(fname)


def matrix(fname, lens, cols, seed, dense_col0=False):
    """(row_ptr, col_idx, vals as integers): random columns (duplicates inside a row happen) and random stored values, with
    0, 1, -1 and p - 1 planted on both sides of every block and chunk seam of the plan and at both ends"""
    f = field(fname)
    rows = len(lens)
    row_ptr = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.uint32)
    nnz = int(row_ptr[-1])
    rng = np.random.default_rng(seed)
    col_idx = rng.integers(0, max(cols, 1), size=nnz).astype(np.uint32)
    if dense_col0:
        for r in range(rows):
            if lens[r]:
                col_idx[int(row_ptr[r])] = 0
    vals = R.rand_elems(f, nnz, seed + 1)
    special = [0, f.one, f.enc(-1), f.p - 1]
    stream, longs, _ = R.plan(rows, row_ptr, T, MR)
    seams = {0, nnz}
    for r0, r1 in stream:
        seams |= {int(row_ptr[r0]), int(row_ptr[r1])}
    for r, chunks in longs:
        seams |= {int(row_ptr[r]) + k * T for k in range(chunks)} | {int(row_ptr[r + 1])}
    for k, s in enumerate(sorted(seams)):
        if s - 1 >= 0 and nnz:
            vals[s - 1] = special[k % 4]
        if s < nnz:
            vals[s] = special[(k + 1) % 4]
    return row_ptr, col_idx, vals


def vector(fname, n, seed):
    """n random stored values with zeros, one, -1 and p - 1 among them"""
    f = field(fname)
    x = R.rand_elems(f, n, seed)
    for i, v in zip(range(0, n, max(n // 7, 1)), [0, f.one, 0, f.enc(-1), f.p - 1, 0, 0]):
        x[i] = v
    return x


def dev(fname, xs):
    return A.DeviceVec.from_host(fname, R.limbs(xs))


def check_all(fname, lens, cols, seed, dense_col0=False):
    f = field(fname)
    rows = len(lens)
    row_ptr, col_idx, vals = matrix(fname, lens, cols, seed, dense_col0)
    x, u = vector(fname, cols, seed + 2), vector(fname, rows, seed + 3)
    want = R.limbs(R.mul(f, rows, row_ptr, col_idx, vals, x))
    t_ptr, t_idx, t_vals = R.transpose(rows, cols, row_ptr, col_idx, vals)
    want_t = R.limbs(R.mul(f, cols, t_ptr, t_idx, t_vals, u))
    dx, du = dev(fname, x), dev(fname, u)
    plain = A.CsrMatrix(fname, rows, cols, row_ptr, col_idx, R.limbs(vals))
    both = A.CsrMatrix(fname, rows, cols, row_ptr, col_idx, R.limbs(vals), transpose=True)
    model_t = A.CsrMatrix(fname, cols, rows, t_ptr, t_idx, R.limbs(t_vals))
    try:
        for m in (plain, both):
            y = m.mul(dx)
            got = y.to_host()
            y.free()
            assert got.shape == want.shape and np.array_equal(got, want), ("mul", np.nonzero((got != want).any(axis=1))[0][:5])
        for m, product in ((both, both.mul_t), (model_t, model_t.mul)):
            y = product(du)
            got = y.to_host()
            y.free()
            assert got.shape == want_t.shape and np.array_equal(got, want_t), ("mul_t", m is both, np.nonzero((got != want_t).any(axis=1))[0][:5])
        assert np.array_equal(dx.to_host(), R.limbs(x)) and np.array_equal(du.to_host(), R.limbs(u))   # the inputs untouched
        with pytest.raises(A.ArkHipError) as e:
            plain.mul_t(du)                                   # transpose without the flag
        assert e.value.code == ERR_ARG
    finally:
        for m in (plain, both, model_t):
            m.free()
        dx.free()
        du.free()


SHAPES = {
    # name: (row lengths, cols)
    "nnz=0": ([0] * 5, 3),
    "1x1": ([1], 1),
    "cols=1": ([2, 0, 1, 3, 1] * 60, 1),
    "empty rows leading, trailing, consecutive": ([0, 0, 0, 2, 0, 0, 1, 3, 0, 0], 6),
    "more single-entry rows than lanes": ([1] * 700, 900),
    "max_rows closes a block of empty rows": ([1] + [0] * (MR + 3) + [2], 5),
    "a block of exactly tile": ([4] * (T // 4) + [5], 3000),
    "a block of tile - 1": ([4] * (T // 4 - 1) + [3] + [4], 3000),
    "tile + 1 does not fit": ([4] * (T // 4 - 1) + [5] + [1], 3000),
    "a row of tile - 1": ([2, T - 1, 3], 5000),
    "a row of tile": ([2, T, 3], 5000),
    "a row of tile + 1": ([2, T + 1, 3], 5000),
    "a row of 3 tile + 5": ([2, 3 * T + 5, 3], 5000),
    "a long row first": ([T + 1, 1, 2], 4000),
    "a long row last": ([1, 2, T + 1], 4000),
    "a long row between stream blocks": ([2] * 1500 + [T + 7] + [2] * 1500, 4000),
    "two long rows in succession": ([1, T + 1, 2 * T + 3, 1], 4000),
    "one row holding every nonzero": ([3 * T + 5], 7000),
}
ONE_FIELD = ("a long row between stream blocks", "max_rows closes a block of empty rows")   # the larger ones: BLS12-381 only
CASES = [(f, name) for f in FR for name in SHAPES if f == "BLS12_381_FR" or name not in ONE_FIELD]


def test_the_shapes_are_where_the_plan_says():
    assert (T, MR) == (2048, 2048) or T <= 1 << 16
    plan = lambda lens: A.csr_plan(len(lens), np.concatenate([[0], np.cumsum(lens)]))[2:]   # noqa: E731
    assert plan(SHAPES["a block of exactly tile"][0]) == (2, 0, 0)
    assert plan(SHAPES["a block of tile - 1"][0]) == (2, 0, 0)
    assert plan(SHAPES["tile + 1 does not fit"][0]) == (2, 0, 0)
    assert plan(SHAPES["a row of tile"][0]) == (3, 0, 0) and plan(SHAPES["a row of tile + 1"][0]) == (2, 1, 2)
    assert plan(SHAPES["a row of 3 tile + 5"][0]) == (2, 1, 4)
    assert plan(SHAPES["two long rows in succession"][0]) == (2, 2, 5)
    assert plan(SHAPES["max_rows closes a block of empty rows"][0]) == (2, 0, 0)


@pytest.mark.parametrize("fname,name", CASES)
def test_mul_and_mul_t(fname, name):
    lens, cols = SHAPES[name]
    check_all(fname, lens, cols, 100 + len(name))


@pytest.mark.parametrize("fname", FR)
def test_a_dense_column_makes_the_transpose_a_long_row(fname):
    """column 0 in every row: row 0 of M^T holds more than a tile (the constant-one column of an R1CS matrix)"""
    lens = [1 + (i % 3) for i in range(T + T // 2 + 9)]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    _, col_idx, _ = matrix(fname, lens, 500, 77, dense_col0=True)
    t_ptr = R.transpose(len(lens), 500, rp, col_idx, [0] * int(rp[-1]))[0]
    assert int(t_ptr[1]) >= len(lens) > T and A.csr_plan(500, t_ptr)[3] == 1
    check_all(fname, lens, 500, 77, dense_col0=True)


def test_degenerate_dimensions():
    """rows = 0, cols = 0, both: legal handles; the products write exactly y_len elements (zeros for cols = 0)"""
    fname = "BLS12_381_FR"
    empty = np.zeros((0, 4), dtype=np.uint64)
    m = A.CsrMatrix(fname, 0, 0, [0], [], empty, transpose=True)
    assert m.mul(A.DeviceVec(fname, 0)).to_host().shape == (0, 4) and m.mul_t(A.DeviceVec(fname, 0)).to_host().shape == (0, 4)
    m.free()
    m = A.CsrMatrix(fname, 0, 5, [0], [], empty, transpose=True)
    x5, x0 = dev(fname, vector(fname, 5, 1)), A.DeviceVec(fname, 0)
    assert m.mul(x5).to_host().shape == (0, 4)
    assert not m.mul_t(x0).to_host().any() and m.mul_t(x0).len == 5
    m.free()
    m = A.CsrMatrix(fname, 3, 0, [0, 0, 0, 0], [], empty, transpose=True)
    out = dev(fname, vector(fname, 3, 2))
    assert m.mul(x0, out=out) is out and not out.to_host().any()          # garbage in `out` is overwritten with zeros
    assert m.mul_t(out).to_host().shape == (0, 4)
    m.free()


def test_out_reuse_and_mul_device_argument_errors():
    """out= is written in full each time; every argument error of ark_hip_fr_csr_mul_device on a live handle"""
    fname = "BLS12_381_FR"
    f = field(fname)
    lens, cols = [2, 0, T + 3, 1], 300
    rows = len(lens)
    row_ptr, col_idx, vals = matrix(fname, lens, cols, 9)
    m = A.CsrMatrix(fname, rows, cols, row_ptr, col_idx, R.limbs(vals), transpose=True)
    out = dev(fname, vector(fname, rows, 5))
    for seed in (20, 21, 22):
        x = vector(fname, cols, seed)
        dx = dev(fname, x)
        assert m.mul(dx, out=out) is out
        assert np.array_equal(out.to_host(), R.limbs(R.mul(f, rows, row_ptr, col_idx, vals, x)))
        dx.free()
    L = lib()
    mul = L.ark_hip_fr_csr_mul_device
    dx, dy = A.DeviceVec(fname, cols), A.DeviceVec(fname, rows)
    big = A.DeviceVec(fname, cols + rows)
    at = lambda v, e: C.c_void_p(v.ptr.value + 32 * e)   # noqa: E731
    h = m._h
    assert mul(h, 0, dx.ptr, cols, dy.ptr, rows) == 0
    assert mul(h, 2, dx.ptr, cols, dy.ptr, rows) == ERR_ARG and mul(h, -1, dx.ptr, cols, dy.ptr, rows) == ERR_ARG
    assert mul(h, 0, dx.ptr, cols - 1, dy.ptr, rows) == ERR_ARG and mul(h, 0, dx.ptr, cols, dy.ptr, rows + 1) == ERR_ARG   # wrong lengths
    assert mul(h, 0, dy.ptr, rows, dx.ptr, cols) == ERR_ARG and mul(h, 1, dx.ptr, cols, dy.ptr, rows) == ERR_ARG           # swapped
    assert mul(h, 1, dy.ptr, rows, dx.ptr, cols) == 0
    assert mul(h, 0, None, cols, dy.ptr, rows) == ERR_ARG and mul(h, 0, dx.ptr, cols, None, rows) == ERR_ARG
    assert mul(h, 0, big.ptr, cols, at(big, cols), rows) == 0                                                             # adjacent: no overlap
    assert mul(h, 0, big.ptr, cols, at(big, cols - 1), rows) == ERR_ARG and mul(h, 0, at(big, 1), cols, big.ptr, rows) == ERR_ARG
    assert mul(h, 0, big.ptr, cols, big.ptr, rows) == ERR_ARG                                                             # in place: never
    with pytest.raises(ValueError):
        m.mul(dy)
    assert L.ark_hip_synchronize() == 0
    m.free()
    m.free()                                          # twice: nothing happens


# ---- end to end: nothing downloaded but the final comparison ------------------------------------------------------------------
def r1cs_squaring_chain(f, n, w0):
    """z = (1, w_0, .., w_n) with w_{i+1} = w_i^2, as constraints (w_i) (w_i) = w_{i+1} for i < n, and for every third i the
    constant-column constraint (w_i + 5) (1) = w_i + 5.  Returns (rows, cols, A, B, C as (row_ptr, col_idx, vals), z)."""
    z = [f.one, w0]
    for _ in range(n):
        z.append(f.mul(z[-1], z[-1]))
    one, five = f.one, f.enc(5)
    a, b, c = [], [], []
    for i in range(n):
        a.append([(1 + i, one)])
        b.append([(1 + i, one)])
        c.append([(2 + i, one)])
        if i % 3 == 0:
            a.append([(0, five), (1 + i, one)])
            b.append([(0, one)])
            c.append([(1 + i, one), (0, five)])

    def csr(rows_):
        rp = np.concatenate([[0], np.cumsum([len(r) for r in rows_])]).astype(np.uint32)
        return rp, np.array([cv for r in rows_ for cv, _ in r], dtype=np.uint32), [v for r in rows_ for _, v in r]
    return len(a), n + 2, csr(a), csr(b), csr(c), z


def test_a_satisfied_r1cs_gives_the_zero_vector():
    fname = "BLS12_381_FR"
    f = field(fname)
    rows, cols, a, b, c, z = r1cs_squaring_chain(f, 3 * T + 11, f.enc(3))
    ms = [A.CsrMatrix(fname, rows, cols, rp, ci, R.limbs(v)) for rp, ci, v in (a, b, c)]

    def residual(zs):
        dz = dev(fname, zs)
        az, bz, cz = (m.mul(dz) for m in ms)
        az *= bz
        az -= cz
        got = az.to_host()
        for v in (dz, az, bz, cz):
            v.free()
        return got
    assert not residual(z).any()
    bad = list(z)
    k = 1 + 2 * T                                      # one witness cell changed: w_k enters rows of A, B (as w_k) and C (as w_{k-1}^2)
    bad[k] = (bad[k] + f.one) % f.p
    got = residual(bad)
    assert got.any()
    hit = set(np.nonzero(got.any(axis=1))[0])
    touched = {r for rp, ci, _ in (a, b, c) for r in range(rows) if k in ci[int(rp[r]):int(rp[r + 1])]}
    assert hit and hit <= touched
    for m in ms:
        m.free()


@pytest.mark.parametrize("fname", FR)
def test_bilinear_is_the_sparse_mle_and_the_adjoint_identity(fname):
    f = field(fname)
    nu_r, nu_c = 9, 8
    rows, cols = 1 << nu_r, 1 << nu_c
    lens = [(i * 7) % 5 for i in range(rows)]
    lens[17] = T + 5                                   # one long row among them
    row_ptr, col_idx, vals = matrix(fname, lens, cols, 31)
    m = A.CsrMatrix(fname, rows, cols, row_ptr, col_idx, R.limbs(vals), transpose=True)
    rx, ry = R.rand_elems(f, nu_r, 41), R.rand_elems(f, nu_c, 42)
    ex = A.DenseMultilinearExtension.eq(fname, R.limbs(rx))
    ey = A.DenseMultilinearExtension.eq(fname, R.limbs(ry))
    got = m.bilinear(ex.evaluations, ey.evaluations)
    cx, cy = [v * f.rinv % f.p for v in rx], [v * f.rinv % f.p for v in ry]          # canonical coordinates
    eqx = [f.enc(mle_ref.eq(i, cx, f.p)) for i in range(rows)]
    eqy = [f.enc(mle_ref.eq(j, cy, f.p)) for j in range(cols)]
    want = R.bilinear(f, rows, row_ptr, col_idx, vals, eqx, eqy)
    assert R.ints(got.reshape(1, 4))[0] == want
    # <u, M v> = <M^T u, v> on random vectors, both sides on the device, and the model's value
    u, v = vector(fname, rows, 51), vector(fname, cols, 52)
    du, dv = dev(fname, u), dev(fname, v)
    mv, mtu = m.mul(dv), m.mul_t(du)
    lhs, rhs = du.inner_product(mv), mtu.inner_product(dv)
    assert np.array_equal(lhs, rhs) and R.ints(lhs.reshape(1, 4))[0] == R.bilinear(f, rows, row_ptr, col_idx, vals, u, v)
    assert np.array_equal(m.bilinear(du, dv), lhs)
    for x in (ex, ey, du, dv, mv, mtu, m):
        x.free()


def test_long_rows_on_poisoned_scratch():
    """tests/csr_scratch_child.py, where the mirror and the test hooks are one library instance: the arrays of M and of the M^T
    that create built, read back (ark_hip_test_csr_dump) and compared array by array with the model's stable transposition;
    then the long-row cases warm, with every scratch buffer poisoned (ark_hip_test_scratch_poison), and on poisoned scratch
    left behind by a larger call: the model's results each time, nothing written past what was asked for"""
    env = dict(os.environ, ARK_HIP_LIB=os.path.join(ROOT, "algebra_amd", "libark_hip_test.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "csr_scratch_child.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "csr scratch ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    assert "ok the transposed structure, array by array" in out.stdout
