"""Child process of tests/test_gpu_csr.py::test_long_rows_on_poisoned_scratch, run with
ARK_HIP_LIB=algebra_amd/libark_hip_test.so so that the Python mirror and the hooks are one library instance (the protocol and
the helpers are those of tests/scratch_reuse_child.py).

The products of a CSR handle keep one partial per chunk of a long row in Context::poly_work, which only grows and is never
cleared; the handle's own arrays are caches and are not poisoned.  Each case runs warm, then with every scratch buffer
filled with the poison word, then poisoned again after a larger call on the same context: the results are those of the
big-integer model every time, no buffer moved, and nothing was written past what the call asked for.

Before that, the same process reads handles back through the hook ark_hip_test_csr_dump: M is the caller's arrays and M^T is
the model's stable transposition, array by array."""
import ctypes as C

import numpy as np

import scratch_reuse_child as H         # asserts the library instance, brings poison() and assert_clean()
import algebra_amd as A
import csr_ref as R

FNAME = "BLS12_381_FR"
F = R.Field(FNAME)


def case(lens, cols, seed, transpose=False, checked=True):
    rows = len(lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nnz = int(row_ptr[-1])
    col_idx = np.random.default_rng(seed).integers(0, cols, size=nnz).astype(np.uint32)
    if transpose:
        col_idx[::2] = 0                 # a dense column: row 0 of M^T is long
    vals = R.rand_elems(F, nnz, seed + 1)
    x = R.rand_elems(F, rows if transpose else cols, seed + 2)
    m = A.CsrMatrix(FNAME, rows, cols, row_ptr, col_idx, R.limbs(vals), transpose=transpose)
    dx = A.DeviceVec.from_host(FNAME, R.limbs(x))
    if checked:
        if transpose:
            t_ptr, t_idx, t_vals = R.transpose(rows, cols, row_ptr, col_idx, vals)
            want = R.limbs(R.mul(F, cols, t_ptr, t_idx, t_vals, x))
        else:
            want = R.limbs(R.mul(F, rows, row_ptr, col_idx, vals, x))

    def run():
        y = m.mul_t(dx) if transpose else m.mul(dx)
        got = y.to_host()
        y.free()
        return not checked or np.array_equal(got, want)
    return run


def dump(m, transpose):
    """(row_ptr, col_idx, vals) of one side of the handle as the device holds them (ark_hip_test_csr_dump)"""
    dims = (C.c_size_t * 3)()
    H._lib.check(H.T.ark_hip_test_csr_dump(m._h, transpose, dims, None, 0, None, None, 0), "ark_hip_test_csr_dump")
    rows, nnz = dims[0], dims[2]
    rp, ci, va = np.zeros(rows + 1, dtype=np.uint32), np.zeros(nnz, dtype=np.uint32), np.zeros((nnz, 4), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    H._lib.check(H.T.ark_hip_test_csr_dump(m._h, transpose, dims, p(rp), rp.size, p(ci), p(va), nnz), "ark_hip_test_csr_dump")
    return (dims[0], dims[1], dims[2]), rp, ci, va


def structure(lens, cols, seed, dense_col0=False):
    """the handle's M is the caller's arrays and its M^T the model's stable transposition, array by array"""
    rows = len(lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nnz = int(row_ptr[-1])
    col_idx = np.random.default_rng(seed).integers(0, max(cols, 1), size=nnz).astype(np.uint32)
    if dense_col0:
        col_idx[::3] = 0
    vals = R.limbs(R.rand_elems(F, nnz, seed + 1))
    m = A.CsrMatrix(FNAME, rows, cols, row_ptr, col_idx, vals, transpose=True)
    dims, rp, ci, va = dump(m, 0)
    assert dims == (rows, cols, nnz) and np.array_equal(rp, row_ptr) and np.array_equal(ci, col_idx) and np.array_equal(va, vals)
    t_ptr, t_idx, t_vals = R.transpose(rows, cols, row_ptr, col_idx, vals)
    dims, rp, ci, va = dump(m, 1)
    assert dims == (cols, rows, nnz), dims
    assert np.array_equal(rp, t_ptr), "row_ptr of the transpose"
    assert np.array_equal(ci, t_idx), "col_idx of the transpose: ascending original rows inside every row"
    assert np.array_equal(va, t_vals), "vals of the transpose follow their entries"
    m.free()
    plain = A.CsrMatrix(FNAME, rows, cols, row_ptr, col_idx, vals)
    d3 = (C.c_size_t * 3)()
    assert H.T.ark_hip_test_csr_dump(plain._h, 1, d3, None, 0, None, None, 0) == -1      # no transpose in this handle
    plain.free()


def main():
    T = A.csr_plan(0, [0])[0]
    structure([0, 3, 0, 0, 2, 5, 1, 0], 4, 0x71)                           # duplicates inside rows, empty rows and columns
    structure([1 + i % 4 for i in range(T + 99)], 300, 0x73, dense_col0=True)   # a dense column: a long row of M^T
    structure([2, 3 * T + 5, 0, T + 1], 50, 0x75)                          # long rows of M, many duplicates
    structure([0] * 7, 3, 0x77)                                            # nnz = 0
    structure([], 0, 0x79)                                                 # 0 x 0
    print("ok the transposed structure, array by array", flush=True)
    big = case([40 * T + 1], 3000, 0x63, checked=False)                    # 41 partials: a larger poly_work
    H.protocol("csr mul: two long rows, ragged chunks", case([2, T + 1, 3 * T + 5, 0, 1], 3000, 0x61), big=big, reach=("poly_work",))
    H.protocol("csr mul: one row holding everything", case([3 * T + 5], 3000, 0x65), big=big, reach=("poly_work",))
    H.protocol("csr mul_t: a dense column", case([3] * (2 * T), 700, 0x67, transpose=True), big=big, reach=("poly_work",))
    print("csr scratch ok", flush=True)


if __name__ == "__main__":
    main()
