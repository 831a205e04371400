"""Sparse constraint matrices on the device: the CSR handle of include/ark_hip.h (ark_hip_fr_csr_*) and
its products with device vectors -- A z, B z, C z of an R1CS / CCS instance, M^T eq(rx), and the sparse multilinear
extension's value eq(rx)^T M eq(ry) (`SparseMultilinearExtension::evaluate` of ark-poly for a matrix).  The Python mirror of
`ark_hip::CsrMatrix` (C++: include/ark_hip.hpp, Rust: rust/ark-hip/src/device.rs).  No arithmetic here."""
import ctypes as C

import numpy as np

from . import curves as cv
from ._lib import check, lib
from .poly import DeviceVec

CSR_WITH_TRANSPOSE = 1


def csr_plan(rows, row_ptr):
    """(tile, max_rows, blocks, long_rows, long_chunks): how a handle with these row_ptr (rows + 1 entries) is cut into work
    (ark_hip_csr_plan; host only, no device needed)."""
    rp = np.ascontiguousarray(row_ptr, dtype=np.uint32).reshape(-1)
    if rp.size != rows + 1:
        raise ValueError("row_ptr must have rows + 1 entries")
    t, mr = C.c_int(), C.c_int()
    b, lr, lc = C.c_size_t(), C.c_size_t(), C.c_size_t()
    check(lib().ark_hip_csr_plan(rows, rp.ctypes.data_as(C.c_void_p), C.byref(t), C.byref(mr), C.byref(b), C.byref(lr), C.byref(lc)),
          "ark_hip_csr_plan")
    return t.value, mr.value, b.value, lr.value, lc.value


class CsrMatrix:
    """A rows x cols matrix over Fr in CSR form on the current GPU.  row_ptr: rows + 1 uint32, col_idx: nnz uint32, vals:
    numpy uint64 [nnz, 4] (Montgomery), all on the host; they are validated and copied once.  transpose=True also keeps M^T
    (stable order), which `mul_t` needs."""

    def __init__(self, field, rows, cols, row_ptr, col_idx, vals, transpose=False):
        self.field = cv.field_id(field)
        self.rows, self.cols = int(rows), int(cols)
        rp = np.ascontiguousarray(row_ptr, dtype=np.uint32).reshape(-1)
        ci = np.ascontiguousarray(col_idx, dtype=np.uint32).reshape(-1)
        v = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, 4)
        if rp.size != self.rows + 1 or v.shape[0] != ci.size:
            raise ValueError("row_ptr must have rows + 1 entries, vals one element per column index")
        self.nnz = int(ci.size)
        self.has_transpose = bool(transpose)
        self._h = C.c_void_p(0)
        check(lib().ark_hip_fr_csr_create(self.field, self.rows, self.cols, rp.ctypes.data_as(C.c_void_p),
                                          ci.ctypes.data_as(C.c_void_p) if self.nnz else None,
                                          v.ctypes.data_as(C.c_void_p) if self.nnz else None, self.nnz,
                                          CSR_WITH_TRANSPOSE if transpose else 0, C.byref(self._h)), "ark_hip_fr_csr_create")

    def free(self):
        if self._h and self._h.value:
            check(lib().ark_hip_fr_csr_free(self._h), "ark_hip_fr_csr_free")
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def _mul(self, t, x, out):
        n_in, n_out = (self.rows, self.cols) if t else (self.cols, self.rows)
        if x.field != self.field or x.len != n_in:
            raise ValueError("the vector's field or length does not fit the matrix")
        if out is None:
            out = DeviceVec(self.field, n_out, _zero=False)
        elif out.field != self.field or out.len != n_out:
            raise ValueError("the output's field or length does not fit the matrix")
        check(lib().ark_hip_fr_csr_mul_device(self._h, t, x.ptr, x.len, out.ptr, out.len), "ark_hip_fr_csr_mul_device")
        return out

    def mul(self, x, out=None):
        """y = M x as a DeviceVec of `rows` elements (x: `cols` elements); asynchronous.  out: the vector to write."""
        return self._mul(0, x, out)

    def mul_t(self, x, out=None):
        """y = M^T x as a DeviceVec of `cols` elements (x: `rows` elements); needs transpose=True."""
        return self._mul(1, x, out)

    def bilinear(self, u, v):
        """u^T M v as a numpy uint64[4]; waits for it.  With u = eq(rx, .), v = eq(ry, .) (DenseMultilinearExtension.eq) that
        is the value of the matrix's sparse multilinear extension at (rx, ry)."""
        t = self.mul(v)
        try:
            return u.inner_product(t)
        finally:
            t.free()
