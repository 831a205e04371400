// C ABI of libark_hip.so: sparse constraint matrices on the device -- the CSR handle, y = M x and y = M^T x over device vectors
// and the host-only plan (see include/ark_hip.h; kernels: spmv.cuh, the cut of rows into work:
// csr_plan.hpp).
#include "capi_core.hpp"
#include "capi_csr.hpp"
#include "spmv.cuh"
using namespace arkhip;
using namespace arkhip::capi;

namespace {

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}
// row_ptr[0] = 0 and non-decreasing (NULL only for no rows)
inline bool row_ptr_ok(size_t rows, const uint32_t* row_ptr) {
  if (!row_ptr) return rows == 0;
  if (row_ptr[0] != 0) return false;
  for (size_t r = 0; r < rows; r++)
    if (row_ptr[r + 1] < row_ptr[r]) return false;
  return true;
}
// one side onto the device: the arrays and the plan made from row_ptr.  The copies are enqueued; the caller waits.
int csr_side_upload(Context* c, CsrSide& s, size_t rows, size_t cols, size_t nnz, const uint32_t* row_ptr, const uint32_t* col_idx,
                    const uint64_t* vals) {
  s.rows = rows;
  s.cols = cols;
  s.nnz = nnz;
  const uint32_t zero = 0;
  if (!row_ptr) row_ptr = &zero;   // rows = 0
  CsrPlan plan;
  csr_plan_rows(rows, row_ptr, true, &plan, &s.n_stream, &s.n_lrow, &s.n_chunk);
  const size_t pw = plan.stream.size() + plan.chunk.size() + plan.lrow.size();
  if (s.csr_ptr.ensure((rows + 1) * 4) || (nnz && (s.csr_idx.ensure(nnz * 4) || s.csr_val.ensure(nnz * 32))) ||
      (pw && s.csr_work.ensure(pw * 4)))
    return ARK_HIP_ERR_NOMEM;
  const int rc = [&]() -> int {
    ARK_HIP_TRY(hipMemcpyAsync(s.csr_ptr.p, row_ptr, (rows + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (nnz) {
      ARK_HIP_TRY(hipMemcpyAsync(s.csr_idx.p, col_idx, nnz * 4, hipMemcpyHostToDevice, c->stream));
      ARK_HIP_TRY(hipMemcpyAsync(s.csr_val.p, vals, nnz * 32, hipMemcpyHostToDevice, c->stream));
    }
    u32* w = (u32*)s.csr_work.p;
    if (!plan.stream.empty()) ARK_HIP_TRY(hipMemcpyAsync(w, plan.stream.data(), plan.stream.size() * 4, hipMemcpyHostToDevice, c->stream));
    w += plan.stream.size();
    if (!plan.chunk.empty()) ARK_HIP_TRY(hipMemcpyAsync(w, plan.chunk.data(), plan.chunk.size() * 4, hipMemcpyHostToDevice, c->stream));
    w += plan.chunk.size();
    if (!plan.lrow.empty()) ARK_HIP_TRY(hipMemcpyAsync(w, plan.lrow.data(), plan.lrow.size() * 4, hipMemcpyHostToDevice, c->stream));
    return 0;
  }();
  // the plan's vectors and the caller's arrays are pageable and may die once this returns: every copy out of them is done
  // before the frame is left, whether or not a later one could be enqueued
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  ARK_HIP_TRY(e);
  return 0;
}
inline CsrView csr_view(const CsrSide& s) {
  CsrView v;
  v.row_ptr = (const u32*)s.csr_ptr.p;
  v.col_idx = (const u32*)s.csr_idx.p;
  v.vals = (const char*)s.csr_val.p;
  v.stream = (const u32*)s.csr_work.p;
  v.chunk = v.stream + 2 * s.n_stream;
  v.lrow = v.chunk + 2 * s.n_chunk;
  v.n_stream = s.n_stream;
  v.n_chunk = s.n_chunk;
  v.n_lrow = s.n_lrow;
  return v;
}

}  // namespace

extern "C" {

int ark_hip_csr_plan(size_t rows, const uint32_t* row_ptr, int* tile, int* max_rows, size_t* blocks, size_t* long_rows,
                     size_t* long_chunks) {
  if (rows >= ((size_t)1 << 32) || !row_ptr_ok(rows, row_ptr)) return ARK_HIP_ERR_ARG;
  if (tile) *tile = CSR_TILE;
  if (max_rows) *max_rows = CSR_MAX_ROWS;
  const uint32_t zero = 0;
  csr_plan_rows(rows, row_ptr ? row_ptr : &zero, false, nullptr, blocks, long_rows, long_chunks);
  return 0;
}

int ark_hip_fr_csr_create(int field, size_t rows, size_t cols, const uint32_t* row_ptr, const uint32_t* col_idx,
                          const uint64_t* vals, size_t nnz, unsigned flags, ark_hip_fr_csr** out) {
  const size_t lim = (size_t)1 << 32;
  if (!field_ops(field) || !out || (flags & ~ARK_HIP_CSR_WITH_TRANSPOSE) || rows >= lim || cols >= lim || nnz >= lim)
    return ARK_HIP_ERR_ARG;
  if ((nnz && (!col_idx || !vals)) || !row_ptr_ok(rows, row_ptr)) return ARK_HIP_ERR_ARG;
  if ((row_ptr ? (size_t)row_ptr[rows] : (size_t)0) != nnz) return ARK_HIP_ERR_ARG;
  for (size_t j = 0; j < nnz; j++)
    if (col_idx[j] >= cols) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  CsrHandle* h = new CsrHandle();
  h->field = field;
  h->logical = c->logical;
  h->has_t = (flags & ARK_HIP_CSR_WITH_TRANSPOSE) != 0;
  int rc = csr_side_upload(c, h->side[0], rows, cols, nnz, row_ptr, col_idx, vals);
  if (rc == 0 && h->has_t) {
    // M^T by a stable counting sort over the columns: inside a row of M^T the entries keep ascending original row order
    std::vector<uint32_t> t_ptr(cols + 1, 0), t_idx(nnz);
    std::vector<uint64_t> t_val(nnz * 4);
    for (size_t j = 0; j < nnz; j++) t_ptr[(size_t)col_idx[j] + 1]++;
    for (size_t q = 0; q < cols; q++) t_ptr[q + 1] += t_ptr[q];
    std::vector<uint32_t> at(t_ptr.begin(), t_ptr.end() - 1);
    for (size_t r = 0; r < rows; r++)
      for (size_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
        const size_t d = at[col_idx[j]]++;
        t_idx[d] = (uint32_t)r;
        memcpy(&t_val[4 * d], vals + 4 * j, 32);
      }
    rc = csr_side_upload(c, h->side[1], cols, rows, nnz, t_ptr.data(), t_idx.data(), t_val.data());
  }
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    h->side[0].release();
    h->side[1].release();
    delete h;
    return rc;
  }
  *out = (ark_hip_fr_csr*)h;
  return 0;
}

int ark_hip_fr_csr_free(ark_hip_fr_csr* m) {
  if (!m) return 0;
  CsrHandle* h = (CsrHandle*)m;
  Scope sc;
  if (int rc = sc.enter(h->logical)) return rc;
  if (int rc = sync_compute(sc.c)) return rc;   // a product in flight may still read the arrays
  h->side[0].release();
  h->side[1].release();
  delete h;
  return 0;
}

int ark_hip_fr_csr_mul_device(const ark_hip_fr_csr* m, int transpose, const void* d_x, size_t x_len, void* d_y, size_t y_len) {
  const CsrHandle* h = (const CsrHandle*)m;
  if (!h || (transpose != 0 && transpose != 1) || (transpose && !h->has_t)) return ARK_HIP_ERR_ARG;
  const CsrSide& s = h->side[transpose];
  if (x_len != s.cols || y_len != s.rows || (x_len && !d_x) || (y_len && !d_y)) return ARK_HIP_ERR_ARG;
  if (x_len && y_len && ranges_overlap(d_x, x_len * 32, d_y, y_len * 32)) return ARK_HIP_ERR_ARG;
  const FieldOps* ops = field_ops(h->field);
  if (!ops) return ARK_HIP_ERR_ARG;
  Scope sc;
  if (int rc = sc.enter(h->logical)) return rc;
  Context* c = sc.c;
  if (y_len == 0) return 0;
  const CsrView v = csr_view(s);
  if (int rc = ops->csr_stream(v, d_x, d_y, c->stream)) return rc;
  if (s.n_lrow) {
    // the long rows' partials: grows only with every stream idle, earlier asynchronous calls may still be using the buffer
    if (c->poly_work.cap < s.n_chunk * 32)
      if (int rc = sync_compute(c)) return rc;
    if (c->poly_work.ensure(s.n_chunk * 32)) return ARK_HIP_ERR_NOMEM;
    if (int rc = ops->csr_long(v, d_x, c->poly_work.p, d_y, c->stream)) return rc;
  }
  return mark_producer(c);
}

}  // extern "C"
