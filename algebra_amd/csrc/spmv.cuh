// Sparse matrix times device vector over Fr: y = M x for a CSR matrix that lives on the device, the step
// in front of every R1CS / CCS prover (A z, B z, C z; M^T eq(rx); the sparse multilinear extension's value).
//   csr_stream_kernel   one workgroup per STREAM block (csr_plan.hpp: consecutive rows, at most CSR_TILE nonzeros and
//                       CSR_MAX_ROWS rows): the lanes walk the block's nonzeros coalesced over col_idx / vals, gather x[col]
//                       and put the Montgomery products into the LDS limb planes of polyops.cuh; after one barrier the lanes
//                       take rows and add each row's products.  Empty rows get zero.
//   csr_chunk_kernel    one workgroup per chunk of a LONG row (more than CSR_TILE nonzeros: the constant-one column of M^T):
//                       every lane sums its products, the workgroup adds its lanes through LDS and leaves ONE partial.
//   csr_fold_kernel     one workgroup per long row adds that row's partials and writes y[row].
// Order between the phases comes from kernel boundaries only; no field element is ever updated atomically and no workgroup
// waits on another.  Every y cell is written by exactly one lane of exactly one kernel: a row belongs to one stream block or is
// one long row.  Every product is a canonical Montgomery product and every sum a canonical modular addition, so the result is
// the canonical residue whatever the order -- bit-exact against big integers.
//
// Nothing here checks an index: ark_hip_fr_csr_create validated row_ptr and col_idx on the host before the handle existed,
// and ark_hip_fr_csr_mul_device checks the lengths of x and y against the handle.
#pragma once
#include "polyops.cuh"
#include "csr_plan.hpp"

namespace arkhip {

static_assert(CSR_TILE == POLY_TILE, "a stream block's products fill the limb planes of polyops.cuh");
static_assert(CSR_MAX_ROWS % POLY_THREADS == 0, "rows of a block are taken in rounds of one per lane");

// one side (M or M^T) of a handle as the kernels see it; every pointer is device memory
struct CsrView {
  const u32* row_ptr;   // rows + 1
  const u32* col_idx;   // nnz
  const char* vals;     // nnz elements
  const u32* stream;    // 2 per stream block: first row, one past the last
  const u32* chunk;     // 2 per chunk: row, index of the chunk inside the row
  const u32* lrow;      // 3 per long row: row, first partial, number of chunks
  size_t n_stream, n_chunk, n_lrow;
};

// the workgroup's lanes' values -> their sum in lane 0 (every lane must call it; lds: planes of at least POLY_THREADS words)
template <class F, int PLANE>
ARK_DEV F csr_sum_lanes(u32 (*lds)[PLANE], F h) {
  const u32 tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < F::N; j++) lds[j][tid] = h.l[j];
#pragma unroll
  for (int s = POLY_LOG_THREADS - 1; s >= 0; s--) {
    const u32 d = 1u << s;
    __syncthreads();
    if (tid < d) {
      F o;
#pragma unroll
      for (int j = 0; j < F::N; j++) o.l[j] = lds[j][tid + d];
      h = F::add(h, o);
#pragma unroll
      for (int j = 0; j < F::N; j++) lds[j][tid] = h.l[j];
    }
  }
  return h;
}

// fn(e, vals[start + e] x[col_idx[start + e]]) for this lane's e < cnt, e = tid, tid + 256, ...: four nonzeros are loaded
// (value and gathered x) before the first of their products is formed, so a lane keeps eight 32-byte loads in flight
template <class F, class Fn>
ARK_DEV void csr_lane_products(const CsrView& m, const char* x, size_t start, u32 cnt, Fn&& fn) {
  constexpr int B = 4;
  const u32 tid = threadIdx.x;
  for (u32 e0 = 0; e0 < cnt; e0 += B * POLY_THREADS) {   // the same trip count for every lane of the workgroup
    F v[B], xv[B];
#pragma unroll
    for (int k = 0; k < B; k++) {
      const u32 e = e0 + (u32)k * POLY_THREADS + tid;
      v[k] = F::zero();
      xv[k] = F::zero();
      if (e < cnt) {
        const size_t j = start + e;
        v[k] = F::load(m.vals + j * F::BYTES);
        xv[k] = F::load(x + (size_t)m.col_idx[j] * F::BYTES);
      }
    }
#pragma unroll
    for (int k = 0; k < B; k++) {
      const u32 e = e0 + (u32)k * POLY_THREADS + tid;
      if (e < cnt) fn(e, F::mul(v[k], xv[k]));
    }
  }
}

template <class F>
__global__ void __launch_bounds__(POLY_THREADS) csr_stream_kernel(CsrView m, const char* x, char* y) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  __shared__ u32 lds[F::N][POLY_PLANE];
  const u32 tid = threadIdx.x;
  const u32 r0 = m.stream[2 * (size_t)blockIdx.x], r1 = m.stream[2 * (size_t)blockIdx.x + 1];
  const u32 base = m.row_ptr[r0];
  const u32 cnt = m.row_ptr[r1] - base;   // <= CSR_TILE by the plan
  csr_lane_products<F>(m, x, base, cnt, [&](u32 e, const F& prod) { poly_lds_put<F>(lds, e + (e >> 3), prod); });
  __syncthreads();
  for (u32 r = r0 + tid; r < r1; r += POLY_THREADS) {   // r1 - r0 <= CSR_MAX_ROWS
    const u32 a = m.row_ptr[r] - base, b = m.row_ptr[r + 1] - base;
    F acc = F::zero();
    for (u32 e = a; e < b; e++) acc = F::add(acc, poly_lds_get<F>(lds, e + (e >> 3)));
    acc.store(y + (size_t)r * F::BYTES);
  }
}

template <class F>
__global__ void __launch_bounds__(POLY_THREADS) csr_chunk_kernel(CsrView m, const char* x, char* partials) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  __shared__ u32 lds[F::N][POLY_THREADS];
  const u32 tid = threadIdx.x;
  const u32 row = m.chunk[2 * (size_t)blockIdx.x], k = m.chunk[2 * (size_t)blockIdx.x + 1];
  const size_t start = (size_t)m.row_ptr[row] + (size_t)k * CSR_TILE, end = m.row_ptr[row + 1];
  const u32 cnt = end - start < (size_t)CSR_TILE ? (u32)(end - start) : (u32)CSR_TILE;   // the last chunk is ragged
  F acc = F::zero();
  csr_lane_products<F>(m, x, start, cnt, [&](u32, const F& prod) { acc = F::add(acc, prod); });
  acc = csr_sum_lanes<F, POLY_THREADS>(lds, acc);
  if (tid == 0) acc.store(partials + (size_t)blockIdx.x * F::BYTES);
}

template <class F>
__global__ void __launch_bounds__(POLY_THREADS) csr_fold_kernel(CsrView m, const char* partials, char* y) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  __shared__ u32 lds[F::N][POLY_THREADS];
  const u32 tid = threadIdx.x;
  const u32 row = m.lrow[3 * (size_t)blockIdx.x], first = m.lrow[3 * (size_t)blockIdx.x + 1], n = m.lrow[3 * (size_t)blockIdx.x + 2];
  F acc = F::zero();
  for (u32 i = tid; i < n; i += POLY_THREADS) acc = F::add(acc, F::load(partials + ((size_t)first + i) * F::BYTES));
  acc = csr_sum_lanes<F, POLY_THREADS>(lds, acc);
  if (tid == 0) acc.store(y + (size_t)row * F::BYTES);
}

template <class F>
int csr_stream_launch(const CsrView& m, const void* x, void* y, hipStream_t s) {
  if (m.n_stream == 0) return 0;
  if (m.n_stream > 0x7fffffffu) return -1000;
  hipLaunchKernelGGL((csr_stream_kernel<F>), dim3((unsigned)m.n_stream), dim3(POLY_THREADS), 0, s, m, (const char*)x, (char*)y);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
// partials: room for m.n_chunk elements, all of them written by the first launch before the second reads them
template <class F>
int csr_long_launch(const CsrView& m, const void* x, void* partials, void* y, hipStream_t s) {
  if (m.n_lrow == 0) return 0;
  if (m.n_chunk > 0x7fffffffu) return -1000;
  hipLaunchKernelGGL((csr_chunk_kernel<F>), dim3((unsigned)m.n_chunk), dim3(POLY_THREADS), 0, s, m, (const char*)x, (char*)partials);
  if (hipGetLastError() != hipSuccess) return -1000;
  hipLaunchKernelGGL((csr_fold_kernel<F>), dim3((unsigned)m.n_lrow), dim3(POLY_THREADS), 0, s, m, (const char*)partials, (char*)y);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace arkhip
