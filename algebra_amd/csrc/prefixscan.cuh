// Prefix scans along device-resident Fr vectors: the accumulator columns of a univariate prover.
//   scan_tile_total_kernel   the total of every tile under a monoid (Fr, *) or (Fr, +);
//   scan_tile_kernel         the inclusive or exclusive scan inside a tile, given the tile's carry-in;
//   ratio_tile_kernel        out[i] = prod_{j < i} num[j] / den[j] inside a tile from the carries of both products and ONE
//                            inverse per tile (the inverse of the denominators' product through the end of the tile).
//
// Reduce-then-scan over the tiles of polyops.cuh (POLY_TILE elements per workgroup, a lane owns POLY_E consecutive elements,
// the element-order and lane-order views exchanged through its padded LDS limb planes): the tile totals are a vector
// POLY_TILE times shorter whose exclusive scan -- the same two kernels -- gives every tile its carry-in.  Order between the
// phases comes from kernel boundaries only: no workgroup ever waits on another.
//
// The ratio: with PN_i, PD_i the exclusive prefix products of num and den, out[i] = PN_i inv0(PD_i).  Inside tile b
// PD_i S_i = CD_(b+1) for the suffix product S_i = prod_{j >= i in the tile} den[j] and the carry CD_(b+1) out of the tile,
// so 1 / PD_i = S_i / CD_(b+1): one inversion per tile (an fr_div launch over the tiles' carries) instead of one per
// element.  That fails exactly in the tile where the running denominator becomes zero; there (a workgroup-uniform branch)
// every lane inverts its own eight prefixes with lane_batch_inverse, which leaves zeros in place.  Tiles after it write zeros.
#pragma once
#include "polyops.cuh"

namespace arkhip {

constexpr int SCAN_OP_PRODUCT = 0, SCAN_OP_SUM = 1, SCAN_OP_RATIO = 2;

struct ScanMul {
  template <class F> ARK_DEV static F id() { return F::one(); }
  template <class F> ARK_DEV static F op(const F& a, const F& b) { return F::mul(a, b); }
};
struct ScanAdd {
  template <class F> ARK_DEV static F id() { return F::zero(); }
  template <class F> ARK_DEV static F op(const F& a, const F& b) { return F::add(a, b); }
};

// poly_tile_load with `fill` instead of zero beyond n (the monoid's identity: the tile's total stays the total of its elements)
template <class F>
ARK_DEV void scan_tile_load(u32 (*lds)[POLY_PLANE], const char* src, size_t base, size_t n, const F& fill, F* x) {
  const u32 tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < POLY_E; k++) {
    const u32 e = (u32)k * POLY_THREADS + tid;
    const size_t gi = base + e;
    F v = fill;
    if (gi < n) v = F::load(src + gi * F::BYTES);
    poly_lds_put<F>(lds, e + (e >> 3), v);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < POLY_E; k++) x[k] = poly_lds_get<F>(lds, tid * (POLY_E + 1) + k);
  __syncthreads();
}
// x[k] = element base + tid * E + k -> dst, element order across the lanes, the tile's elements below n only
template <class F>
ARK_DEV void scan_tile_store(u32 (*lds)[POLY_PLANE], const F* x, char* dst, size_t base, size_t n) {
  const u32 tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < POLY_E; k++) poly_lds_put<F>(lds, tid * (POLY_E + 1) + k, x[k]);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < POLY_E; k++) {
    const u32 e = (u32)k * POLY_THREADS + tid;
    const size_t gi = base + e;
    if (gi < n) poly_lds_get<F>(lds, e + (e >> 3)).store(dst + gi * F::BYTES);
  }
}
// Scan over the lanes' values h (Hillis-Steele, 8 steps): UP == true gives lane t the total of the lanes BELOW it, UP == false
// of the lanes ABOVE it -- the exclusive form, the identity at the open end.  `at` is the first of 2 * POLY_THREADS words of
// every plane the scan may use (ping-pong: the values of a step are still being read from the other half).  Every lane
// must call it; it ends with every lane done reading LDS.
template <class F, class OP, bool UP>
ARK_DEV F scan_lanes_exclusive(u32 (*lds)[POLY_PLANE], u32 at, F h) {
  const u32 tid = threadIdx.x;
  u32 o = at;
  poly_lds_put<F>(lds, o + tid, h);
#pragma unroll
  for (int j = 0; j < POLY_LOG_THREADS; j++) {
    const u32 d = 1u << j;
    __syncthreads();
    if (UP) {
      if (tid >= d) h = OP::template op<F>(poly_lds_get<F>(lds, o + tid - d), h);
    } else {
      if (tid + d < POLY_THREADS) h = OP::template op<F>(h, poly_lds_get<F>(lds, o + tid + d));
    }
    o ^= POLY_THREADS;
    poly_lds_put<F>(lds, o + tid, h);
  }
  __syncthreads();
  F r = OP::template id<F>();
  if (UP) {
    if (tid > 0) r = poly_lds_get<F>(lds, o + tid - 1);
  } else {
    if (tid + 1 < POLY_THREADS) r = poly_lds_get<F>(lds, o + tid + 1);
  }
  __syncthreads();
  return r;
}

// totals[b] = the total of tile b's elements below n
template <class F, class OP>
__global__ void __launch_bounds__(POLY_THREADS) scan_tile_total_kernel(const char* src, size_t n, char* totals) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  __shared__ u32 lds[F::N][POLY_PLANE];
  const u32 tid = threadIdx.x;
  F x[POLY_E];
  scan_tile_load<F>(lds, src, (size_t)blockIdx.x * POLY_TILE, n, OP::template id<F>(), x);
  F h = x[0];
#pragma unroll
  for (int k = 1; k < POLY_E; k++) h = OP::template op<F>(h, x[k]);
  poly_lds_put<F>(lds, tid, h);
#pragma unroll
  for (int j = POLY_LOG_THREADS - 1; j >= 0; j--) {
    const u32 d = 1u << j;
    __syncthreads();
    if (tid < d) {
      h = OP::template op<F>(h, poly_lds_get<F>(lds, tid + d));
      poly_lds_put<F>(lds, tid, h);
    }
  }
  if (tid == 0) h.store(totals + (size_t)blockIdx.x * F::BYTES);
}

// dst[i] = carry (op) the total of the tile's elements up to i (exclusive != 0: before i) for the tile's i < n, where carry =
// carries[b] (the identity when carries == nullptr).  The last tile writes the total through its end to `total` when that is
// not null.  dst may BE src: the tile is read completely before any of it is written, and no other tile reads it.
template <class F, class OP>
__global__ void __launch_bounds__(POLY_THREADS) scan_tile_kernel(const char* src, size_t n, const char* carries, int exclusive,
                                                                 char* dst, char* total) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  __shared__ u32 lds[F::N][POLY_PLANE];
  const u32 tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * POLY_TILE;
  F x[POLY_E];
  scan_tile_load<F>(lds, src, base, n, OP::template id<F>(), x);
  F h = x[0];
#pragma unroll
  for (int k = 1; k < POLY_E; k++) h = OP::template op<F>(h, x[k]);
  F p = scan_lanes_exclusive<F, OP, true>(lds, 0, h);
  if (carries) p = OP::template op<F>(F::load(carries + (size_t)blockIdx.x * F::BYTES), p);
#pragma unroll
  for (int k = 0; k < POLY_E; k++) {
    const F before = p;
    p = OP::template op<F>(p, x[k]);
#pragma unroll
    for (int j = 0; j < F::N; j++) x[k].l[j] = exclusive ? before.l[j] : p.l[j];   // limb by limb: a select of two structs goes through memory
  }
  if (total && blockIdx.x + 1 == gridDim.x && tid == POLY_THREADS - 1) p.store(total);
  scan_tile_store<F>(lds, x, dst, base, n);
}

// out[i] = PN_i inv0(PD_i) for the tile's i < n.  cn[b]: the product of num before tile b (nullptr: one, a vector of a single
// tile); cdi[b]: the product of den THROUGH tile b, icd[b] its inverse (zero for zero).  The last tile writes
// PN_n inv0(PD_n) to `last` when that is not null.  out may BE num or den: both tiles are read completely before any of
// the output is written, and no other tile reads them.
template <class F>
__global__ void __launch_bounds__(POLY_THREADS) ratio_tile_kernel(const char* num, const char* den, size_t n, const char* cn,
                                                                  const char* cdi, const char* icd, char* out, char* last) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  __shared__ u32 lds[F::N][POLY_PLANE];
  const u32 tid = threadIdx.x;
  const size_t b = blockIdx.x, base = b * POLY_TILE;
  const bool is_last = blockIdx.x + 1 == gridDim.x && tid == POLY_THREADS - 1;
  F x[POLY_E];
  // the carry of den INTO the tile and the inverse of its carry OUT of it: the same for every lane
  const F cd_in = b ? F::load(cdi + (b - 1) * F::BYTES) : F::one();
  const F inv_out = F::load(icd + b * F::BYTES);
  if (cd_in.is_zero()) {   // a zero denominator in an earlier tile: inv0(PD_i) = 0 from here on
#pragma unroll
    for (int k = 0; k < POLY_E; k++) {
      const size_t gi = base + (size_t)k * POLY_THREADS + tid;
      if (gi < n) F::zero().store(out + gi * F::BYTES);
    }
    if (last && is_last) F::zero().store(last);
    return;
  }
  // PN: the exclusive prefix products of num, carried in
  scan_tile_load<F>(lds, num, base, n, F::one(), x);
  F h = x[0];
#pragma unroll
  for (int k = 1; k < POLY_E; k++) h = F::mul(h, x[k]);
  F p = scan_lanes_exclusive<F, ScanMul, true>(lds, 0, h);
  if (cn) p = F::mul(F::load(cn + b * F::BYTES), p);
#pragma unroll
  for (int k = 0; k < POLY_E; k++) {
    const F before = p;
    p = F::mul(p, x[k]);
    x[k] = before;
  }
  const F pn_end = p;   // PN at the first element of the next lane
  F d[POLY_E];
  scan_tile_load<F>(lds, den, base, n, F::one(), d);
  h = d[0];
#pragma unroll
  for (int k = 1; k < POLY_E; k++) h = F::mul(h, d[k]);
  if (!inv_out.is_zero()) {
    // 1 / PD_i = S_i / CD_(b+1): the suffix products of den, with the inverse carried in from the top
    F q = F::mul(scan_lanes_exclusive<F, ScanMul, false>(lds, 0, h), inv_out);
    if (last && is_last) F::mul(pn_end, q).store(last);   // q = inv_out here: nothing lies above the last lane
#pragma unroll
    for (int k = POLY_E - 1; k >= 0; k--) {
      q = F::mul(q, d[k]);
      x[k] = F::mul(x[k], q);
    }
  } else {
    // the running denominator becomes zero inside this tile: the prefixes themselves, inverted lane by lane
    F pd = F::mul(scan_lanes_exclusive<F, ScanMul, true>(lds, 0, h), cd_in);
#pragma unroll
    for (int k = 0; k < POLY_E; k++) {
      const F before = pd;
      pd = F::mul(pd, d[k]);
      d[k] = before;
    }
    lane_batch_inverse<F, POLY_E>(
        0, 1, POLY_E, [&](size_t i) { return d[i]; },
        [&](size_t i, const F& zi, bool nonzero) { x[i] = nonzero ? F::mul(x[i], zi) : F::zero(); });
    if (last && is_last) F::zero().store(last);   // PD_n = CD_(b+1) = 0
  }
  scan_tile_store<F>(lds, x, out, base, n);
}

template <class F>
int scan_tile_total_launch(int op, const void* src, size_t n, void* totals, hipStream_t s) {
  if (n == 0) return 0;
  const size_t tiles = (n + POLY_TILE - 1) / POLY_TILE;
  if (op == SCAN_OP_SUM)
    hipLaunchKernelGGL((scan_tile_total_kernel<F, ScanAdd>), dim3((unsigned)tiles), dim3(POLY_THREADS), 0, s, (const char*)src, n,
                       (char*)totals);
  else
    hipLaunchKernelGGL((scan_tile_total_kernel<F, ScanMul>), dim3((unsigned)tiles), dim3(POLY_THREADS), 0, s, (const char*)src, n,
                       (char*)totals);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
template <class F>
int scan_tile_launch(int op, const void* src, size_t n, const void* carries, int exclusive, void* dst, void* total, hipStream_t s) {
  if (n == 0) return 0;
  const size_t tiles = (n + POLY_TILE - 1) / POLY_TILE;
  if (op == SCAN_OP_SUM)
    hipLaunchKernelGGL((scan_tile_kernel<F, ScanAdd>), dim3((unsigned)tiles), dim3(POLY_THREADS), 0, s, (const char*)src, n,
                       (const char*)carries, exclusive, (char*)dst, (char*)total);
  else
    hipLaunchKernelGGL((scan_tile_kernel<F, ScanMul>), dim3((unsigned)tiles), dim3(POLY_THREADS), 0, s, (const char*)src, n,
                       (const char*)carries, exclusive, (char*)dst, (char*)total);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
template <class F>
int ratio_tile_launch(const void* num, const void* den, size_t n, const void* cn, const void* cdi, const void* icd, void* out,
                      void* last, hipStream_t s) {
  if (n == 0) return 0;
  const size_t tiles = (n + POLY_TILE - 1) / POLY_TILE;
  hipLaunchKernelGGL((ratio_tile_kernel<F>), dim3((unsigned)tiles), dim3(POLY_THREADS), 0, s, (const char*)num, (const char*)den, n,
                     (const char*)cn, (const char*)cdi, (const char*)icd, (char*)out, (char*)last);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace arkhip
