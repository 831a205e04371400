// Fractional sums on device-resident tables of Fr, in section 12's conventions (index bit 0 is the first
// variable, canonical Montgomery residues) and section 19's tree layout:
//   frac_tree_kernel    W consecutive levels of the binary tree that adds fractions (N, D), both trees in one launch;
//   fr_count_*_kernel   the multiplicity table m[j] = #{i : indices[i] = j} of a lookup, built in place in its output.
// No LDS, no barrier, no cross-lane traffic, no scratch buffer.  The only atomics are the counts' global atomicAdd.
//
// The tree pairs over the LAST variable, as the product tree does:
//   N_k[i] = N_{k+1}[i] D_{k+1}[i + 2^k] + N_{k+1}[i + 2^k] D_{k+1}[i],   D_k[i] = D_{k+1}[i] D_{k+1}[i + 2^k],   i < 2^k,
// so N_0[0] / D_0[0] = sum_b N_nu[b] / D_nu[b] without an inversion anywhere; a zero denominator is just a value.  Each tree
// has the layout of the product tree (grand_product.cuh): L_k at element 2^nu - 2^(k+1) of the 2^nu - 1, the root last.
//
// frac_tree_kernel<F, W, HAS_NUM> is prod_tree_kernel's scheme on two sources.  A lane owns output index o < 2^(m-W) and loads
// the 2^W elements src[o + t 2^(m-W)] of both sources -- the lanes of a wave read runs of contiguous 2 KiB -- pairs register t
// with t + 2^(W-1), then with t + 2^(W-2), ..., and stores every level of both trees at o + t 2^(m-W) of its level.  A pair
// costs one product for D and ONE sum of two products under one Montgomery reduction for N (Fp::sop2: operands below p give
// (2 p^2 + m p) / R < 2p, one conditional subtraction makes the canonical residue), so 3 (2^W - 1) limb products and
// 2 (2^W - 1) reductions per 2^(W+1) elements read.  HAS_NUM = false is the first launch of a sum whose numerators are all
// one (the witness side of a lookup): no numerator is read and the first level is N = D[i] + D[i + h], D = D[i] D[i + h].
#pragma once
#include "grand_product.cuh"

namespace arkhip {

// levels per launch: a lane holds 2^(W+1) elements, 128 VGPRs of data at W = 3 (144 allocated, 3 waves per SIMD) against 64
// at W = 2 (93, 5 waves).  Builds of 1, 2 and 3 were timed in one session (tools/bench_fraction_sum.py): at 2^24 with
// numerators 2 and 3 are level within their spreads (0.593 / 0.590 ms) and 1 is slower (0.675); with ones 2 is fastest
// (0.461 against 0.532 and 0.549); 2 is also fastest at 2^20 and 2^22.  2 ships.
// -DARK_FRAC_TREE_W=1|2|3 on capi_poly.hip and field_unit.hip builds the variants.
#ifdef ARK_FRAC_TREE_W
constexpr int FRAC_TREE_MAX_W = ARK_FRAC_TREE_W;
constexpr bool FRAC_TREE_VARIANT_BUILD = true;
#else
constexpr int FRAC_TREE_MAX_W = 2;
constexpr bool FRAC_TREE_VARIANT_BUILD = false;
#endif
static_assert(FRAC_TREE_MAX_W >= 1 && FRAC_TREE_MAX_W <= 3, "kernels are built for 1, 2 and 3 levels");
constexpr int FRAC_TREE_MAX_LAUNCHES = 64 / FRAC_TREE_MAX_W + 1;

// the levels each launch forms for tables of nv variables: full launches from the tables down, the remainder LAST
static inline int frac_tree_launches(int nv, int* widths) {
  int launches = 0;
  while (nv > 0) {
    const int w = nv < FRAC_TREE_MAX_W ? nv : FRAC_TREE_MAX_W;
    if (widths) widths[launches] = w;
    launches++;
    nv -= w;
  }
  return launches;
}
// the plan as the C entry reports it, as prod_tree_plan: the full launches as one run, then the one remainder launch
static inline int frac_tree_plan(int nv, int* widths) {
  int runs = 0;
  if (nv >= FRAC_TREE_MAX_W) widths[runs++] = nv - nv % FRAC_TREE_MAX_W;
  if (nv % FRAC_TREE_MAX_W) widths[runs++] = nv % FRAC_TREE_MAX_W;
  return runs;
}

// forms levels m-1 .. m-W of both trees from the 2^m elements of nsrc = N_m (not read when !HAS_NUM: all ones) and
// dsrc = D_m; ndst / ddst are where N_(m-1) / D_(m-1) begin, the lower levels follow them.  A source may lie in the same
// buffer as its destination, before it: the launch reads only the sources and writes only from the destinations on.
template <class F, int W, bool HAS_NUM>
__global__ void __launch_bounds__(64) frac_tree_kernel(const char* __restrict__ nsrc, const char* __restrict__ dsrc, int m,
                                                       char* __restrict__ ndst, char* __restrict__ ddst) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  static_assert(W >= 1 && W <= 3, "a lane holds 2^(W+1) elements");
  constexpr int E = 1 << W;
  const size_t n_out = (size_t)1 << (m - W);
  const size_t n = (size_t)1 << m;
  const size_t o = ((size_t)blockIdx.x << MLE_LANE_LOG) + threadIdx.x;
  if (o >= n_out) return;
  F d[E], u[E];
#pragma unroll
  for (int t = 0; t < E; t++) {
    d[t] = F::load(dsrc + (o + (size_t)t * n_out) * F::BYTES);
    if constexpr (HAS_NUM) u[t] = F::load(nsrc + (o + (size_t)t * n_out) * F::BYTES);
  }
#pragma unroll
  for (int a = 0; a < W; a++) {
    const size_t off = (n - (n >> a)) * F::BYTES;   // level m-1-a: 2^(m-1-a) = (E >> (a+1)) n_out elements
#pragma unroll
    for (int t = 0; t < (E >> (a + 1)); t++) {
      const int h = E >> (a + 1);
      if (!HAS_NUM && a == 0) u[t] = F::add(d[t], d[t + h]);
      else u[t] = F::sop2(u[t], d[t + h], u[t + h], d[t]);
      d[t] = F::mul(d[t], d[t + h]);
      u[t].store(ndst + off + (o + (size_t)t * n_out) * F::BYTES);
      d[t].store(ddst + off + (o + (size_t)t * n_out) * F::BYTES);
    }
  }
}

template <class F, int W, bool HAS_NUM>
int frac_tree_launch_one(const void* nsrc, const void* dsrc, int m, void* ndst, void* ddst, hipStream_t s) {
  const size_t waves = m - W > MLE_LANE_LOG ? (size_t)1 << (m - W - MLE_LANE_LOG) : 1;
  if (waves > 0x7fffffffu) return -1000;
  hipLaunchKernelGGL((frac_tree_kernel<F, W, HAS_NUM>), dim3((unsigned)waves), dim3(64), 0, s, (const char*)nsrc, (const char*)dsrc,
                     m, (char*)ndst, (char*)ddst);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
template <class F, bool HAS_NUM>
int frac_tree_launch_w(const void* nsrc, const void* dsrc, int m, int w, void* ndst, void* ddst, hipStream_t s) {
  if (w == 1) return frac_tree_launch_one<F, 1, HAS_NUM>(nsrc, dsrc, m, ndst, ddst, s);
  if constexpr (FRAC_TREE_MAX_W >= 2)
    if (w == 2) return frac_tree_launch_one<F, 2, HAS_NUM>(nsrc, dsrc, m, ndst, ddst, s);
  if constexpr (FRAC_TREE_MAX_W >= 3)
    if (w == 3) return frac_tree_launch_one<F, 3, HAS_NUM>(nsrc, dsrc, m, ndst, ddst, s);
  return -1000;
}
// forms w levels (1 <= w <= min(m, FRAC_TREE_MAX_W)) of both trees from the 2^m elements of the sources; nsrc == nullptr: ones
template <class F>
int frac_tree_launch(const void* nsrc, const void* dsrc, int m, int w, void* ndst, void* ddst, hipStream_t s) {
  if (w < 1 || w > FRAC_TREE_MAX_W || w > m || m > 62) return -1000;
  return nsrc ? frac_tree_launch_w<F, true>(nsrc, dsrc, m, w, ndst, ddst, s) : frac_tree_launch_w<F, false>(nullptr, dsrc, m, w, ndst, ddst, s);
}

// ---- the multiplicity table ---------------------------------------------------------------------------------------------
// Three launches on one stream, the output its own workspace: clear the cells; count into the first 32-bit word of cell
// indices[i] with a global atomicAdd (n < 2^32: a count fits the word); turn every cell's count c into the Montgomery residue
// c R mod p -- one Montgomery product by R^2 mod p -- and rewrite the whole cell.
template <class F>
__global__ void __launch_bounds__(256) fr_count_clear_kernel(char* out, size_t table_len) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= table_len) return;
  F::zero().store(out + j * F::BYTES);
}
// an index >= table_len is skipped
template <class F>
__global__ void __launch_bounds__(256) fr_count_add_kernel(const u32* __restrict__ indices, size_t n, char* out, size_t table_len) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t j = indices[i];
  if (j >= table_len) return;
  atomicAdd((unsigned int*)(out + j * F::BYTES), 1u);
}
template <class F>
__global__ void __launch_bounds__(256) fr_count_mont_kernel(char* out, size_t table_len) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= table_len) return;
  F c = F::zero();
  c.l[0] = *(const u32*)(out + j * F::BYTES);
  F::to_mont(c).store(out + j * F::BYTES);
}
template <class F>
int fr_count_launch(const void* indices, size_t n, void* out, size_t table_len, hipStream_t s) {
  const size_t cells = (table_len + 255) / 256, items = (n + 255) / 256;
  if (table_len == 0 || cells > 0x7fffffffu || items > 0x7fffffffu) return -1000;
  hipLaunchKernelGGL((fr_count_clear_kernel<F>), dim3((unsigned)cells), dim3(256), 0, s, (char*)out, table_len);
  if (n) hipLaunchKernelGGL((fr_count_add_kernel<F>), dim3((unsigned)items), dim3(256), 0, s, (const u32*)indices, n, (char*)out, table_len);
  hipLaunchKernelGGL((fr_count_mont_kernel<F>), dim3((unsigned)cells), dim3(256), 0, s, (char*)out, table_len);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace arkhip
