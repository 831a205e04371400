// Grand products on device-resident tables of Fr, in section 12's conventions (index bit 0 is the first
// variable, canonical Montgomery residues):
//   prod_tree_kernel    W consecutive levels of the binary product tree over a table, in one launch;
//   fr_lincomb_kernel   out[i] = c0 + sum_k c_k T_k[i], the fingerprints that are a grand product's leaves, in one pass.
// No LDS, no barrier, no cross-lane traffic, no atomics, no scratch buffer.
//
// The tree pairs over the LAST variable: L_k[i] = L_{k+1}[i] L_{k+1}[i + 2^k] for i < 2^k, so the two factors of a level are
// the two contiguous halves of the level above, and L_k(r) = sum_x eq(r, x) L_{k+1}(x, 0) L_{k+1}(x, 1) is a sumcheck over
// two views.  The levels lie one after the other in the layout of the opening quotients (mle_open.cuh): L_k at element
// 2^nu - 2^(k+1) of the 2^nu - 1, the product last.
//
// prod_tree_kernel<F, W>.  The source is the 2^m elements of L_m.  A lane owns output index o < 2^(m-W) and loads the 2^W
// elements src[o + t 2^(m-W)]: the lanes of a wave read 2^W runs of contiguous 2 KiB.  These are exactly the elements below
// L_(m-W)[o], and pairing over the top index bit is pairing register t with register t + 2^(W-1), then t with t + 2^(W-2), ...:
// every level is formed between the lane's own registers and stored at o + t 2^(m-W) of its level, again 2 KiB per wave and
// instruction.  2^W - 1 products per 2^W elements read, the number the tree has.  A later launch reads the level the one before
// it wrote in the tree buffer itself.  A wave takes 64 consecutive output indices.  A loop over several such chunks per wave
// (section 12's grouping) was measured level at 2^20 and 2^22 and slower at 2^24 -- the kernel has no per-wave setup to spread --
// and was taken out.
#pragma once
#include "mle.cuh"

namespace arkhip {

// levels per launch: 2^3 elements = 64 VGPRs of data per lane.  Builds of 1, 2 and 3 were measured: 3 and 2 are level at 2^22
// and 2^24, 2 is about 5 us faster at 2^20, 1 is slower everywhere
constexpr int PROD_TREE_MAX_W = 3;
constexpr int PROD_TREE_MAX_LAUNCHES = 64 / PROD_TREE_MAX_W + 1;

// the levels each launch forms for a table of nv variables: full launches from the table down, the remainder LAST, where the
// level it reads has 2 or 4 elements (a remainder launch on the table itself would read all of it for one level)
static inline int prod_tree_launches(int nv, int* widths) {
  int launches = 0;
  while (nv > 0) {
    const int w = nv < PROD_TREE_MAX_W ? nv : PROD_TREE_MAX_W;
    if (widths) widths[launches] = w;
    launches++;
    nv -= w;
  }
  return launches;
}
// The plan as the C entry reports it: a table of 58 variables takes 20 launches, so an entry is a RUN of consecutive launches
// of one kernel instantiation -- first the full launches (a multiple of PROD_TREE_MAX_W levels in all), then the one remainder
// launch.  At most two entries.
static inline int prod_tree_plan(int nv, int* widths) {
  int runs = 0;
  if (nv >= PROD_TREE_MAX_W) widths[runs++] = nv - nv % PROD_TREE_MAX_W;
  if (nv % PROD_TREE_MAX_W) widths[runs++] = nv % PROD_TREE_MAX_W;
  return runs;
}

// forms L_(m-1) .. L_(m-W) from the 2^m elements of src = L_m; dst is where L_(m-1) begins, the lower levels follow it.
// src may lie in the same buffer as dst, before it: the launch reads only src and writes only from dst on.
template <class F, int W>
__global__ void __launch_bounds__(64) prod_tree_kernel(const char* __restrict__ src, int m, char* __restrict__ dst) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  static_assert(W >= 1 && W <= 3, "a lane holds 2^W elements");
  constexpr int E = 1 << W;
  const size_t n_out = (size_t)1 << (m - W);
  const size_t n = (size_t)1 << m;
  const size_t o = ((size_t)blockIdx.x << MLE_LANE_LOG) + threadIdx.x;
  if (o >= n_out) return;
  F x[E];
#pragma unroll
  for (int t = 0; t < E; t++) x[t] = F::load(src + (o + (size_t)t * n_out) * F::BYTES);
#pragma unroll
  for (int a = 0; a < W; a++) {
    char* lvl = dst + (n - (n >> a)) * F::BYTES;   // L_(m-1-a): 2^(m-1-a) = (E >> (a+1)) n_out elements
#pragma unroll
    for (int t = 0; t < (E >> (a + 1)); t++) {
      x[t] = F::mul(x[t], x[t + (E >> (a + 1))]);
      x[t].store(lvl + (o + (size_t)t * n_out) * F::BYTES);
    }
  }
}

template <class F, int W>
int prod_tree_launch_one(const void* src, int m, void* dst, hipStream_t s) {
  const size_t waves = m - W > MLE_LANE_LOG ? (size_t)1 << (m - W - MLE_LANE_LOG) : 1;
  if (waves > 0x7fffffffu) return -1000;
  hipLaunchKernelGGL((prod_tree_kernel<F, W>), dim3((unsigned)waves), dim3(64), 0, s, (const char*)src, m, (char*)dst);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
// forms w levels (1 <= w <= min(m, PROD_TREE_MAX_W)) from the 2^m elements of src
template <class F>
int prod_tree_launch(const void* src, int m, int w, void* dst, hipStream_t s) {
  if (w < 1 || w > PROD_TREE_MAX_W || w > m || m > 62) return -1000;
  if (w == 1) return prod_tree_launch_one<F, 1>(src, m, dst, s);
  if (w == 2) return prod_tree_launch_one<F, 2>(src, m, dst, s);
  return prod_tree_launch_one<F, 3>(src, m, dst, s);
}

constexpr int LINCOMB_MAX_TABLES = 8;
// the tables and coefficients of one linear combination, by value in the kernel arguments
struct FrLincomb {
  const char* tab[LINCOMB_MAX_TABLES];
  FrConst coeff[LINCOMB_MAX_TABLES];
  FrConst c0;
  u32 ntables;
  u32 has_c0;
};
// out[i] = c0 + sum_k coeff[k] tab[k][i]; out may be one of the tables: a lane reads element i of every table before it writes
template <class F>
__global__ void __launch_bounds__(256) fr_lincomb_kernel(FrLincomb lc, char* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  F acc = lc.has_c0 ? fr_from_const<F>(lc.c0) : F::zero();
#pragma unroll
  for (int k = 0; k < LINCOMB_MAX_TABLES; k++)
    if ((u32)k < lc.ntables) acc = F::add(acc, F::mul(fr_from_const<F>(lc.coeff[k]), F::load(lc.tab[k] + i * F::BYTES)));
  acc.store(out + i * F::BYTES);
}
template <class F>
int fr_lincomb_launch(const FrLincomb& lc, void* out, size_t n, hipStream_t s) {
  if (n == 0) return 0;
  if (lc.ntables < 1 || lc.ntables > (u32)LINCOMB_MAX_TABLES || (n + 255) / 256 > 0x7fffffffu) return -1000;
  hipLaunchKernelGGL((fr_lincomb_kernel<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lc, (char*)out, n);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace arkhip
