// Gate expressions on device vectors: for ncolumns <= 16 vectors of n elements of Fr and nterms <= 16
// terms of 1 to 8 factors, each factor a column read at a rotation,
//   out[i] = c0 + sum_j c_j prod_q col[ tc_{j,q} ][ (i + rot_{j,q}) mod n ],   0 <= i < n
// -- the row-by-row constraint expression of a univariate (Plonk-style) prover over a domain or an extended coset, where "the
// next row" of a coset of blow-up k is k indices on.  The univariate counterpart of the sumcheck round's list of products
// (sumcheck.cuh): the same term structure with a rotation per factor, and a vector where the round produces sums.
//
// One lane per row, grid-strided under GATE_BLOCKS workgroups.  The term structure arrives by value in the kernel's arguments
// and every loop over terms and factors is wave-uniform and rolled: the code holds one product and one load.  A factor is
// loaded where it is used, from a wave-uniform base pointer at (i + rot) with one conditional subtraction of n -- the host has
// reduced rot to [0, n) -- so a wave reads 2 KiB of contiguous memory per factor, but for the one wave that straddles the
// wrap.  Nothing is kept between factors: a (column, rotation) read twice is read twice, the second time from the caches.
// Holding the columns in registers and picking with compare-and-select chains, as the sumcheck round does with its 8 tables,
// costs at 16 columns about what the product it feeds costs.
//
// A coefficient equal to one costs no product; any other folds into the term's first factor.  Without c0 the first term
// starts the sum, so one unit term of one factor is a load and a store: the rotated copy.
// No scratch buffer, no atomics, no LDS.  out may be a column that is read at rotation 0 only: a lane reads row i of every
// factor before it writes row i, and no other lane touches that row.
#pragma once
#include "devops.cuh"
#include "polyops.cuh"

namespace arkhip {

constexpr int GATE_MAX_COLUMNS = 16;
constexpr int GATE_MAX_TERMS = 16;
constexpr int GATE_MAX_DEGREE = 8;
constexpr int GATE_THREADS = 256;
constexpr int GATE_BLOCKS = 2048;   // the grid's cap: eight workgroups per compute unit of an MI355X, every wave slot at <= 64 VGPRs

// the expression, by value
struct GateTerms {
  const char* col[GATE_MAX_COLUMNS];
  unsigned long long rot[GATE_MAX_TERMS][GATE_MAX_DEGREE];   // reduced to [0, n)
  FrConst coeff[GATE_MAX_TERMS];
  FrConst c0;
  u32 len[GATE_MAX_TERMS];
  u32 tab[GATE_MAX_TERMS];    // the column of factor q of term j in bits 4q .. 4q+3
  u32 nterms;
  u32 unit;                   // bit j: c_j is one and costs no product
  u32 has_c0;
};

// launch geometry for n rows: the workgroups and the rows one lane walks (1 until the cap is reached)
static inline void gate_geometry(size_t n, unsigned* blocks, size_t* rows_per_lane) {
  size_t b = (n + GATE_THREADS - 1) / GATE_THREADS;
  if (b > (size_t)GATE_BLOCKS) b = GATE_BLOCKS;
  *blocks = (unsigned)b;
  *rows_per_lane = b ? (n + b * GATE_THREADS - 1) / (b * GATE_THREADS) : 0;
}

template <class F>
__global__ void __launch_bounds__(GATE_THREADS) gate_sum_of_products_kernel(GateTerms tm, char* out, size_t n) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  const size_t stride = (size_t)gridDim.x * GATE_THREADS;
  for (size_t i = (size_t)blockIdx.x * GATE_THREADS + threadIdx.x; i < n; i += stride) {
    F acc = fr_from_const<F>(tm.c0);
#pragma unroll 1
    for (u32 j = 0; j < tm.nterms; j++) {
      const u32 len = tm.len[j], tabs = tm.tab[j];
      const bool unit = (tm.unit >> j) & 1u;
      F pr = fr_from_const<F>(tm.coeff[j]);
#pragma unroll 1
      for (u32 q = 0; q < len; q++) {
        size_t at = i + (size_t)tm.rot[j][q];
        if (at >= n) at -= n;
        const F x = F::load(tm.col[(tabs >> (4 * q)) & 0xfu] + at * F::BYTES);
        if (q == 0 && unit) pr = x;
        else pr = F::mul(pr, x);
      }
      if (j == 0 && !tm.has_c0) acc = pr;
      else acc = F::add(acc, pr);
    }
    acc.store(out + i * F::BYTES);
  }
}

template <class F>
int gate_sum_of_products_launch(const GateTerms& tm, void* out, size_t n, hipStream_t s) {
  if (n == 0) return 0;
  if (tm.nterms < 1 || tm.nterms > (u32)GATE_MAX_TERMS) return -1000;
  unsigned blocks;
  size_t rpl;
  gate_geometry(n, &blocks, &rpl);
  hipLaunchKernelGGL((gate_sum_of_products_kernel<F>), dim3(blocks), dim3(GATE_THREADS), 0, s, tm, (char*)out, n);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace arkhip
