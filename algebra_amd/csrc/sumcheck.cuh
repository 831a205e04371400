// The sumcheck prover's round on device-resident tables of Fr: for ntables <= 8 multilinear tables T_k of
// 2^m elements and nterms <= 8 terms c_j prod_{k in term j} f_k (1 to 4 factors, repeats allowed), the D + 1 elements
//   evals[t] = sum_{b < 2^(m-1)} sum_j c_j prod_{k in term j} ( T_k[2b] + t (T_k[2b+1] - T_k[2b]) ),   t = 0 .. D,
// D the longest term.  Index bit 0 is the first variable, as in mle.cuh.  The shape of the sum is ListOfProductsOfPolynomials
// of ark-linear-sumcheck; that crate is outside the reference's own, the table conventions are dense.rs:224-257.
//   sumcheck_round_kernel<F, NT, false>  the round sums of the tables as they are;
//   sumcheck_round_kernel<F, NT, true>   first binds the previous challenge r: reads T_k four consecutive elements at a time,
//                                        writes T'_k[i] = T_k[2i] + r (T_k[2i+1] - T_k[2i]) and sums over T' -- a round reads
//                                        every table once;
//   sumcheck_fold_kernel                 adds the workgroups' partial sums: the second stage of the reduction.
// NT is the number of tables the lane holds in registers, 4 or 8.
//
// A lane walks its grid-strided pairs b.  Of a pair it keeps, per table, the row's value at t = 0 and the difference of its two
// elements; a term picks its factors from them (the term structure arrives by value in the kernel's arguments and every loop
// over terms and factors is wave-uniform), folds c_j into its first factor unless c_j is one, and walks t = 0 .. D: the product
// of the factors goes to the accumulator of t, then every factor moves on by one ADDITION of its difference.  The loop over t
// is rolled -- its body holds the only products of the term -- and the five accumulators rotate through it by one place per
// step, so each is addressed by a fixed register.
//
// Products per pair: sum_j ((len_j - 1) (D + 1) + (c_j != 1 ? 2 : 0)), and 2 per table when the challenge is bound first.
// The reduction is exact (field addition is associative): lanes -> workgroup through LDS -> one partial per workgroup and t
// in Context::poly_work -> sumcheck_fold_kernel.  No field atomics, no workgroup waits on another.
#pragma once
#include "mle.cuh"

namespace arkhip {

constexpr int SUMCHECK_MAX_TABLES = 8;
constexpr int SUMCHECK_MAX_TERMS = 8;
constexpr int SUMCHECK_MAX_DEGREE = 4;
constexpr int SUMCHECK_EVALS = SUMCHECK_MAX_DEGREE + 1;
constexpr int SUMCHECK_THREADS = 256;
constexpr int SUMCHECK_BLOCKS = 1024;   // the grid's cap: four workgroups per compute unit of an MI355X

// the terms of one round, by value
struct SumcheckTerms {
  u32 ntables, nterms, degree;
  u32 unit;                            // bit j: c_j is one and costs no product
  u32 len[SUMCHECK_MAX_TERMS];
  u32 tab[SUMCHECK_MAX_TERMS];         // the table of factor q of term j in bits 8q .. 8q+7
  FrConst coeff[SUMCHECK_MAX_TERMS];
  FrConst r;                           // the challenge the fused round binds first
};
struct SumcheckTables {
  const char* src[SUMCHECK_MAX_TABLES];
  char* dst[SUMCHECK_MAX_TABLES];      // the bound tables (fused round only)
};
// one round as the host hands it to a field's translation unit
struct SumcheckRound {
  SumcheckTables tb;
  SumcheckTerms tm;
  size_t npairs;     // pairs of rows summed: 2^(m-1); 1 when m = 0
  int fused;         // bind tm.r first
  int last;          // m = 0: the bound tables have one element, evals[0] is the sum's value there and evals[1 .. D] are zero
  unsigned blocks;
  void* partials;    // blocks * SUMCHECK_EVALS elements (blocks > 1)
  void* out;         // SUMCHECK_EVALS elements
};

// launch geometry of a round over 2^m-element tables: the workgroups and the pairs one lane walks
static inline void sumcheck_geometry(int m, unsigned* blocks, size_t* pairs_per_lane) {
  const size_t npairs = m >= 1 ? (size_t)1 << (m - 1) : 1;
  size_t b = (npairs + SUMCHECK_THREADS - 1) / SUMCHECK_THREADS;
  if (b > (size_t)SUMCHECK_BLOCKS) b = SUMCHECK_BLOCKS;
  *blocks = (unsigned)b;
  *pairs_per_lane = (npairs + b * SUMCHECK_THREADS - 1) / (b * SUMCHECK_THREADS);
}

// v[idx] for a wave-uniform idx without a runtime-indexed register array
template <class F, int NT>
ARK_DEV F sumcheck_pick(const F (&v)[NT], u32 idx) {
  F r = v[0];
#pragma unroll
  for (int k = 1; k < NT; k++) r = mle_pick<F>(idx == (u32)k, v[k], r);
  return r;
}
// the sum of the workgroup's 256 values in lane 0 (the tree of fr_inner_product_kernel); lds may be reused after the call
template <class F>
ARK_DEV F sumcheck_block_sum(F acc, u32 (*lds)[SUMCHECK_THREADS]) {
  const u32 tid = threadIdx.x;
  __syncthreads();   // the previous use of lds is over
#pragma unroll
  for (int j = 0; j < F::N; j++) lds[j][tid] = acc.l[j];
  for (u32 d = SUMCHECK_THREADS / 2; d >= 1; d >>= 1) {
    __syncthreads();
    if (tid < d) {
      F o;
#pragma unroll
      for (int j = 0; j < F::N; j++) o.l[j] = lds[j][tid + d];
      acc = F::add(acc, o);
#pragma unroll
      for (int j = 0; j < F::N; j++) lds[j][tid] = acc.l[j];
    }
  }
  return acc;
}

// out: SUMCHECK_EVALS elements per workgroup, [blockIdx.x][t]
template <class F, int NT, bool FUSED>
__global__ void __launch_bounds__(SUMCHECK_THREADS) sumcheck_round_kernel(SumcheckTables tb, SumcheckTerms tm, size_t npairs, int last,
                                                                          char* out) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  static_assert(NT == 4 || NT == 8, "tables a lane holds");
  __shared__ u32 lds[F::N][SUMCHECK_THREADS];
  const size_t stride = (size_t)gridDim.x * SUMCHECK_THREADS;
  const u32 degree = tm.degree;
  F a0 = F::zero(), a1 = F::zero(), a2 = F::zero(), a3 = F::zero(), a4 = F::zero();
  const F r = fr_from_const<F>(tm.r);
  // eight input and eight output pointers, the challenge, a coefficient and the modulus do not fit the scalar registers:
  // the eight-table fused round reads its output pointers from LDS where it stores
  __shared__ char* dst_lds[FUSED && NT == 8 ? NT : 1];
  if (FUSED && NT == 8) {
    if (threadIdx.x < (u32)NT) dst_lds[threadIdx.x] = tb.dst[threadIdx.x];
    __syncthreads();
  }
  for (size_t p = (size_t)blockIdx.x * SUMCHECK_THREADS + threadIdx.x; p < npairs; p += stride) {
    F lo[NT], df[NT];
#pragma unroll
    for (int k = 0; k < NT; k++) {
      lo[k] = F::zero();
      df[k] = F::zero();
      if ((u32)k < tm.ntables) {
        if (FUSED) {
          const char* s = tb.src[k] + p * (4 * F::BYTES);
          char* d = (NT == 8 ? dst_lds[k] : tb.dst[k]) + p * (last ? F::BYTES : 2 * F::BYTES);
          lo[k] = mle_bind<F>(F::load(s), F::load(s + F::BYTES), r);
          lo[k].store(d);
          if (!last) {
            const F hi = mle_bind<F>(F::load(s + 2 * F::BYTES), F::load(s + 3 * F::BYTES), r);
            hi.store(d + F::BYTES);
            df[k] = F::sub(hi, lo[k]);
          }
        } else {
          const char* s = tb.src[k] + p * (2 * F::BYTES);
          lo[k] = F::load(s);
          df[k] = F::sub(F::load(s + F::BYTES), lo[k]);
        }
      }
    }
#pragma unroll 1
    for (u32 j = 0; j < tm.nterms; j++) {
      const u32 len = tm.len[j], tabs = tm.tab[j];
      F fv[SUMCHECK_MAX_DEGREE], fd[SUMCHECK_MAX_DEGREE];
#pragma unroll
      for (int q = 0; q < SUMCHECK_MAX_DEGREE; q++) {
        const u32 idx = (u32)q < len ? (tabs >> (8 * q)) & 0xffu : 0u;
        fv[q] = sumcheck_pick<F, NT>(lo, idx);
        fd[q] = sumcheck_pick<F, NT>(df, idx);
      }
      if (!((tm.unit >> j) & 1u)) {
        const F c = fr_from_const<F>(tm.coeff[j]);
        fv[0] = F::mul(c, fv[0]);
        fd[0] = F::mul(c, fd[0]);
      }
#pragma unroll 1
      for (u32 t = 0; t < (u32)SUMCHECK_EVALS; t++) {
        F sum = a0;
        if (t <= degree) {
          F pr = fv[0];
#pragma unroll
          for (int q = 1; q < SUMCHECK_MAX_DEGREE; q++)
            if ((u32)q < len) pr = F::mul(pr, fv[q]);
          sum = F::add(sum, pr);
        }
        if (t < degree) {
#pragma unroll
          for (int q = 0; q < SUMCHECK_MAX_DEGREE; q++)
            if ((u32)q < len) fv[q] = F::add(fv[q], fd[q]);
        }
        // the accumulator of t is a0 in step t: after the five steps every one is back in its place
        a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = sum;
      }
    }
  }
  const F acc[SUMCHECK_EVALS] = {a0, a1, a2, a3, a4};
#pragma unroll
  for (int t = 0; t < SUMCHECK_EVALS; t++) {
    F s = F::zero();
    if ((u32)t <= degree && !(last && t > 0)) s = sumcheck_block_sum<F>(acc[t], lds);   // uniform: every lane takes the same side
    if (threadIdx.x == 0) s.store(out + ((size_t)blockIdx.x * SUMCHECK_EVALS + t) * F::BYTES);
  }
}

// out[t] = sum_b partials[b][t], one workgroup
template <class F>
__global__ void __launch_bounds__(SUMCHECK_THREADS) sumcheck_fold_kernel(const char* partials, u32 blocks, char* out) {
  __shared__ u32 lds[F::N][SUMCHECK_THREADS];
#pragma unroll 1
  for (int t = 0; t < SUMCHECK_EVALS; t++) {
    F acc = F::zero();
    for (u32 b = threadIdx.x; b < blocks; b += SUMCHECK_THREADS)
      acc = F::add(acc, F::load(partials + ((size_t)b * SUMCHECK_EVALS + t) * F::BYTES));
    acc = sumcheck_block_sum<F>(acc, lds);
    if (threadIdx.x == 0) acc.store(out + (size_t)t * F::BYTES);
  }
}

template <class F, int NT, bool FUSED>
int sumcheck_round_launch_one(const SumcheckRound& rd, hipStream_t s) {
  char* first = (char*)(rd.blocks == 1 ? rd.out : rd.partials);
  hipLaunchKernelGGL((sumcheck_round_kernel<F, NT, FUSED>), dim3(rd.blocks), dim3(SUMCHECK_THREADS), 0, s, rd.tb, rd.tm, rd.npairs,
                     rd.last, first);
  if (hipGetLastError() != hipSuccess) return -1000;
  if (rd.blocks > 1)
    hipLaunchKernelGGL((sumcheck_fold_kernel<F>), dim3(1), dim3(SUMCHECK_THREADS), 0, s, (const char*)rd.partials, rd.blocks,
                       (char*)rd.out);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
template <class F>
int sumcheck_round_launch(const SumcheckRound& rd, hipStream_t s) {
  if (rd.blocks == 0 || rd.blocks > (unsigned)SUMCHECK_BLOCKS || rd.npairs == 0 || rd.tm.ntables > (u32)SUMCHECK_MAX_TABLES) return -1000;
  if (rd.last && (!rd.fused || rd.npairs != 1)) return -1000;
  const bool small = rd.tm.ntables <= 4;
  if (rd.fused) return small ? sumcheck_round_launch_one<F, 4, true>(rd, s) : sumcheck_round_launch_one<F, 8, true>(rd, s);
  return small ? sumcheck_round_launch_one<F, 4, false>(rd, s) : sumcheck_round_launch_one<F, 8, false>(rd, s);
}

}  // namespace arkhip
