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
// The whole proof in one wait (section 23; sumcheck_prove_run) queues, with the challenges derived on the device (transcript.cuh):
//   sumcheck_round_kernel<F, NT, true, true>  the fused round with r read from a device cell;
//   sumcheck_challenge_kernel            one lane hashes a round's sums: proof buffer, new state, the cell, the point;
//   sumcheck_tail_kernel<F, NT>          every remaining round in one workgroup once the tables are small;
//   sumcheck_finals_kernel               gathers the one-element tables and the value when there is no tail.
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
#include "transcript.cuh"

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
  union {
    FrConst r;                         // the challenge the fused round binds first
    const char* r_cell;                // ... or the device cell that holds it (sumcheck_round_kernel<.., CELL>)
  };
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

// one pair's terms: with the tables' values at t = 0 (lo) and their differences (df), adds every term's value at t = 0 .. D
// to the accumulator of t.  The tail's copy of the walk inside sumcheck_round_kernel, which keeps its own text so that its
// instantiations compile to what profiles/sumcheck_resources.txt records.
template <class F, int NT>
ARK_DEV void sumcheck_pair_terms(const F (&lo)[NT], const F (&df)[NT], const SumcheckTerms& tm, F& a0, F& a1, F& a2, F& a3, F& a4) {
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
      if (t <= tm.degree) {
        F pr = fv[0];
#pragma unroll
        for (int q = 1; q < SUMCHECK_MAX_DEGREE; q++)
          if ((u32)q < len) pr = F::mul(pr, fv[q]);
        sum = F::add(sum, pr);
      }
      if (t < tm.degree) {
#pragma unroll
        for (int q = 0; q < SUMCHECK_MAX_DEGREE; q++)
          if ((u32)q < len) fv[q] = F::add(fv[q], fd[q]);
      }
      // the accumulator of t is a0 in step t: after the five steps every one is back in its place
      a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = sum;
    }
  }
}

// out: SUMCHECK_EVALS elements per workgroup, [blockIdx.x][t]
// CELL: the challenge the fused round binds is read from a device cell (the whole proof of sumcheck_prove_run), not from tm.r
template <class F, int NT, bool FUSED, bool CELL = false>
__global__ void __launch_bounds__(SUMCHECK_THREADS) sumcheck_round_kernel(SumcheckTables tb, SumcheckTerms tm, size_t npairs, int last,
                                                                          char* out) {
  static_assert(FUSED || !CELL, "only a fused round binds a challenge");
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  static_assert(NT == 4 || NT == 8, "tables a lane holds");
  __shared__ u32 lds[F::N][SUMCHECK_THREADS];
  const size_t stride = (size_t)gridDim.x * SUMCHECK_THREADS;
  const u32 degree = tm.degree;
  F a0 = F::zero(), a1 = F::zero(), a2 = F::zero(), a3 = F::zero(), a4 = F::zero();
  const F r = CELL ? F::load(tm.r_cell) : fr_from_const<F>(tm.r);
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

// ---- the whole proof in one wait ----------------------------------------------------------------
constexpr int SUMCHECK_TAIL_MAX_VARS = 14;       // ARK_HIP_SUMCHECK_TAIL_MAX_VARS
constexpr int SUMCHECK_TAIL_DEFAULT_VARS = 10;   // the fastest of the sweep in profiles/sumcheck_device.json
constexpr int SUMCHECK_MSG_WORDS = TRANSCRIPT_HEAD_WORDS + 8 * SUMCHECK_EVALS;

struct TranscriptState { u32 w[TRANSCRIPT_STATE_WORDS]; };
// the proof as the host hands it to a field's translation unit; every device pointer but the tables lies in Context::poly_work
struct SumcheckProve {
  SumcheckTerms tm;
  const char* src[SUMCHECK_MAX_TABLES];       // the caller's tables: never written
  char* set[2][SUMCHECK_MAX_TABLES];          // d_work: the halves and the quarters the bound tables alternate between
  unsigned num_vars;
  int tail_from;                              // 0: no tail
  TranscriptState state0;                     // the caller's state, by value: the first hash starts from it
  void *sums, *partials;                      // SUMCHECK_EVALS elements | SUMCHECK_EVALS per workgroup of the largest round
  void *cell, *state;                         // the challenge | the 32 bytes of state
  void *rounds, *point, *finals, *value;      // num_vars (D + 1) | num_vars | ntables | 1 elements
};
// where the launches of a proof change kind: rounds i < hand (tables of num_vars - i variables) are round kernels + a challenge
// launch each, the tail takes over at round `hand` (its tables have at most tail_from variables); without a tail the last
// bind is the m = 0 round and a gather
static inline int sumcheck_prove_hand(unsigned num_vars, int tail_from) {
  return tail_from <= 0 ? (int)num_vars : ((int)num_vars > tail_from ? (int)num_vars - tail_from : 0);
}
static inline int sumcheck_prove_launches(unsigned num_vars, int tail_from) {
  const int hand = sumcheck_prove_hand(num_vars, tail_from);
  int launches = 0;
  for (int i = 0; i < hand; i++) {
    unsigned b;
    size_t ppl;
    sumcheck_geometry((int)num_vars - i, &b, &ppl);
    launches += (b > 1 ? 2 : 1) + 1;
  }
  return launches + (tail_from <= 0 ? 2 : 1);
}

// One lane: hashes the round's D + 1 sums with the state, writes them to the proof, the new state, the challenge to the cell
// and to the point.  first: the state is state0 (nothing has been hashed on the device yet).
template <class F>
__global__ void __launch_bounds__(64) sumcheck_challenge_kernel(const char* sums, u32 count, TranscriptState state0, int first, char* state,
                                                                 char* round_out, char* cell, char* point_out) {
  __shared__ u32 msg[SUMCHECK_MSG_WORDS];
  if (threadIdx.x != 0) return;
  for (int i = 0; i < TRANSCRIPT_STATE_WORDS; i++) msg[i] = first ? state0.w[i] : ((const u32*)state)[i];
  for (u32 t = 0; t < count; t++) {
    const F s = F::load(sums + (size_t)t * F::BYTES);
    s.store(round_out + (size_t)t * F::BYTES);
    transcript_put_element<F>(msg, t, s);
  }
  const F r = transcript_challenge_words<F>(msg, count);
  for (int i = 0; i < TRANSCRIPT_STATE_WORDS; i++) ((u32*)state)[i] = msg[i];
  r.store(cell);
  r.store(point_out);
}

// lanes k < ntables: finals[k] = the one element of bound table k; lane ntables: value = sums[0]
template <class F>
__global__ void __launch_bounds__(64) sumcheck_finals_kernel(SumcheckTables tb, u32 ntables, const char* sums, char* finals, char* value) {
  const u32 k = threadIdx.x;
  if (k < ntables) F::load(tb.src[k]).store(finals + (size_t)k * F::BYTES);
  if (k == ntables) F::load(sums).store(value);
}

struct SumcheckTailArgs {
  const char* src[SUMCHECK_MAX_TABLES];   // the tables the tail starts from, of m variables (+ 1 when a challenge is pending)
  char* set[2][SUMCHECK_MAX_TABLES];      // set[0] is written first
};
// Every remaining round in one workgroup.  On entry the tables have m variables -- m + 1 and the cell holds the challenge to
// bind first when `pending`.  Per round: lanes sum their pairs, the LDS tree reduces per t, lane 0 hashes and leaves r in LDS;
// then all lanes bind into the other table set in global memory.  Every loop bound is an argument; a workgroup barrier
// orders the set's writes before its reads by the same workgroup; no other workgroup exists.
template <class F, int NT>
__global__ void __launch_bounds__(SUMCHECK_THREADS) sumcheck_tail_kernel(SumcheckTailArgs ta, SumcheckTerms tm, u32 m, int pending, u32 round,
                                                                         TranscriptState state0, int first, char* state, const char* cell,
                                                                         char* rounds, char* point, char* finals, char* value) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  __shared__ u32 lds[F::N][SUMCHECK_THREADS];
  __shared__ u32 msg[SUMCHECK_MSG_WORDS];
  __shared__ u32 r_lds[F::N];
  __shared__ const char* tabs[3][SUMCHECK_MAX_TABLES];   // [0]: the tables as they arrive; [1], [2]: the two sets
  const u32 tid = threadIdx.x;
  const u32 degree = tm.degree, ntables = tm.ntables;
  if (tid < (u32)SUMCHECK_MAX_TABLES) {
    tabs[0][tid] = ta.src[tid];
    tabs[1][tid] = ta.set[0][tid];
    tabs[2][tid] = ta.set[1][tid];
  }
  if (tid < (u32)TRANSCRIPT_STATE_WORDS) msg[tid] = first ? state0.w[tid] : ((const u32*)state)[tid];
  if (pending && tid < (u32)F::N) r_lds[tid] = ((const u32*)cell)[tid];
  __syncthreads();
  u32 cur = 0, nxt = 1;
  if (pending) m += 1;
  bool bind = pending != 0;
  for (;;) {
    if (bind) {   // tables of m variables -> m - 1, into the set that is not read
      F r;
#pragma unroll
      for (int j = 0; j < F::N; j++) r.l[j] = r_lds[j];
      const u32 half = 1u << (m - 1);
      for (u32 k = 0; k < ntables; k++) {
        const char* s = tabs[cur][k];
        char* d = (char*)tabs[nxt][k];
        for (u32 i = tid; i < half; i += SUMCHECK_THREADS)
          mle_bind<F>(F::load(s + (size_t)i * (2 * F::BYTES)), F::load(s + (size_t)i * (2 * F::BYTES) + F::BYTES), r).store(d + (size_t)i * F::BYTES);
      }
      m -= 1;
      cur = nxt;
      nxt = cur == 1 ? 2 : 1;
      __syncthreads();   // the set is written: this workgroup reads it next
    }
    bind = true;
    if (m == 0) break;
    F a0 = F::zero(), a1 = F::zero(), a2 = F::zero(), a3 = F::zero(), a4 = F::zero();
    const u32 npairs = 1u << (m - 1);
    for (u32 p = tid; p < npairs; p += SUMCHECK_THREADS) {
      F lo[NT], df[NT];
#pragma unroll
      for (int k = 0; k < NT; k++) {
        lo[k] = F::zero();
        df[k] = F::zero();
        if ((u32)k < ntables) {
          const char* s = tabs[cur][k] + (size_t)p * (2 * F::BYTES);
          lo[k] = F::load(s);
          df[k] = F::sub(F::load(s + F::BYTES), lo[k]);
        }
      }
      sumcheck_pair_terms<F, NT>(lo, df, tm, a0, a1, a2, a3, a4);
    }
    const F acc[SUMCHECK_EVALS] = {a0, a1, a2, a3, a4};
#pragma unroll
    for (int t = 0; t < SUMCHECK_EVALS; t++) {
      if ((u32)t <= degree) {   // uniform
        const F s = sumcheck_block_sum<F>(acc[t], lds);
        if (tid == 0) {
          s.store(rounds + ((size_t)round * (degree + 1) + t) * F::BYTES);
          transcript_put_element<F>(msg, (u32)t, s);
        }
      }
    }
    if (tid == 0) {
      const F r = transcript_challenge_words<F>(msg, degree + 1);
      r.store(point + (size_t)round * F::BYTES);
#pragma unroll
      for (int j = 0; j < F::N; j++) r_lds[j] = r.l[j];
    }
    round += 1;
    __syncthreads();   // r is in LDS
  }
  // m = 0: the one-element tables are the values f_k(point); the sum's value there is what the m = 0 round calls evals[0]
  F lo[NT], df[NT];
#pragma unroll
  for (int k = 0; k < NT; k++) {
    df[k] = F::zero();
    lo[k] = (u32)k < ntables ? F::load(tabs[cur][k]) : F::zero();
  }
  F a0 = F::zero(), a1 = F::zero(), a2 = F::zero(), a3 = F::zero(), a4 = F::zero();
  sumcheck_pair_terms<F, NT>(lo, df, tm, a0, a1, a2, a3, a4);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < NT; k++)
      if ((u32)k < ntables) lo[k].store(finals + (size_t)k * F::BYTES);
    a0.store(value);
    for (int i = 0; i < TRANSCRIPT_STATE_WORDS; i++) ((u32*)state)[i] = msg[i];
  }
}

// queues the whole proof on s; nothing waits
template <class F, int NT>
int sumcheck_prove_run_nt(const SumcheckProve& pv, hipStream_t s) {
  const unsigned nv = pv.num_vars, nt = pv.tm.ntables, deg = pv.tm.degree;
  const int hand = sumcheck_prove_hand(nv, pv.tail_from);
  SumcheckTables tb = {};
  for (unsigned k = 0; k < nt; k++) tb.src[k] = pv.src[k];
  SumcheckTerms tm = pv.tm;   // for the rounds that bind: the challenge is where the challenge kernel left it
  tm.r_cell = (const char*)pv.cell;
  int next = 0;
  for (int i = 0; i < hand; i++) {
    const int m = (int)nv - i;   // variables of the tables this round sums
    unsigned blocks;
    size_t ppl;
    sumcheck_geometry(m, &blocks, &ppl);
    char* first = (char*)(blocks == 1 ? pv.sums : pv.partials);
    const size_t npairs = (size_t)1 << (m - 1);
    if (i == 0) {
      hipLaunchKernelGGL((sumcheck_round_kernel<F, NT, false>), dim3(blocks), dim3(SUMCHECK_THREADS), 0, s, tb, pv.tm, npairs, 0, first);
    } else {
      for (unsigned k = 0; k < nt; k++) tb.dst[k] = pv.set[next][k];
      hipLaunchKernelGGL((sumcheck_round_kernel<F, NT, true, true>), dim3(blocks), dim3(SUMCHECK_THREADS), 0, s, tb, tm, npairs, 0, first);
      for (unsigned k = 0; k < nt; k++) tb.src[k] = tb.dst[k];
      next ^= 1;
    }
    if (hipGetLastError() != hipSuccess) return -1000;
    if (blocks > 1)
      hipLaunchKernelGGL((sumcheck_fold_kernel<F>), dim3(1), dim3(SUMCHECK_THREADS), 0, s, (const char*)pv.partials, blocks, (char*)pv.sums);
    if (hipGetLastError() != hipSuccess) return -1000;
    hipLaunchKernelGGL((sumcheck_challenge_kernel<F>), dim3(1), dim3(64), 0, s, (const char*)pv.sums, deg + 1, pv.state0, i == 0 ? 1 : 0,
                       (char*)pv.state, (char*)pv.rounds + (size_t)i * (deg + 1) * F::BYTES, (char*)pv.cell,
                       (char*)pv.point + (size_t)i * F::BYTES);
    if (hipGetLastError() != hipSuccess) return -1000;
  }
  if (pv.tail_from <= 0) {   // the m = 0 round binds the last challenge; then the gather
    for (unsigned k = 0; k < nt; k++) tb.dst[k] = pv.set[next][k];
    hipLaunchKernelGGL((sumcheck_round_kernel<F, NT, true, true>), dim3(1), dim3(SUMCHECK_THREADS), 0, s, tb, tm, (size_t)1, 1, (char*)pv.sums);
    if (hipGetLastError() != hipSuccess) return -1000;
    for (unsigned k = 0; k < nt; k++) tb.src[k] = tb.dst[k];
    hipLaunchKernelGGL((sumcheck_finals_kernel<F>), dim3(1), dim3(64), 0, s, tb, nt, (const char*)pv.sums, (char*)pv.finals, (char*)pv.value);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  }
  SumcheckTailArgs ta = {};
  for (unsigned k = 0; k < nt; k++) {
    ta.src[k] = tb.src[k];
    ta.set[0][k] = pv.set[next][k];
    ta.set[1][k] = pv.set[next ^ 1][k];
  }
  hipLaunchKernelGGL((sumcheck_tail_kernel<F, NT>), dim3(1), dim3(SUMCHECK_THREADS), 0, s, ta, pv.tm, (u32)((int)nv - hand), hand > 0 ? 1 : 0,
                     (u32)hand, pv.state0, hand == 0 ? 1 : 0, (char*)pv.state, (const char*)pv.cell, (char*)pv.rounds, (char*)pv.point,
                     (char*)pv.finals, (char*)pv.value);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
template <class F>
int sumcheck_prove_run(const SumcheckProve& pv, hipStream_t s) {
  if (pv.num_vars == 0 || pv.num_vars > 58 || pv.tm.ntables == 0 || pv.tm.ntables > (u32)SUMCHECK_MAX_TABLES) return -1000;
  if (pv.tail_from < 0 || pv.tail_from > SUMCHECK_TAIL_MAX_VARS) return -1000;
  return pv.tm.ntables <= 4 ? sumcheck_prove_run_nt<F, 4>(pv, s) : sumcheck_prove_run_nt<F, 8>(pv, s);
}

}  // namespace arkhip
