// Polynomial operations on device-resident coefficient / evaluation vectors of Fr:
//   poly_tile_value_kernel   per-tile Horner values: DensePolynomial::evaluate (poly/src/polynomial/univariate/dense.rs:42-92) and the
//                            first phase of the division by x - z;
//   poly_tile_divide_kernel  synthetic division by x - z inside a tile, given the tile's carry-in (the naive division of
//                            DenseOrSparsePolynomial::divide_with_q_and_r for a degree-1 divisor, univariate/mod.rs:145-159);
//   poly_vanishing_kernel    DensePolynomial::divide_by_vanishing_poly (dense.rs:168-211);
//   poly_lagrange_kernel     the denominators of EvaluationDomain::evaluate_all_lagrange_coefficients (poly/src/domain/mod.rs:157-222);
//   fr_inner_product_*       sum a_i b_i.
//
// Division by x - z is the recurrence s[i] = p[i] + z s[i+1], s[n] = 0: q[i] = s[i+1], remainder s[0] = p(z).  Reduce-then-scan
// over tiles of POLY_TILE elements: the tile values V_b = sum_e p[b T + e] z^e form a polynomial of ceil(n / T) coefficients
// whose division by x - z^T gives every tile its carry-in s[(b+1) T] (quotient) and p(z) (remainder) -- the same problem, T times
// shorter, solved by the same two kernels until one tile is left.  Order between the phases comes from kernel boundaries
// only: no workgroup ever waits on another.
//
// Inside a tile a lane owns POLY_E CONSECUTIVE elements (the suffix order the recurrence needs) while global memory is
// read and written in element order across the lanes (a wave moves contiguous 2 KiB): the two views are exchanged through
// LDS, one 32-bit limb plane per limb with one pad word per POLY_E elements, so both the lane-consecutive and the
// element-consecutive accesses are free of bank conflicts (word strides 1 and POLY_E + 1 = 9).
#pragma once
#include "devops.cuh"

namespace arkhip {

constexpr int POLY_TILE = 2048;     // elements per tile = per workgroup
constexpr int POLY_THREADS = 256;
constexpr int POLY_E = POLY_TILE / POLY_THREADS;   // consecutive elements per lane
constexpr int POLY_LOG_THREADS = 8;
constexpr int POLY_PLANE = POLY_TILE + POLY_TILE / POLY_E;   // words per limb plane (padded)
static_assert(POLY_E == 8 && (1 << POLY_LOG_THREADS) == POLY_THREADS, "the pad rule e + (e >> 3) and the 8 scan steps assume this");

// scan levels of a length-n division / evaluation: 1 while one tile holds everything, one more per factor POLY_TILE
static inline int poly_scan_levels(size_t n) {
  int levels = 1;
  while (n > (size_t)POLY_TILE) {
    n = (n + POLY_TILE - 1) / POLY_TILE;
    levels++;
  }
  return levels;
}

// powers of the point of one level, computed once on the host and passed by value: z and z^(E 2^j), j = 0 .. 7
struct PolyPowers {
  FrConst z;
  FrConst zs[POLY_LOG_THREADS];
};

template <class F>
ARK_DEV F fr_from_const(const FrConst& k) {
  F r;
#pragma unroll
  for (int j = 0; j < F::N; j++) r.l[j] = k.l[j];
  return r;
}
template <class F>
ARK_DEV void poly_lds_put(u32 (*lds)[POLY_PLANE], u32 at, const F& v) {
#pragma unroll
  for (int j = 0; j < F::N; j++) lds[j][at] = v.l[j];
}
template <class F>
ARK_DEV F poly_lds_get(u32 (*lds)[POLY_PLANE], u32 at) {
  F v;
#pragma unroll
  for (int j = 0; j < F::N; j++) v.l[j] = lds[j][at];
  return v;
}

// tile [base, base + T) of src (zero beyond n) -> x[k] = element base + tid * E + k; ends with every lane done reading LDS
template <class F>
ARK_DEV void poly_tile_load(u32 (*lds)[POLY_PLANE], const char* src, size_t base, size_t n, F* x) {
  const u32 tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < POLY_E; k++) {
    const u32 e = (u32)k * POLY_THREADS + tid;
    const size_t gi = base + e;
    F v = F::zero();
    if (gi < n) v = F::load(src + gi * F::BYTES);
    poly_lds_put<F>(lds, e + (e >> 3), v);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < POLY_E; k++) x[k] = poly_lds_get<F>(lds, tid * (POLY_E + 1) + k);
  __syncthreads();
}
// h = sum_k x[k] z^k
template <class F>
ARK_DEV F poly_lane_horner(const F* x, const F& z) {
  F h = x[POLY_E - 1];
#pragma unroll
  for (int k = POLY_E - 2; k >= 0; k--) h = F::add(x[k], F::mul(z, h));
  return h;
}

// vals[b] = sum_e src[b T + e] z^e
template <class F>
__global__ void __launch_bounds__(POLY_THREADS) poly_tile_value_kernel(const char* src, size_t n, PolyPowers pw, char* vals) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  __shared__ u32 lds[F::N][POLY_PLANE];
  const u32 tid = threadIdx.x;
  F x[POLY_E];
  poly_tile_load<F>(lds, src, (size_t)blockIdx.x * POLY_TILE, n, x);
  F h = poly_lane_horner<F>(x, fr_from_const<F>(pw.z));
  poly_lds_put<F>(lds, tid, h);
  // sum_t h_t z^(E t): halve the lane count, the upper half enters with z^(E d)
#pragma unroll
  for (int j = POLY_LOG_THREADS - 1; j >= 0; j--) {
    const u32 d = 1u << j;
    __syncthreads();
    if (tid < d) {
      h = F::add(h, F::mul(fr_from_const<F>(pw.zs[j]), poly_lds_get<F>(lds, tid + d)));
      poly_lds_put<F>(lds, tid, h);
    }
  }
  if (tid == 0) h.store(vals + (size_t)blockIdx.x * F::BYTES);
}

// dst[i] = s[i + 1] for the tile's i < n - 1, where s[i] = src[i] + z s[i + 1] and s[(b + 1) T] = carries[b] (0 for the last
// tile, and everywhere when carries == nullptr); tile 0 writes s[0] to rem when that is not null.  dst may BE src: the tile is
// read completely before any of it is written, and no other tile reads it.
template <class F>
__global__ void __launch_bounds__(POLY_THREADS) poly_tile_divide_kernel(const char* src, size_t n, PolyPowers pw, const char* carries,
                                                                        char* dst, char* rem) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  __shared__ u32 lds[F::N][POLY_PLANE];
  const u32 tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * POLY_TILE;
  F x[POLY_E];
  poly_tile_load<F>(lds, src, base, n, x);
  const F z = fr_from_const<F>(pw.z);
  F carry = F::zero();
  if (carries && blockIdx.x + 1 < gridDim.x) carry = F::load(carries + (size_t)blockIdx.x * F::BYTES);
  F h = poly_lane_horner<F>(x, z);
  if (tid == POLY_THREADS - 1) h = F::add(h, F::mul(fr_from_const<F>(pw.zs[0]), carry));
  // inclusive suffix scan over the lanes: S_t = sum_{u >= t} h_u z^(E (u - t)); step d folds in the lane d further up
  u32 o = 0;
  poly_lds_put<F>(lds, tid, h);
#pragma unroll
  for (int j = 0; j < POLY_LOG_THREADS; j++) {
    const u32 d = 1u << j;
    __syncthreads();
    if (tid + d < POLY_THREADS) h = F::add(h, F::mul(fr_from_const<F>(pw.zs[j]), poly_lds_get<F>(lds, o + tid + d)));
    o ^= POLY_THREADS;   // ping-pong: the values of this step are still being read from the other half
    poly_lds_put<F>(lds, o + tid, h);
  }
  __syncthreads();
  F s = tid + 1 < POLY_THREADS ? poly_lds_get<F>(lds, o + tid + 1) : carry;   // s[base + (tid + 1) E]
  __syncthreads();
#pragma unroll
  for (int k = POLY_E - 1; k >= 0; k--) {
    const F q = s;
    s = F::add(x[k], F::mul(z, s));
    x[k] = q;
  }
  if (rem && blockIdx.x == 0 && tid == 0) s.store(rem);
#pragma unroll
  for (int k = 0; k < POLY_E; k++) poly_lds_put<F>(lds, tid * (POLY_E + 1) + k, x[k]);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < POLY_E; k++) {
    const u32 e = (u32)k * POLY_THREADS + tid;
    const size_t gi = base + e;
    if (gi + 1 < n) poly_lds_get<F>(lds, e + (e >> 3)).store(dst + gi * F::BYTES);
  }
}

template <class F>
int poly_tile_value_launch(const void* src, size_t n, const PolyPowers& pw, void* vals, hipStream_t s) {
  if (n == 0) return 0;
  const size_t tiles = (n + POLY_TILE - 1) / POLY_TILE;
  hipLaunchKernelGGL((poly_tile_value_kernel<F>), dim3((unsigned)tiles), dim3(POLY_THREADS), 0, s, (const char*)src, n, pw, (char*)vals);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
template <class F>
int poly_tile_divide_launch(const void* src, size_t n, const PolyPowers& pw, const void* carries, void* dst, void* rem, hipStream_t s) {
  if (n == 0) return 0;
  const size_t tiles = (n + POLY_TILE - 1) / POLY_TILE;
  hipLaunchKernelGGL((poly_tile_divide_kernel<F>), dim3((unsigned)tiles), dim3(POLY_THREADS), 0, s, (const char*)src, n, pw,
                     (const char*)carries, (char*)dst, (char*)rem);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// Division by x^m - 1 for n >= m: lane t < m walks its residue class t, t + m, t + 2m, ... from the top, so the work is
// O(n) however many multiples of m fit (the reference adds n / m shifted copies, dense.rs:183-188) and a wave reads and
// writes contiguous runs.  q: n - m elements, r: m elements; neither may alias p.  The parallelism is m and a lane's n / m
// steps are serial: made for the prover's case (n a few times m, m large); a small domain under a long polynomial runs on a
// few workgroups only.
template <class F>
__global__ void __launch_bounds__(256) poly_vanishing_kernel(const char* p, size_t n, size_t m, char* q, char* r) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  F acc = F::zero();
  for (size_t i = (n - 1 - t) / m; i >= 1; i--) {
    const size_t idx = t + i * m;
    acc = F::add(acc, F::load(p + idx * F::BYTES));
    acc.store(q + (idx - m) * F::BYTES);
  }
  F::add(F::load(p + t * F::BYTES), acc).store(r + t * F::BYTES);
}
template <class F>
int poly_vanishing_launch(const void* p, size_t n, size_t m, void* q, void* r, hipStream_t s) {
  if (m == 0 || n < m) return -1000;
  hipLaunchKernelGGL((poly_vanishing_kernel<F>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, (const char*)p, n, m,
                     (char*)q, (char*)r);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// w^t by square and multiply from the top bit: once per lane, its further elements follow by steps of w^lanes
template <class F>
ARK_DEV F poly_lane_power(const F& w, size_t t) {
  F r = F::one();
  for (int b = 63 - __clzll((unsigned long long)(t | 1)); b >= 0; b--) {
    r = F::sqr(r);
    if ((t >> b) & 1) r = F::mul(r, w);
  }
  return r;
}
// d_i = a w^i - c for i < n; onehot == 0: out[i] = d_i (the inverse Lagrange coefficients: a = l_0 tau, c = l_0 h,
// w = g^-1, domain/mod.rs:204-215 with the two running products folded into one); onehot != 0: out[i] = d_i == 0 ? 1 : 0
// (tau in the coset: a = h, w = g, c = tau, :175-189).  Lane t owns i = t, t + lanes, ...: a wave writes contiguous runs.
template <class F>
__global__ void __launch_bounds__(128) poly_lagrange_kernel(FrConst a, FrConst c, FrConst w, FrConst wstep, int onehot, char* out,
                                                            size_t n, size_t lanes) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= lanes) return;
  const F cc = fr_from_const<F>(c), step = fr_from_const<F>(wstep);
  F cur = F::mul(fr_from_const<F>(a), poly_lane_power<F>(fr_from_const<F>(w), t));   // a w^i
  for (size_t i = t; i < n; i += lanes) {
    F d = F::sub(cur, cc);
    if (onehot) d = d.is_zero() ? F::one() : F::zero();
    d.store(out + i * F::BYTES);
    cur = F::mul(cur, step);
  }
}
// lanes of poly_lagrange_kernel for n outputs: 8 strided elements per lane
static inline size_t poly_lagrange_lanes(size_t n) { return (n + 7) / 8; }
template <class F>
int poly_lagrange_launch(const uint64_t* a4, const uint64_t* c4, const uint64_t* w4, const uint64_t* wstep4, int onehot, void* out,
                         size_t n, size_t lanes, hipStream_t s) {
  if (n == 0) return 0;
  if (lanes != poly_lagrange_lanes(n)) return -1000;   // wstep4 = w^lanes was computed for this partition
  FrConst k[4];
  const uint64_t* src[4] = {a4, c4, w4, wstep4};
  for (int q = 0; q < 4; q++)
    for (int j = 0; j < 4; j++) { k[q].l[2 * j] = (u32)src[q][j]; k[q].l[2 * j + 1] = (u32)(src[q][j] >> 32); }
  hipLaunchKernelGGL((poly_lagrange_kernel<F>), dim3((unsigned)((lanes + 127) / 128)), dim3(128), 0, s, k[0], k[1], k[2], k[3],
                     onehot, (char*)out, n, lanes);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// sum_i a[i] b[i]: every lane sums its grid-strided products, a workgroup adds its lanes' sums through LDS and leaves one
// partial; the same kernel with b == nullptr then adds the partials in one workgroup.
constexpr int INNER_BLOCKS = 1024;
template <class F>
__global__ void __launch_bounds__(256) fr_inner_product_kernel(const char* a, const char* b, size_t n, char* out) {
  __shared__ u32 lds[F::N][256];
  const u32 tid = threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  F acc = F::zero();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + tid; i < n; i += stride) {
    const F x = F::load(a + i * F::BYTES);
    acc = F::add(acc, b ? F::mul(x, F::load(b + i * F::BYTES)) : x);
  }
#pragma unroll
  for (int j = 0; j < F::N; j++) lds[j][tid] = acc.l[j];
  for (u32 d = 128; d >= 1; d >>= 1) {
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
  if (tid == 0) acc.store(out + (size_t)blockIdx.x * F::BYTES);
}
// partials: room for INNER_BLOCKS elements; out: one element (device memory)
template <class F>
int fr_inner_product_launch(const void* a, const void* b, size_t n, void* partials, void* out, hipStream_t s) {
  size_t blocks = (n + 255) / 256;
  if (blocks > (size_t)INNER_BLOCKS) blocks = INNER_BLOCKS;
  if (blocks == 0) blocks = 1;   // n == 0: the empty sum
  hipLaunchKernelGGL((fr_inner_product_kernel<F>), dim3((unsigned)blocks), dim3(256), 0, s, (const char*)a, (const char*)b, n,
                     (char*)(blocks == 1 ? out : partials));
  if (hipGetLastError() != hipSuccess) return -1000;
  if (blocks > 1)
    hipLaunchKernelGGL((fr_inner_product_kernel<F>), dim3(1), dim3(256), 0, s, (const char*)partials, (const char*)nullptr, blocks,
                       (char*)out);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace arkhip
