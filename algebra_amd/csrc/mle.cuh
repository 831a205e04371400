// Dense multilinear extensions on device-resident evaluation tables of Fr:
//   mle_fold_kernel      MultilinearExtension::fix_variables / Polynomial::evaluate of DenseMultilinearExtension
//                        (poly/src/evaluations/multivariate/multilinear/dense.rs:224-257, :460-465): several variables per launch;
//   mle_relabel_kernel   relabel / relabel_in_place (dense.rs:76-92, swap_bits: multilinear/mod.rs:90-96);
//   fr_axpy_kernel       r = a + k x, the AddAssign<(F, &Self)> of dense.rs:319-327 in one pass.
//
// Binding variable 0 of a table t maps out[b] = t[2b] + r (t[2b+1] - t[2b]); index bit 0 is the first variable.  Folds in
// different index bits commute and every value is a canonical residue, so any order of the folds gives the reference's bits.
//
// One launch binds the w <= MLE_TILE_LOG lowest index bits of its input.  A WAVE is the unit of work (workgroups are one wave:
// no LDS, no barrier): it takes 2^GL consecutive tiles of 2^MLE_TILE_LOG = 512 elements.  Of a tile, lane l owns the MLE_E = 8
// strided elements k * 64 + l -- a wave's load instruction reads contiguous 2 KiB -- so index bits 0..5 are the lane number
// and bits 6..8 the register slot.
//   phase A  (w > 6)  binds bits 6..w-1 between a lane's own registers, every lane busy: 8 - 2^(9-w) products per tile.  What is
//            left of the tiles of the wave are S = 2^(9-w+GL) <= 8 values per lane: independent output STREAMS, numbered by
//            index bits w..w+2.
//   phase B  binds bits 0..min(w,6)-1 across lanes.  While a lane holds S' >= 2 streams, the two lanes of a pair each keep one
//            half of the streams and hand the other half over (__shfl_xor), so both do S'/2 useful products and the lane bit
//            takes the place of the top stream bit; with one stream left both lanes of a pair compute the same value.
// Products issued per element for a full tile: (7 2^GL + sum) / (8 2^GL), sum = 4+2+1+1+1+1 for GL = 3: 66 / 64 = 1.03
// (GL = 2: 1.09, GL = 1: 1.25, GL = 0: 1.63); binding one variable costs the 0.5 the arithmetic needs.
#pragma once
#include "polyops.cuh"

namespace arkhip {

constexpr int MLE_TILE_LOG = 9;   // variables one launch can bind
constexpr int MLE_LANE_LOG = 6;   // index bits held by the lane number
constexpr int MLE_E = 8;          // strided elements of a tile per lane
constexpr int MLE_MAX_PASSES = 8; // 7 * 9 >= 63
static_assert((1 << (MLE_TILE_LOG - MLE_LANE_LOG)) == MLE_E, "slots are the tile's index bits above the lane's");

// the points of one launch, by value: r[j] binds index bit j of the launch's input
struct MlePoint {
  FrConst r[MLE_TILE_LOG];
};

// widths of the launches that bind `dim` variables: as many full tiles as fit, the remainder last
static inline int mle_fold_passes(int dim, int* widths) {
  int passes = 0;
  while (dim > 0) {
    const int w = dim < MLE_TILE_LOG ? dim : MLE_TILE_LOG;
    if (widths) widths[passes] = w;
    passes++;
    dim -= w;
  }
  return passes;
}
// tiles per wave (log2) of a launch that binds w bits of 2^m elements: the most that still leaves 2^MLE_MIN_WAVES_LOG waves
// (two per SIMD of an MI355X; 9 and 13 measured slower, profiles/mle_threshold_ab.txt)
constexpr int MLE_MIN_WAVES_LOG = 11;
static inline int mle_fold_group_log(int m, int w) {
  int gl = w > MLE_LANE_LOG ? w - MLE_LANE_LOG : 0;
  while (gl > 0 && m - (MLE_TILE_LOG + gl) < MLE_MIN_WAVES_LOG) gl--;
  return gl;
}

template <class F>
ARK_DEV F mle_bind(const F& lo, const F& hi, const F& r) { return F::add(lo, F::mul(r, F::sub(hi, lo))); }
template <class F>
ARK_DEV F mle_pick(bool c, const F& a, const F& b) {   // c ? a : b
  F v;
#pragma unroll
  for (int j = 0; j < F::N; j++) v.l[j] = c ? a.l[j] : b.l[j];
  return v;
}
template <class F>
ARK_DEV F mle_lane_xor(const F& a, int mask) {
  F v;
#pragma unroll
  for (int j = 0; j < F::N; j++) v.l[j] = (u32)__shfl_xor((int)a.l[j], mask, 64);
  return v;
}

// dst[i >> WB] for the 2^m elements of src, m >= WB; src and dst do not overlap
template <class F, int WB, int GL>
__global__ void __launch_bounds__(64) mle_fold_kernel(const char* __restrict__ src, size_t n, MlePoint pt, char* __restrict__ dst) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  static_assert(WB >= 1 && WB <= MLE_TILE_LOG && GL >= 0 && (GL == 0 || GL <= WB - MLE_LANE_LOG), "at most 8 streams per lane");
  constexpr int NA = WB > MLE_LANE_LOG ? WB - MLE_LANE_LOG : 0;   // bits bound between registers
  constexpr int NB = WB - NA;                                     // bits bound across lanes
  constexpr int NV = MLE_E >> NA;                                 // values a tile leaves per lane
  constexpr int S = NV << GL;                                     // streams per lane
  const u32 lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x << (MLE_TILE_LOG + GL);
  F y[S];
#pragma unroll
  for (int q = 0; q < S; q++) y[q] = F::zero();
#pragma unroll 1
  for (int g = 0; g < (1 << GL); g++) {
    F x[MLE_E];
#pragma unroll
    for (int k = 0; k < MLE_E; k++) {
      const size_t gi = base + ((size_t)g << MLE_TILE_LOG) + (u32)k * 64 + lane;
      x[k] = F::zero();
      if (gi < n) x[k] = F::load(src + gi * F::BYTES);
    }
#pragma unroll
    for (int a = 0; a < NA; a++) {
      const F r = fr_from_const<F>(pt.r[MLE_LANE_LOG + a]);
#pragma unroll
      for (int t = 0; t < (MLE_E >> (a + 1)); t++) x[t] = mle_bind<F>(x[2 * t], x[2 * t + 1], r);
    }
    // the streams of the tiles so far move down, this tile's enter at the top: y[g NV + q] in the end
#pragma unroll
    for (int q = 0; q + NV < S; q++) y[q] = y[q + NV];
#pragma unroll
    for (int q = 0; q < NV; q++) y[S - NV + q] = x[q];
  }
  int cnt = S;     // streams a lane holds; a constant in every unrolled step
  u32 top = 0;     // the stream bits that lane bits have taken over
#pragma unroll
  for (int j = 0; j < NB; j++) {
    const bool up = (lane >> j) & 1;
    const F r = fr_from_const<F>(pt.r[j]);
    if (cnt >= 2) {
      const int h = cnt / 2;
#pragma unroll
      for (int t = 0; t < h; t++) {
        const F keep = mle_pick<F>(up, y[h + t], y[t]);
        const F got = mle_lane_xor<F>(mle_pick<F>(up, y[t], y[h + t]), 1 << j);
        y[t] = mle_bind<F>(mle_pick<F>(up, got, keep), mle_pick<F>(up, keep, got), r);
      }
      top = top * 2 + (up ? 1u : 0u);
      cnt = h;
    } else {
      const F got = mle_lane_xor<F>(y[0], 1 << j);
      y[0] = mle_bind<F>(mle_pick<F>(up, got, y[0]), mle_pick<F>(up, y[0], got), r);
    }
  }
  // a lane pair that computed the same value writes it once: the lane whose bits past the exchanged ones are zero
  constexpr int S_LOG = S == 8 ? 3 : S == 4 ? 2 : S == 2 ? 1 : 0;
  constexpr int JX = NB < S_LOG ? NB : S_LOG;   // steps that halved the streams
  const bool writer = ((lane & ((1u << NB) - 1)) >> JX) == 0;
  const size_t n_out = n >> WB;
  const size_t out_base = ((size_t)blockIdx.x << (MLE_TILE_LOG + GL - WB)) + (lane >> WB);
#pragma unroll
  for (int t = 0; t < (S >> JX); t++) {
    const u32 stream = top * (u32)(S >> JX) + (u32)t;
    const size_t o = out_base + ((size_t)stream << (MLE_LANE_LOG - NB));
    if (writer && o < n_out) y[t].store(dst + o * F::BYTES);
  }
}

template <class F, int WB, int GL>
int mle_fold_launch_one(const void* src, int m, const MlePoint& pt, void* dst, hipStream_t s) {
  const size_t n = (size_t)1 << m;
  const size_t waves = m > MLE_TILE_LOG + GL ? n >> (MLE_TILE_LOG + GL) : 1;
  if (waves > 0x7fffffffu) return -1000;
  hipLaunchKernelGGL((mle_fold_kernel<F, WB, GL>), dim3((unsigned)waves), dim3(64), 0, s, (const char*)src, n, pt, (char*)dst);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
// binds the w lowest index bits of the 2^m elements of src (1 <= w <= min(m, MLE_TILE_LOG)) with pt.r[0 .. w-1]
template <class F>
int mle_fold_launch(const void* src, int m, int w, const MlePoint& pt, void* dst, hipStream_t s) {
  if (w < 1 || w > MLE_TILE_LOG || w > m || m > 62) return -1000;
  const int gl = mle_fold_group_log(m, w);
#define ARK_MLE_CASE(WB, GL) \
  if (w == WB && gl == GL) return mle_fold_launch_one<F, WB, GL>(src, m, pt, dst, s);
  ARK_MLE_CASE(1, 0) ARK_MLE_CASE(2, 0) ARK_MLE_CASE(3, 0) ARK_MLE_CASE(4, 0) ARK_MLE_CASE(5, 0) ARK_MLE_CASE(6, 0)
  ARK_MLE_CASE(7, 0) ARK_MLE_CASE(7, 1)
  ARK_MLE_CASE(8, 0) ARK_MLE_CASE(8, 1) ARK_MLE_CASE(8, 2)
  ARK_MLE_CASE(9, 0) ARK_MLE_CASE(9, 1) ARK_MLE_CASE(9, 2) ARK_MLE_CASE(9, 3)
#undef ARK_MLE_CASE
  return -1000;
}

// swap_bits(x, a, b, k) of multilinear/mod.rs:90-96
ARK_HD size_t mle_swap_bits(size_t x, int a, int b, int k) {
  const size_t mask = ((size_t)1 << k) - 1;
  const size_t d = ((x >> a) ^ (x >> b)) & mask;
  return x ^ ((d << a) | (d << b));
}
// dst[i] = src[swap_bits(i)]; dst == src (the same pointer): lane i exchanges with its image j when i < j, and no other lane
// touches either element
template <class F>
__global__ void __launch_bounds__(256) mle_relabel_kernel(const char* src, size_t n, int a, int b, int k, char* dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t j = mle_swap_bits(i, a, b, k);
  if (src != dst) {
    F::load(src + j * F::BYTES).store(dst + i * F::BYTES);
  } else if (i < j) {
    const F u = F::load(src + i * F::BYTES), v = F::load(src + j * F::BYTES);
    v.store(dst + i * F::BYTES);
    u.store(dst + j * F::BYTES);
  }
}
template <class F>
int mle_relabel_launch(const void* src, size_t n, int a, int b, int k, void* dst, hipStream_t s) {
  if (n == 0) return 0;
  if ((n + 255) / 256 > 0x7fffffffu) return -1000;
  hipLaunchKernelGGL((mle_relabel_kernel<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const char*)src, n, a, b, k,
                     (char*)dst);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// r[i] = a[i] + k x[i]; r may alias a or x
template <class F>
__global__ void __launch_bounds__(256) fr_axpy_kernel(const char* a, FrConst k, const char* x, char* r, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  F::add(F::load(a + i * F::BYTES), F::mul(fr_from_const<F>(k), F::load(x + i * F::BYTES))).store(r + i * F::BYTES);
}
template <class F>
int fr_axpy_launch(const void* a, const uint64_t* k4, const void* x, void* r, size_t n, hipStream_t s) {
  if (n == 0) return 0;
  if ((n + 255) / 256 > 0x7fffffffu) return -1000;
  FrConst k;
  for (int j = 0; j < 4; j++) { k.l[2 * j] = (u32)k4[j]; k.l[2 * j + 1] = (u32)(k4[j] >> 32); }
  hipLaunchKernelGGL((fr_axpy_kernel<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const char*)a, k, (const char*)x,
                     (char*)r, n);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace arkhip
