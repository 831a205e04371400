// Multilinear openings on device-resident tables of Fr, in section 12's conventions (index bit 0 is the
// first variable, canonical Montgomery residues):
//   mle_eq_kernel     the table eq(r, b) = prod_i (b_i ? r_i : 1 - r_i), times a scale: a write-only pass;
//   mle_quot_kernel   the fold of mle.cuh that also stores every level's differences q_i[b] = f_i[2b+1] - f_i[2b], the
//                     quotients of f(x) - f(z) = sum_i (x_i - z_i) q_i(x_{i+1}, ...).
// Workgroups are one wave: no LDS, no barrier, no atomics.
//
// mle_eq_kernel.  A wave owns 2^gl consecutive tiles of 2^MLE_TILE_LOG = 512 outputs; of a tile, lane l writes the 8 elements
// k * 64 + l (a store instruction of the wave covers contiguous 2 KiB).  Once per wave a lane builds the weights of its own
// low index bits: 5 products for its lane number (bits 0..5), then 1 + 2 + 4 = 7 for the three slot bits, each doubling
// v -> (v - v r, v r) by ONE product; these are the 8 values w[k] it keeps.  The weight of a tile's high bits is one element
// of a table of 2^(m-9) entries, which an earlier launch of this same kernel wrote (the topmost launch takes the scale in
// its place), so no launch reads more than 1/512 of what it writes.  Per tile a lane then issues 8 products h w[k].
// Products issued per output: 1 + 12 / (8 2^gl).  The doubling's 0.5 per output is the cost of the LAST level alone, given
// the level before it; a pass that reads no half-size table pays for all levels, sum_k 2^-k = 1.
//
// mle_quot_kernel.  The quotients fix the ORDER of the folds -- q_i is a difference of the table with variables 0..i-1 bound --
// so a tile binds its bits from the lowest up, and a lane owns 8 CONSECUTIVE elements: index bits 0..2 are the register slot,
// bits 3..8 the lane number.
//   phase A  binds bits 0..min(w,3)-1 between a lane's own registers; every difference is stored by the lane that formed it.
//   phase B  binds bits 3..w-1 across lanes with one value per lane: step j exchanges with lane ^ 2^j; the 2^(j+1) lanes of a
//            group compute the same difference, and the one whose low j+1 lane bits are zero stores it.
// Products issued per element of a full tile: (7 + 6) / 8 = 1.63, of which 0.5 are needed (the fold's figure at one tile per
// wave, mle.cuh).  Segment i of the output starts at element 2^nu - 2^(nu-i): wave-uniform.
#pragma once
#include "mle.cuh"

namespace arkhip {

constexpr int MLE_EQ_MAX_GROUP_LOG = 3;   // at most 8 tiles per wave
// the launches of the eq table of nv variables, in order: launch p writes the table of the TOP widths[0] + .. + widths[p]
// variables, the remainder first (the smallest table), every later one a full tile's 9
static inline int mle_eq_passes(int nv, int* widths) {
  if (nv == 0) {
    if (widths) widths[0] = 0;
    return 1;
  }
  int passes = 0;
  const int first = nv % MLE_TILE_LOG ? nv % MLE_TILE_LOG : MLE_TILE_LOG;
  for (int left = nv, w = first; left > 0; left -= w, w = MLE_TILE_LOG) {
    if (widths) widths[passes] = w;
    passes++;
  }
  return passes;
}
// tiles per wave (log2) of a launch that writes 2^m outputs: the most that still leaves 2^MLE_MIN_WAVES_LOG waves
static inline int mle_eq_group_log(int m) {
  int gl = m - MLE_TILE_LOG - MLE_MIN_WAVES_LOG;
  if (gl < 0) gl = 0;
  return gl > MLE_EQ_MAX_GROUP_LOG ? MLE_EQ_MAX_GROUP_LOG : gl;
}

// dst[t 512 + i] = hi[t] prod_{j < 9} (bit j of i ? pt.r[j] : 1 - pt.r[j]) for t 512 + i < n_out; hi == nullptr: one tile, and
// `top` (unit: one) stands for hi[0].  A launch of fewer than 9 variables gets zeros for the missing r[j]: their factor is
// one where the bit is clear, and the outputs where it is set lie past n_out.
template <class F>
__global__ void __launch_bounds__(64) mle_eq_kernel(const char* __restrict__ hi, FrConst top, int unit, MlePoint pt, size_t n_out, int gl,
                                                    char* __restrict__ dst) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  const u32 lane = threadIdx.x;
  F w[MLE_E];
  {
    const F r0 = fr_from_const<F>(pt.r[0]);
    w[0] = mle_pick<F>(lane & 1, r0, F::sub(F::one(), r0));
  }
#pragma unroll
  for (int j = 1; j < MLE_LANE_LOG; j++) {
    const F t = F::mul(w[0], fr_from_const<F>(pt.r[j]));
    w[0] = mle_pick<F>((lane >> j) & 1, t, F::sub(w[0], t));
  }
#pragma unroll
  for (int a = 0; a < MLE_TILE_LOG - MLE_LANE_LOG; a++) {
    const F r = fr_from_const<F>(pt.r[MLE_LANE_LOG + a]);
#pragma unroll
    for (int t = 0; t < (1 << a); t++) {
      w[t + (1 << a)] = F::mul(w[t], r);
      w[t] = F::sub(w[t], w[t + (1 << a)]);
    }
  }
#pragma unroll 1
  for (int g = 0; g < (1 << gl); g++) {
    const size_t tile = ((size_t)blockIdx.x << gl) + (u32)g;
    if ((tile << MLE_TILE_LOG) >= n_out) break;
    F h = unit ? F::one() : fr_from_const<F>(top);
    if (hi) h = F::load(hi + tile * F::BYTES);
#pragma unroll
    for (int k = 0; k < MLE_E; k++) {
      const size_t o = (tile << MLE_TILE_LOG) + (u32)k * 64 + lane;
      if (o < n_out) F::mul(h, w[k]).store(dst + o * F::BYTES);
    }
  }
}

// writes the 2^m outputs of one launch (m <= 62; hi: 2^(m-9) elements when m > 9, else nullptr)
template <class F>
int mle_eq_launch(const void* hi, const FrConst& top, int unit, const MlePoint& pt, int m, void* dst, hipStream_t s) {
  if (m < 0 || m > 62 || (m > MLE_TILE_LOG) != (hi != nullptr)) return -1000;
  const int gl = mle_eq_group_log(m);
  const size_t tiles = m > MLE_TILE_LOG ? (size_t)1 << (m - MLE_TILE_LOG) : 1;
  const size_t waves = tiles >> gl;
  if (waves == 0 || waves > 0x7fffffffu) return -1000;
  hipLaunchKernelGGL((mle_eq_kernel<F>), dim3((unsigned)waves), dim3(64), 0, s, (const char*)hi, top, unit, pt, (size_t)1 << m, gl,
                     (char*)dst);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// binds the WB lowest index bits of the 2^m = n elements of src (m >= WB) as mle_fold_kernel does, in order, and stores the
// differences: those of bit j are the n >> (j+1) elements from element n - (n >> j) of quot.  src, quot and dst do not overlap.
template <class F, int WB>
__global__ void __launch_bounds__(64) mle_quot_kernel(const char* __restrict__ src, size_t n, MlePoint pt, char* __restrict__ quot,
                                                      char* __restrict__ dst) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  static_assert(WB >= 1 && WB <= MLE_TILE_LOG, "a launch binds 1 .. 9 bits");
  constexpr int SLOT_LOG = MLE_TILE_LOG - MLE_LANE_LOG;   // index bits held by the register slot
  constexpr int NA = WB < SLOT_LOG ? WB : SLOT_LOG;       // bits bound between registers
  constexpr int NB = WB - NA;                             // bits bound across lanes
  const u32 lane = threadIdx.x;
  const size_t e0 = ((size_t)blockIdx.x << MLE_TILE_LOG) + lane * (u32)MLE_E;
  F x[MLE_E];
#pragma unroll
  for (int k = 0; k < MLE_E; k++) {
    x[k] = F::zero();
    if (e0 + (u32)k < n) x[k] = F::load(src + (e0 + (u32)k) * F::BYTES);
  }
#pragma unroll
  for (int a = 0; a < NA; a++) {
    const F r = fr_from_const<F>(pt.r[a]);
    char* seg = quot + (n - (n >> a)) * F::BYTES;
    const size_t nseg = n >> (a + 1), q0 = e0 >> (a + 1);
#pragma unroll
    for (int t = 0; t < (MLE_E >> (a + 1)); t++) {
      const F d = F::sub(x[2 * t + 1], x[2 * t]);
      if (q0 + (u32)t < nseg) d.store(seg + (q0 + (u32)t) * F::BYTES);
      x[t] = F::add(x[2 * t], F::mul(r, d));
    }
  }
  const size_t n_out = n >> WB;
  if (NB == 0) {
#pragma unroll
    for (int t = 0; t < (MLE_E >> NA); t++) {
      const size_t o = (e0 >> WB) + (u32)t;
      if (o < n_out) x[t].store(dst + o * F::BYTES);
    }
    return;
  }
  const size_t v0 = e0 >> SLOT_LOG;   // this lane's index among the n / 8 values phase A left
  F y = x[0];
#pragma unroll
  for (int j = 0; j < NB; j++) {
    const bool up = (lane >> j) & 1;
    const F r = fr_from_const<F>(pt.r[SLOT_LOG + j]);
    const F got = mle_lane_xor<F>(y, 1 << j);
    const F lo = mle_pick<F>(up, got, y), hi = mle_pick<F>(up, y, got);
    const F d = F::sub(hi, lo);
    const size_t q = v0 >> (j + 1);
    if ((lane & ((2u << j) - 1)) == 0 && q < (n >> (SLOT_LOG + j + 1))) d.store(quot + (n - (n >> (SLOT_LOG + j)) + q) * F::BYTES);
    y = F::add(lo, F::mul(r, d));
  }
  const size_t o = v0 >> NB;
  if ((lane & ((1u << NB) - 1)) == 0 && o < n_out) y.store(dst + o * F::BYTES);
}

template <class F, int WB>
int mle_quot_launch_one(const void* src, int m, const MlePoint& pt, void* quot, void* dst, hipStream_t s) {
  const size_t n = (size_t)1 << m;
  const size_t waves = m > MLE_TILE_LOG ? n >> MLE_TILE_LOG : 1;
  if (waves > 0x7fffffffu) return -1000;
  hipLaunchKernelGGL((mle_quot_kernel<F, WB>), dim3((unsigned)waves), dim3(64), 0, s, (const char*)src, n, pt, (char*)quot, (char*)dst);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
// binds the w lowest index bits of the 2^m elements of src (1 <= w <= min(m, MLE_TILE_LOG)) with pt.r[0 .. w-1]
template <class F>
int mle_quot_launch(const void* src, int m, int w, const MlePoint& pt, void* quot, void* dst, hipStream_t s) {
  if (w < 1 || w > MLE_TILE_LOG || w > m || m > 62) return -1000;
#define ARK_MLE_CASE(WB) \
  if (w == WB) return mle_quot_launch_one<F, WB>(src, m, pt, quot, dst, s);
  ARK_MLE_CASE(1) ARK_MLE_CASE(2) ARK_MLE_CASE(3) ARK_MLE_CASE(4) ARK_MLE_CASE(5) ARK_MLE_CASE(6) ARK_MLE_CASE(7) ARK_MLE_CASE(8)
  ARK_MLE_CASE(9)
#undef ARK_MLE_CASE
  return -1000;
}

}  // namespace arkhip
