// Host-side planning of the MSM pipeline (msm.cuh): the window plan, the geometry of the partition sort and of the bucket
// reduction, run parts, window groups -- and every ARK_HIP_MSM_* environment knob.  Pure functions of their arguments: no
// HIP, no device; a plain C++17 compiler builds this header, and tests/test_msm_geometry_host.py reaches it without a GPU.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "params.hpp"

#if defined(__HIP__)
#define ARK_PLAN_HD __host__ __device__ __forceinline__
#else
#define ARK_PLAN_HD inline
#endif

namespace arkhip {
typedef uint32_t u32;

// ---- environment knobs ---------------------------------------------------------------------------
// msm_knobs() is the only reader of an ARK_HIP_MSM_* variable (and of ARK_HIP_PLAN_DEBUG).  A default-constructed MsmKnobs
// is the library with nothing set.  "once": read at the first call of the process; "per call": read at every call (tests
// and sweeps set these in-process).  INTEGRATION.md section 5 tabulates the same fields.
struct MsmKnobs {
  bool lazy = true;              // once      ARK_HIP_MSM_LAZY=0: the saturated accumulate kernels on every curve (A/B reference)
  bool probe = true;             // once      ARK_HIP_MSM_PROBE=0: no width probe (K0), device and streamed entries
  bool compact = true;           // once      ARK_HIP_MSM_COMPACT=0: zero scalars stay in the pipeline (no K0c)
  bool heavy_side = true;        // once      ARK_HIP_MSM_HEAVY_SIDE=0: the heavy-run kernels stay in line on the MSM stream
  bool big_slices = true;        // once      ARK_HIP_MSM_BIG_SLICES=0: no sliced pass B for oversized super-buckets
  bool plan_debug = false;       // once      ARK_HIP_PLAN_DEBUG (set): the cost model's terms per candidate c, on stderr
  int groups = 0;                // once      ARK_HIP_MSM_GROUPS=1 / 2: force the number of window groups (0: by n)
  int split_level = -1;          // once      ARK_HIP_MSM_SPLIT_LEVEL=0 / non-zero: force the one-lane / two-wave level-0 kernel (-1: by size)
  size_t parts_lanes = 262144;   // once      ARK_HIP_MSM_PARTS_LANES: lanes the split runs may fill (0: never split runs)
  int c = 0;                     // per call  ARK_HIP_MSM_C=3 .. 26: window bits of a plain MSM (0: the cost model)
  int c_prepared = 0;            // per call  ARK_HIP_MSM_C_PREPARED=3 .. 26: window bits of a prepared base set
  int l0 = 0;                    // per call  ARK_HIP_MSM_L0=1 .. 128: level-0 chunk length of the reduction (0: the rules)
  int stage2 = -1;               // per call  ARK_HIP_MSM_STAGE2=0 / 1: one-kernel / two-digit second stage (-1: by m)
  int chunk = 0;                 // per call  ARK_HIP_MSM_CHUNK=256 .. 16384 (a power of two): chunk of the one-kernel second stage
  int heavy = 0;                 // per call  ARK_HIP_MSM_HEAVY>=64: heavy-run threshold (0: computed on the device)
  int hb = -1;                   // per call  ARK_HIP_MSM_HB: super-bucket bits of sort pass A, where the window allows them
  int tile = 0;                  // per call  ARK_HIP_MSM_TILE=8192 / 16384: keys per workgroup of sort pass A
  int run_parts = 0;             // per call  ARK_HIP_MSM_RUN_PARTS=1 / 2 / 4 / 8: lanes per (window, bucket) run
};

inline MsmKnobs msm_knobs() {
  const auto first_char = [](const char* name) { const char* e = getenv(name); return e ? e[0] : '\0'; };
  const auto number = [](const char* name, long unset) { const char* e = getenv(name); return e ? atol(e) : unset; };
  const auto within = [](long v, long lo, long hi) { return v >= lo && v <= hi ? (int)v : 0; };
  static const MsmKnobs once = [&] {
    MsmKnobs k;
    k.lazy = first_char("ARK_HIP_MSM_LAZY") != '0';
    k.probe = number("ARK_HIP_MSM_PROBE", 1) != 0;
    k.compact = first_char("ARK_HIP_MSM_COMPACT") != '0';
    k.heavy_side = number("ARK_HIP_MSM_HEAVY_SIDE", 1) != 0;
    k.big_slices = number("ARK_HIP_MSM_BIG_SLICES", 1) != 0;
    k.plan_debug = getenv("ARK_HIP_PLAN_DEBUG") != nullptr;
    k.groups = (int)number("ARK_HIP_MSM_GROUPS", 0);
    k.split_level = (int)number("ARK_HIP_MSM_SPLIT_LEVEL", -1);
    k.parts_lanes = (size_t)number("ARK_HIP_MSM_PARTS_LANES", 262144);
    return k;
  }();
  MsmKnobs k = once;
  k.c = within(number("ARK_HIP_MSM_C", 0), 3, 26);
  k.c_prepared = within(number("ARK_HIP_MSM_C_PREPARED", 0), 3, 26);
  k.l0 = within(number("ARK_HIP_MSM_L0", 0), 1, 128);
  const char s2 = first_char("ARK_HIP_MSM_STAGE2");
  k.stage2 = s2 == '0' ? 0 : (s2 == '1' ? 1 : -1);
  const long chunk = number("ARK_HIP_MSM_CHUNK", 0);
  k.chunk = (chunk & (chunk - 1)) == 0 ? within(chunk, 256, 16384) : 0;
  k.heavy = within(number("ARK_HIP_MSM_HEAVY", 0), 64, 0x7fffffff);
  k.hb = (int)number("ARK_HIP_MSM_HB", -1);
  k.tile = (int)number("ARK_HIP_MSM_TILE", 0);
  const long rp = number("ARK_HIP_MSM_RUN_PARTS", 0);
  k.run_parts = (rp & (rp - 1)) == 0 ? within(rp, 1, 8) : 0;
  return k;
}

// ---- scalar width classes (K0, msm.cuh) ------------------------------------------------------------
static constexpr int MSM_WIDTH_CLASSES = 9;
static constexpr int MSM_WIDTH_TOP[MSM_WIDTH_CLASSES] = {0, 1, 8, 16, 32, 64, 128, 192, 256};   // class k: TOP[k-1] < b <= TOP[k]
struct MsmWidths {
  u32 max_bits;
  u32 count[MSM_WIDTH_CLASSES];
};
// true when the classes say "not n uniform full-width scalars": fewer than half wider than 128 bits
static inline bool msm_widths_skewed(const MsmWidths& w) {
  uint64_t seen = 0, wide = 0;
  for (int k = 0; k < MSM_WIDTH_CLASSES; k++) {
    seen += w.count[k];
    if (MSM_WIDTH_TOP[k] > 128) wide += w.count[k];
  }
  return 2 * wide < seen;
}

// ---- window plan -----------------------------------------------------------------------------------
struct MsmPlan {
  int c;          // window bits (widest windows)
  int W;          // windows
  int narrow;     // the top `narrow` windows are c-1 bits wide, so that the widths sum to bits exactly and no
                  // window is left with only a few significant bits (0: uniform widths)
  size_t nb;      // bucket slots of the sort = W << (c-1)
  bool shared;    // prepared base set: the W windows share one set of 2^(c-1) buckets
  unsigned parts = 0;   // small plain MSMs: lanes per (window, bucket) run the accumulate kernel should use (0: its own rule)
  size_t nbuckets() const { return shared ? ((size_t)1 << (c - 1)) : nb; }
  int red_windows() const { return shared ? 1 : W; }
};

// relative cost of one mixed addition (Fp384 G1 = 1): Fp256 ~0.5; Fp2 over Fp384 2.7 (measured: 0.49 ns against
// 0.18 ns per addition at full occupancy)
static inline double msm_mul_cost(int curve_id) { return curve_id == 0 ? 0.5 : (curve_id >= 3 ? 2.7 : 1.0); }
// lanes that hold one point of the accumulate field: one (G1), a lane pair (G2, Fp2)
static inline u32 msm_lanes_per_point(int curve_id) { return curve_id >= 3 ? 2u : 1u; }
static inline int msm_scalar_bits(int curve_id) {
  switch (curve_id) {
    case 0: return BN254_FR::BITS;
    case 1: case 4: return BLS12_381_FR::BITS;
    default: return BLS12_377_FR::BITS;
  }
}

// Window widths: W windows of c bits, except that the top `narrow` windows are c-1 bits wide, so that the widths
// add up to the scalar's bit length exactly and no window is left with only a few significant bits.
ARK_PLAN_HD int msm_window_width(int w, int c, int W, int narrow) {
  return w >= W - narrow ? c - 1 : c;
}
static inline void msm_window_layout(int c, int bits, int* W, int* narrow) {
  // signed digits of a (bits-1)-bit value (after the s -> r-s fold) need bits significant positions in total
  // (the top window is not recoded and must keep one spare bit).  W windows of c bits, the top `narrow` of them
  // one bit narrower so that the widths add up exactly.
  int w = (bits + c - 1) / c;
  int deficit = w * c - bits;
  if (deficit > w || c < 3) {  // cannot be spread one bit per window: uniform widths, sparse top window
    *W = (bits + 1 + c - 1) / c;
    *narrow = 0;
    return;
  }
  *W = w;
  *narrow = deficit;
}

// Window size.  Model (seconds) of the phases that depend on c, from this chip's measured rates
// (profiles/): mixed additions stream at ~5.5e9/s (Fp384; scaled by `mul_cost` for other fields) but a
// single bucket is a serial chain (~14 us per addition on a lightly loaded SIMD), the first reduction
// level costs 2 full additions per bucket, the bit-sliced remainder ~0.5 ms.  With a prepared base set
// (`shared`) only one bucket set is reduced, which moves the optimum to wider windows.
// Every served curve accumulates on carry-free limbs, so the G1 terms below are those kernels' (the saturated ones of
// ARK_HIP_MSM_LAZY=0 are a reference, planned like the shipped ones).
static inline MsmPlan msm_make_plan(size_t n, int bits, double mul_cost, bool shared, const MsmWidths* widths, bool split_runs,
                                    const MsmKnobs& knobs) {
  int best_c = 3;
  double best = 1e300;
  const int forced_c = shared ? knobs.c_prepared : knobs.c;
  if (forced_c) {
    best_c = forced_c;
  } else {
    // c <= bits: a window wider than the scalar only adds empty buckets to sort and reduce (msm_u16 at 2^24: the model's
    // c = 19 took 8.2 ms, c = 17 -- one window of exactly the 2^16 buckets the digits reach -- 4.1 ms;
    // profiles/r4_narrow_scalars.txt)
    const int c_max = shared ? 25 : 23;
    for (int c = 3; c <= (bits < c_max ? (bits < 3 ? 3 : bits) : c_max); c++) {
      int W, narrow;
      msm_window_layout(c, bits, &W, &narrow);
      double nbk = (double)(W - narrow) * (double)(1u << (c - 1)) + (double)narrow * (double)(1u << (c - 2));
      if (shared) nbk = (double)(1u << (c - 1));
      double entries = (double)n * W;
      if (widths) {
        // measured width classes (K0): a scalar of b bits has digits in the windows below bit b + 1 only
        entries = 0.0;
        for (int k = 1; k < MSM_WIDTH_CLASSES; k++) {
          int need = (MSM_WIDTH_TOP[k] + 1 + c - 1) / c;
          if (need > W) need = W;
          entries += (double)widths->count[k] * need;
        }
        if (entries < 1.0) entries = 1.0;
      }
      const double madd = 1.0 / 5.5e9 * mul_cost, fadd = 1.4 / 5.5e9 * mul_cost;
      const bool fp2 = mul_cost > 2.0;  // a lane PAIR per bucket
      // accumulate: throughput-bound when the buckets make several rounds over the chip's resident lanes (2 waves x 4
      // SIMDs x 256 CUs x 64 lanes; a G2 bucket takes a lane pair); with a single round the kernel lasts as long as
      // its most loaded lane (Poisson tail): ~24 us per addition on a fully occupied SIMD, ~14 us with one wave per SIMD
      // (profiles/r2_small_n_sweep.txt)
      double acc = entries * madd;
      if (shared) {
        const double lanes = 131072.0 / (fp2 ? 2.0 : 1.0);
        const double load = entries / nbk, lmax = load + 3.0 * sqrt(load) + 2.0;
        // one dependent addition: a wave alone on its SIMD runs a chain faster; over Fp2 ~30 us whatever the occupancy
        // (BLS12-377 G2 2^16, c = 15 / 16 / 17: 25 / 28 / 31 us -- profiles/r2_msm_sweeps.txt)
        const double per_add = fp2 ? 30e-6 : (nbk <= lanes / 2 ? 14e-6 : 24e-6) * mul_cost;
        const double walk = lmax * per_add + W * 5e-6;                          // + run switches of a shared bucket
        if (nbk <= lanes || walk > acc) acc = walk;
      } else if (fp2) {
        // G2 plain path on the carry-free lane-pair kernels, fitted on BLS12-377 G2 2^16 / 2^20 / 2^22, c = 13 .. 21
        // (profiles/r4_planner_sweeps.txt): 0.40 ns per entry, rising for narrow windows (c = 15: 0.47, c = 14: 0.63); one
        // lane pair walks one (window, bucket) run at 38 us per dependent addition, the most loaded run sets the floor
        acc = entries * 0.40e-9 * (1.0 + ldexp(1.0, 13 - c));
        const double load = entries / nbk;
        const double chain = (load + 3.0 * sqrt(load) + 2.0) * 38e-6;
        if (chain > acc) acc = chain;
      } else {
        // G1 on carry-free limbs (round 3; BN254 since round 4, scaled by its mul_cost): 7.0e9 instead of 5.5e9 mixed
        // additions/s (the factor 0.79 below).
        // One lane walks one (window, bucket) run, and the kernel lasts at least as long as its most loaded lane: measured
        // 19 us per dependent addition for BLS12-381 whatever the occupancy (2^15 / 2^16, mean loads 2 .. 128:
        // profiles/r3_window_sweep.txt), 14-18 us for BN254.
        const double load = entries / nbk;
        // (round 5, profiles/r5_window_sweep_mid_sizes.txt) the first point of a bucket is a copy, not an addition:
        // entries - occupied buckets additions (2^19, c = 16 / 17: 7.86e6 / 6.88e6 additions in 1.13 / 1.00 ms; 2^20, c = 17:
        // 1.475e7 in 2.07 ms), and a launch of only ~2 rounds over the chip's 131 072 resident lanes pays for its ragged last
        // round: c = 15 (2.78e5 lanes) runs 5-9 % over the rate at 2^18 / 2^19 where c = 16 (four rounds) and wider match it
        // That saving is there while the bucket array stays in the 256 MB last-level cache (<= ~1e6 buckets of 192 B); beyond,
        // a bucket's first touch and its store cost what the copy saves (2^22: c = 19 / 20, 2.2e6 / 5.5e6 buckets, run at
        // 6.5e9 entries/s against c = 17's 6.8e9): the credit fades out between 1e6 and 4e6 buckets.
        const double rounds = nbk / 131072.0;
        const double credit = nbk <= 1e6 ? 1.0 : (nbk >= 4e6 ? 0.0 : (4e6 - nbk) / 3e6);
        acc = (entries - credit * nbk * (1.0 - exp(-load))) * madd * 0.79 * (rounds >= 1.0 ? 1.0 + 0.3 / (rounds * rounds) : 1.0);
        const double lmax = load + 3.0 * sqrt(load) + 2.0;
        // one dependent addition: 19 us on 14 x 28-bit limbs, 13.5 us on BN254's 9 x 29 (2^17, c = 15 / 16: 0.24 / 0.165 ms)
        const double chain = lmax * (mul_cost < 1.0 ? 13.5e-6 : 19e-6);
        if (chain > acc) acc = chain;
        if (!widths && (narrow > 0 || W * c == bits)) {
          // the TOP window: scalars below r (folded below r / 2) reach only r / 2^bits of its buckets -- 0.58 for BLS12-377's
          // r = 0x12ab..., 0.76 for BN254's, 0.91 for BLS12-381's -- so its runs are that much longer than the layout says and,
          // sorted to the front, are what the kernel's last waves are still walking: ~11 us per dependent addition once few
          // waves are left (BLS12-377 G1 2^18: accumulate 0.89 ms with c = 15, 0.57 with c = 16, where BLS12-381 takes 0.63 /
          // 0.55; 2^17: 0.51 / 0.32; 2^16, c = 14: 0.47 against 0.36)
          const double frac = bits == 253 ? 0.583 : (bits == 254 ? 0.756 : (bits == 255 ? 0.906 : 1.0));
          const int wt = narrow > 0 ? c - 1 : c;
          const double load_top = (double)n / (frac * ldexp(1.0, wt - 1));
          const double chain_top = (load_top + 3.0 * sqrt(load_top) + 2.0) * 11e-6 * (mul_cost < 1.0 ? 0.7 : 1.0);
          if (chain_top > acc) acc = chain_top;
        }
      }
      // level 0 of the reduction: 2 full additions per bucket; over Fp2 with ONE bucket set (a lane PAIR per bucket: half
      // the lanes, the same chain length) the kernels run at ~40 % of the addition throughput (measured: BLS12-377 G2 2^16, 2^18 buckets 1.7 ms,
      // 2^16 buckets 0.76 ms; 2^22, 2^19 buckets 2.2 ms -- profiles/r2_msm_sweeps.txt)
      double red0 = nbk * 2.0 * fadd * (fp2 && shared ? 2.5 : 1.0);
      const double red0_lat = (fp2 && shared) ? 0.6e-3 : 2.0 * 8.0 * 21e-6 * mul_cost;  // latency floor of the reduction (G2: measured 0.62-0.76 ms for 2^12..2^16 buckets)
      if (red0_lat > red0) red0 = red0_lat;
      double bits_stage = 0.5e-3 * mul_cost;                    // bit-sliced stage + host tail
      if (!shared && fp2) {
        // measured reduction of the plain G2 path: 0.45 ms + 2.6 ns per bucket up to ~10^6 buckets (short level-0 chunks: the
        // bit-sliced stage is almost half of it), 1.25 ns per bucket beyond (same sweeps)
        // (round 5 refit, profiles/r5_g2_window_sweep.txt: the lane-pair kernels of round 4 reduce 1.97e6 buckets in 4.6 ms,
        // 4.98e6 in 10.6, 1.36e7 in 23 -- 1.7 ns per bucket beyond the first 1.2e6, not the 1.25 of the saturated kernels this
        // line was fitted on; the old figure made c = 19 look 1.7 ms cheaper than it is and cost BLS12-377 G2 2^20 14 %)
        // (the L0 = 16 rule of the same round made 2.8e5 .. 9.8e5 buckets 0.3-0.5 ms cheaper than this line says; a refit on that moved
        // 2^20 to c = 17 and lost 8 % on BLS12-381 G2 -- 9.72 against 8.98 ms, profiles/r5_window_sweep_mid_sizes.txt -- so it stays)
        red0 = 0.45e-3 + (nbk < 1.2e6 ? nbk : 1.2e6) * 2.6e-9 + (nbk > 1.2e6 ? nbk - 1.2e6 : 0.0) * 1.7e-9;
        bits_stage = 0.0;
      }
      if (!shared && !fp2) {
        // plain path, fitted on BLS12-381 2^16 .. 2^24 (profiles/r3_window_sweep.txt): 0.2 ms + 0.45 ns per bucket
        // + 1.4 ns per bucket for the first 3e5 (few buckets leave the chip's lanes idle, the chains dominate)
        // (round 5 refit on the split-level kernels, BLS12-381 G1: 1.56e5 buckets 0.43 ms, 2.8e5 0.54, 5.2e5 0.65-0.71, 9.8e5
        // 0.95, 3.7e6 2.1, 6.8e6 3.6; BN254 half of that: 0.40 ms + 0.47 ns per bucket + 0.10 ns for the first 1e6.  The older
        // fit -- 0.2 ms + 0.40 ns + 1.4 ns for the first 3e5 -- was 0.1 ms high between 3e5 and 1e6 buckets, 0.25 ms low at 6.8e6)
        // Counted half way between the occupied slots and W 2^(c-1): the reduction walks every window at full width, and the
        // empty upper half of a narrow one costs it its lanes' launch and barriers but no additions (2^23, c = 19: 2.09 ms with
        // 11 of 14 windows narrow on BLS12-381, 1.67 with 13 of 14 on BLS12-377; c = 18, uniform, 1.26)
        const double nred = 0.5 * (nbk + (double)W * ldexp(1.0, c - 1));
        red0 = (nred * 0.47e-9 + (nred < 1e6 ? nred : 1e6) * 0.10e-9) * mul_cost;
        bits_stage = 0.40e-3 * mul_cost;
      }
      // partition sort: per entry, plus a per-(window, bucket) term.  On the shared path at n >= 2^23 the latter is
      // measured nearly flat up to c = 22 (9 super-bucket bits + 12 bits finished in LDS, msm_part_split); beyond that the
      // super-bucket histogram grows and so do both sort passes (2^25: c = 24 costs +2.8 ms of sort and +7 ms of
      // reduction for -4.7 ms of accumulation; BN254 2^23 / 2^24: c = 22 beats 20 by 6-7 %; profiles/r2_msm_sweeps.txt)
      const double per_bucket = (shared && n >= ((size_t)1 << 23) && c <= 22) ? 1.5e-11 : 1.0e-10;
      const double sort = (double)n * W * 2.0e-11 + (double)W * (double)(1u << (c - 1)) * per_bucket;   // every key is read, live or not
      double cost = acc + red0 + bits_stage + sort;
      if (narrow == W) continue;  // every window one bit narrower: the layout of c - 1 with twice the buckets
      if (narrow == 0) {
        // uniform widths: a top window with only a few significant bits funnels n/2^tb points into each of 2^tb
        // buckets: correct (heavy-bucket path) but measured ~1.4x slower on the plain path and ~2x on a prepared set
        // (BLS12-377 G2 2^16: c = 18 3.7 ms against 1.9 ms at c = 17; 2^24 G1: c = 21, 23)
        const int tb = (bits - 1) - (W - 1) * c;
        if (tb >= (shared ? 0 : 1) && tb <= 5) cost *= shared ? 2.0 : 1.4;
        // narrow scalars (two to five windows): a top window that is more than two bits short of full is a large share
        // of the work and loses more -- msm_u32 with c = 18 (18 + 15 bits) 12.5 ms at 2^24 against 8.8 ms for the exact
        // 17 + 16 layout; only a top window that holds nothing but the carry bit (tb = 0: one heavy bucket) is cheap
        else if (!shared && !fp2 && bits <= 129 && tb > 5 && tb < c - 3) cost *= 1.4;
      }
      if ((size_t)n * (size_t)W >= (1ull << 32)) continue;  // 32-bit sort positions
      if (knobs.plan_debug)
        fprintf(stderr, "plan n=%zu c=%d W=%d narrow=%d: accumulate %.3f reduce %.3f + %.3f sort %.3f -> %.3f ms\n", n, c, W, narrow,
                acc * 1e3, red0 * 1e3, bits_stage * 1e3, sort * 1e3, cost * 1e3);
      if (cost < best) { best = cost; best_c = c; }
    }
  }
  unsigned parts = 0;
  if (split_runs && !shared && !widths && bits > 128 && !forced_c) {
    // Small plain MSMs (round 5, profiles/r5_small_n_run_parts.txt).  Below ~2^17 pairs the accumulate kernel lasts as long as
    // its most loaded bucket (a Poisson tail of dependent additions at ~17 us each) and the model above answers with wide
    // windows -- few points per bucket, many buckets to reduce.  Narrower windows with every run walked by 4 or 8 lanes
    // (msm_accumulate_parts_kernel: the chain is cut, the pieces are summed by msm_sum_parts_kernel) win on both sides:
    // BLS12-381 G1 2^16 c = 14 -> 12: reduce 0.43 -> 0.27 ms, accumulate 0.36 -> 0.40, call 1.11 -> 0.99 ms; 2^14 0.91 -> 0.79;
    // 2^12 0.80 -> 0.71; 2^8 0.69 -> 0.60; BN254 2^16 0.67 -> 0.60; BLS12-377 G2 2^14 2.00 -> 1.61, 2^12 1.74 -> 1.39.
    // From 2^17 (G2: 2^16) the model's choice with one lane per run is the faster one again.  BLS12-377 G1 leaves the rule at
    // 2^15 already (1.09 against 1.07 ms, 2^16 1.29 against 1.22; 2^14 0.81 against 0.99): r = 0x12ab... x 2^240 fills only
    // 0.58 of its top window's buckets, whose runs are then twice as long as anybody else's and set the kernel's time.
    // (ARK_HIP_MSM_C, ARK_HIP_MSM_L0 and ARK_HIP_MSM_RUN_PARTS force any other cell for a sweep.)
    const bool fp2 = mul_cost > 2.0;
    int logn = 0;
    while (((size_t)1 << logn) < n) logn++;
    if (n >= 256 && n <= (fp2 ? (size_t)24576 : bits == 253 ? (size_t)20480 : (size_t)73728)) {
      const int cap = fp2 ? 11 : 12;
      best_c = logn - 2 < cap ? logn - 2 : cap;
      parts = (!fp2 && (n >> (best_c - 1)) >= 32) ? 8u : 4u;
    }
  }
  MsmPlan p;
  p.c = best_c;
  p.shared = shared;
  p.parts = parts;
  msm_window_layout(best_c, bits, &p.W, &p.narrow);
  p.nb = (size_t)p.W << (best_c - 1);
  return p;
}

// THE plan of curve `curve_id` for n scalars of `bits` bits: what every entry point, ark_hip_msm_plan and the streamed
// pieces use.  shared: a prepared base set.  widths: measured width classes of a plain MSM (nullptr: n uniform scalars).
// Small plain MSMs count on split runs (msm_make_plan), which only the carry-free kernels have and which the pieces of a
// streamed MSM (`streamed`) never take.
static inline MsmPlan msm_default_plan(int curve_id, size_t n, int bits, bool shared, const MsmWidths* widths,
                                       const MsmKnobs& knobs = msm_knobs(), bool streamed = false) {
  return msm_make_plan(n, bits, msm_mul_cost(curve_id), shared, widths, !shared && !streamed && knobs.lazy, knobs);
}

// plan of a plain MSM whose width classes were MEASURED over all n scalars (msm_enqueue after K0; ark_hip_msm_plan_widths):
// windows for the widest scalar unless fewer than 8 bits would be saved, window size from the digits the classes have
static inline MsmPlan msm_plan_for_widths(int curve_id, size_t n, const MsmWidths& w, const MsmKnobs& knobs = msm_knobs()) {
  const int slack = 8, field_bits = msm_scalar_bits(curve_id);
  int bits = field_bits;
  if ((int)w.max_bits + 1 + slack <= field_bits) bits = (w.max_bits ? (int)w.max_bits : 1) + 1;
  return msm_default_plan(curve_id, n, bits, false, &w, knobs);
}

// ---- geometry of the partition sort (msm_sort.cuh) and of the bucket order pass -----------------------
static constexpr int PART_LO_BITS = 10;        // buckets per super-bucket = 2^10 by default (2^9 measured no better) ...
static constexpr int PART_LO_BITS_MAX = 12;    // ... up to 2^12 where the window is wide (msm_part_split)
static constexpr u32 PART_LDS_WORDS = (160 * 1024 - 64) / 4;  // dynamic LDS of the finish kernel, u32 words
static constexpr int PART_TILE = 8192;         // keys per workgroup in pass A (64 KiB of staged pairs) ...
static constexpr int PART_TILE_BIG = 16384;    // ... 128 KiB where pass A has >= 2^11 super-buckets (n >= 2^26): the per-tile
                                               // histogram array halves and the runs a tile writes per super-bucket double
                                               // (2^26, c = 22: 4 entries = 32 B per run with 8192 keys)
static constexpr size_t PART_SCATTER_LDS_MAX = 160 * 1024 - 4096 - 64;   // dynamic LDS the scatter kernel may ask for
static constexpr u32 PART_BIG = 1u << 17;      // entries above which a super-bucket is finished in slices (msm_sort.cuh)
static constexpr int SCAN_TILE = 2048;         // elements per block of the scan kernels (256 threads x 8)
static constexpr int ORDER_TILE = 2048;
static constexpr int ORDER_BINS = 256;

// Split of the B = c-1 bucket bits into HB super-bucket bits (pass A) and LB bits finished in LDS (pass B).  Pass A
// keeps 2^HB counters per (window, 8192-key tile): its histogram array -- W * 2^HB * n/8192 counters, written and
// scanned in bin-major order -- is what grows with wide windows, so HB is kept as small as pass B allows: a
// super-bucket (n / 2^HB entries on average) must fit the finish kernel's LDS staging area (~32 K entries) and has at
// most 2^12 buckets.
static inline void msm_part_split(size_t n, int B, int* HB, int* LB, const MsmKnobs& knobs) {
  int hb = 0;
  if (B > PART_LO_BITS) {
    hb = B - PART_LO_BITS;                       // 2^10 buckets per super-bucket ...
    if (hb > 9) {                                // ... unless that needs more than 2^9 counters per tile
      hb = B - PART_LO_BITS_MAX;
      if (hb < 9) hb = 9;
    }
    int lg = 0;
    while (((size_t)1 << lg) < n) lg++;
    if (hb < lg - 15) hb = lg - 15;              // super-bucket (n / 2^hb entries) within the LDS staging area
    if (hb > B) hb = B;
    const int v = knobs.hb;                      // tuning knob (tools/): super-bucket bits of pass A
    if (v >= 0 && v <= B && B - v <= PART_LO_BITS_MAX) hb = v;
  } else {
    // few buckets per window (narrow scalars: msm_u8 plans ONE window of 2^8): still split, or a single workgroup of
    // pass B finishes the whole window (2^24 keys through one CU)
    int lg = 0;
    while (((size_t)1 << lg) < n) lg++;
    hb = lg - 15;
    if (hb < 0) hb = 0;
    if (hb > B) hb = B;
  }
  *HB = hb;
  *LB = B - hb;
}
// staging entries of the finish kernel for a given LB
static inline u32 msm_part_stage_cap(int LB) { return PART_LDS_WORDS - 1024u - (1u << LB) - 16u; }
static inline u32 msm_part_tile(int HB, const MsmKnobs& knobs) {
  // the big tile must fit the scatter kernel's LDS beside its 2 x 2^HB counters (HB = 11: 16 + 128 KiB; from HB = 12,
  // i.e. n >= 2^27, it does not -- 32 + 128 KiB -- and the 8192-key tile stays)
  const bool fits = ((size_t)8 << HB) + (size_t)PART_TILE_BIG * 8 <= PART_SCATTER_LDS_MAX;
  if (knobs.tile == PART_TILE || (knobs.tile == PART_TILE_BIG && fits)) return (u32)knobs.tile;   // tuning knob
  return (HB >= 11 && fits) ? (u32)PART_TILE_BIG : (u32)PART_TILE;
}

struct MsmSortGeom {
  int HB, LB;            // bucket-id split of the two-pass partition sort
  u32 nsuper;            // super-buckets of all windows = W << HB
  u32 tile, ntiles;      // keys per workgroup of pass A, workgroups per window
  size_t nthist;         // pass A's histogram cells = nsuper x ntiles
  size_t lds_a, lds_b;   // dynamic LDS of the scatter kernel (pass A) and of the finish kernel (pass B)
  u32 stage_cap;         // staging entries of the finish kernel
  bool big_on;           // super-buckets too large for one workgroup of pass B (skewed scalars) are finished in slices; below
  size_t big_region;     // 2^18 keys per window none can exist.  big_region: their u32 words per window group
  u32 noblk;             // order pass: blocks over all accumulated buckets,
  size_t nohist, nsums;  // their histogram cells, and the scan scratch words of one window group (sort and order scans share it)
};
static inline MsmSortGeom msm_sort_geometry(size_t n, const MsmPlan& pl, const MsmKnobs& knobs) {
  MsmSortGeom g;
  msm_part_split(n, pl.c - 1, &g.HB, &g.LB, knobs);
  g.nsuper = (u32)pl.W << g.HB;
  g.tile = msm_part_tile(g.HB, knobs);
  g.ntiles = (u32)((n + g.tile - 1) / g.tile);
  g.nthist = (size_t)g.nsuper * g.ntiles;
  g.lds_a = ((size_t)8 << g.HB) + (size_t)g.tile * 8;
  g.stage_cap = msm_part_stage_cap(g.LB);
  g.lds_b = ((size_t)(1 << g.LB) + 1024 + g.stage_cap) * 4;
  g.big_on = knobs.big_slices && n > (size_t)2 * PART_BIG;
  g.big_region = (size_t)g.nsuper + 2 * pl.nb;
  const u32 ntscan = (u32)((g.nthist + SCAN_TILE - 1) / SCAN_TILE);
  g.noblk = (u32)((pl.nbuckets() + ORDER_TILE - 1) / ORDER_TILE);
  g.nohist = (size_t)g.noblk * ORDER_BINS;
  const u32 noscan = (u32)((g.nohist + SCAN_TILE - 1) / SCAN_TILE);
  g.nsums = (size_t)(ntscan > noscan ? ntscan : noscan) + 2;
  return g;
}

// ---- geometry of the bucket reduction: level 0 (chunked running sums over L0 buckets per lane), then the bit-sliced sums ----
struct MsmReduceGeom {
  u32 red_narrow, red_full;   // a window's own bucket count: the narrow windows (the top pl.narrow ones of a plain job) fill the
                              // lower half of their cells
  u32 L0;                     // level-0 chunk length
  size_t m, mn;               // (S, A) pairs per full / per narrow window after level 0 (the last chunk may be ragged)
  int nbits;                  // bits of a pair's index: 2^nbits >= m
  u32 Q;                      // quantities per window = nbits + 1
  bool two_digit;             // second stage: row and column sums, then the bit-sliced sums of those; or one kernel over all pairs
  u32 d2, rows2;              // two-digit form: D = 2^d2 columns, rows of D pairs
  size_t nsum2;               // ... R, RA, C of one window
  u32 chunk, nchunks;         // one-kernel form: pairs per workgroup, workgroups per (window, quantity)
  size_t npart, npairs;       // chunk partials and part sums of the job
};
// lanes_per_point: 1 (G1) or 2 (G2); scalar_bits: the curve's scalar field; resident_lanes: chunks the level-0 kernel keeps
// resident on the chip (its occupancy x 128 x CUs; 0: unknown, the power of two stays)
static inline MsmReduceGeom msm_reduce_geometry(const MsmPlan& pl, u32 lanes_per_point, int scalar_bits, size_t resident_lanes,
                                                const MsmKnobs& knobs) {
  MsmReduceGeom g;
  const int Wr = pl.red_windows();
  const size_t mwin = (size_t)1 << (pl.c - 1);
  g.red_narrow = (!pl.shared && mwin >= 2) ? (u32)pl.narrow : 0u;
  g.red_full = (u32)Wr - g.red_narrow;
  u32 L0 = 32;
  {
    size_t want = (mwin * (size_t)Wr) >> 17;  // keep ~1e5 (S, A) pairs for the bit-sliced stage
    u32 p2 = 1;
    while (p2 < want) p2 <<= 1;
    // few buckets: short chains beat fewer pairs (measured: 2^15 buckets L0 = 2, 2^16..2^17 L0 = 4, profiles/r2_msm_sweeps.txt)
    const size_t nbr = mwin * (size_t)Wr;
    const u32 l0_min = nbr <= ((size_t)1 << 15) ? 2 : (nbr <= ((size_t)1 << 17) ? 4 : 8);
    if (p2 < l0_min) p2 = l0_min;
    if (p2 < L0) L0 = p2;
    // one shared bucket set (prepared base set), measured per bucket count (profiles/r2_msm_sweeps.txt, sessions L0 / AN):
    // 2^18 buckets L0 = 8, 2^19 .. 2^21 L0 = 16 (2^19: reduction 1.32 -> 0.99 ms against L0 = 8)
    if (Wr == 1 && nbr > ((size_t)1 << 18)) L0 = nbr <= ((size_t)1 << 21) ? 16 : 32;
    // (round 5) 2^19 .. 2^20 buckets on the one-lane-per-point curves (c = 17: 2^21 / 2^22 pairs): with L0 = 16 the two-wave
    // level-0 form still fits one round of the chip (2 x 61 440 lanes, 17 steps) and hands the bit-sliced stage half the pairs
    // of L0 = 8, whose 245 760 split lanes do not fit and whose one-wave form walks 16 steps: reduction 1.18 -> 0.95 ms,
    // 2^21 6.35 -> 5.99 ms, 2^22 11.20 -> 10.82 (profiles/r5_reduce_geometry_sweep.txt, session r5rs2)
    if (Wr > 1 && lanes_per_point == 1 && nbr > ((size_t)1 << 19) && nbr <= ((size_t)1 << 20)) L0 = 16;
    // (round 5) the lane-pair curves (G2) from 2^18 buckets (c >= 15: 2^17 pairs and up): their bit-sliced stage is the
    // expensive half, and twice the chain for half the pairs pays -- BLS12-377 G2 reduction 1.58 -> 1.28 ms at 2.8e5 buckets
    // (2^18: 4.65 -> 4.25 ms), 1.70 -> 1.38 at 5.2e5 (2^19 6.69 -> 6.30, 2^20 10.49 -> 10.10; BLS12-381 G2 2^20 10.13 -> 9.64),
    // 2.93 -> 2.46 at 9.8e5 (2^21 18.04 -> 17.52); at 1.6e5 buckets L0 = 8 stays the best cell (same sweeps, sessions r5g2r / r5g2r2)
    // -- and the same holds further up: 9.8e5 buckets L0 = 32 (2.46 -> 2.13 ms); 3.7e6 (2^22, c = 19) L0 = 64 on BLS12-377 G2 (13 of
    // its 14 windows are narrow: 4.32 -> 3.95 ms, session r5g2l) but 32 on BLS12-381 G2 (11 narrow: 5.85 against 6.5 ms, r5g2l3).
    // One rule covers every cell measured: the power of two at or above buckets / 32 768, from 8 to 32 (BLS12-377: 64).
    if (Wr > 1 && lanes_per_point == 2 && nbr > ((size_t)1 << 18)) {
      const u32 cap = scalar_bits == 253 ? 64u : 32u;
      u32 q = 8;
      while (q < cap && (size_t)q * 32768 < nbr) q <<= 1;
      L0 = q;
    }
    // Large plain jobs on the one-lane-per-point curves (the rules above say 32): the chunks that hold buckets are a
    // non-integer number of rounds of the chip's resident lanes (2^24, c = 20: 172 032 chunks on 131 072 lanes = 1.31 rounds of a
    // 64-addition chain, the second at a third of the occupancy).  Keep the number of rounds and shorten the chain until they are
    // full: the smallest L0 whose chunks still fit k rounds (2^24: k = 2, L0 = 22).
    if (Wr > 1 && lanes_per_point == 1 && L0 == 32 && nbr > ((size_t)1 << 21) && resident_lanes) {
      const auto chunks = [&](u32 L) { return g.red_full * ((mwin + L - 1) / L) + g.red_narrow * ((mwin / 2 + L - 1) / L); };
      const size_t rounds = (chunks(32) + resident_lanes - 1) / resident_lanes;
      while (L0 > 8 && chunks(L0 - 1) <= rounds * resident_lanes) L0--;
    }
    if (knobs.l0) L0 = (u32)knobs.l0;  // tuning knob: any chunk length 1 .. 128
    if (L0 > mwin) L0 = (u32)mwin;
  }
  g.L0 = L0;
  g.m = (mwin + L0 - 1) / L0;
  g.mn = g.red_narrow ? (mwin / 2 + L0 - 1) / L0 : g.m;
  g.nbits = 0;
  while (((size_t)1 << g.nbits) < g.m) g.nbits++;
  g.Q = (u32)g.nbits + 1;
  // second stage: the two-digit form (row and column sums, then the bit-sliced sums of those) from 2048 pairs per window
  // (a lane pair per point: 1024), the one-kernel form below that (ARK_HIP_MSM_STAGE2=0 / 1 forces one).  Measured
  // (profiles/reduce_geometry_free_l0.txt, reduction in ms, one-kernel form at its best chunk -> two digits): BLS12-381 G1
  // m = 512 (2^16) 0.27 -> 0.34, m = 2048 (2^18) 0.53 -> 0.50, m = 4096 (2^20 / 2^22) 0.75 -> 0.62 / 1.08 -> 0.85, m = 16 384
  // (2^24, L0 = 32) 3.58 -> 3.06; BN254 m = 512 0.16 -> 0.20, m = 4096 0.32 -> 0.29; BLS12-377 G2 m = 1024 (2^18) 1.25 -> 1.08,
  // m = 2048 (2^20) 1.57 -> 1.20, m = 4096 (2^22) 4.39 -> 3.35
  g.two_digit = g.m >= (lanes_per_point == 2 ? 1024u : 2048u);
  if (knobs.stage2 >= 0) g.two_digit = knobs.stage2 == 1;
  g.d2 = (u32)g.nbits / 2;                                               // low digit: D = 2^d2 columns
  g.rows2 = (u32)((g.m + ((size_t)1 << g.d2) - 1) >> g.d2);              // high digit: rows of D pairs
  g.nsum2 = 2 * (size_t)g.rows2 + ((size_t)1 << g.d2);                   // R, RA, C of one window
  // chunk of the bit-sliced stage: a workgroup's 256 lanes stride over it (chunk/256 serial additions each) before the
  // 8-step LDS tree -- both pure latency, so chunks are kept short once there are enough of them to fill the chip
  // (few workgroups, e.g. one window of a prepared set at small n: latency only, 2^16 1.39 -> 1.11 ms; many: throughput)
  u32 chunk = (size_t)Wr * g.Q * ((g.m + 4095) / 4096) < 512 ? 1024 : 4096;
  if (Wr == 1) chunk = g.m <= 16384 ? 1024 : (g.m <= 65536 ? 2048 : 4096);  // measured: m = 2^15 pairs 2048 (0.77 -> 0.70 ms)
  if (knobs.chunk) chunk = (u32)knobs.chunk;
  if (chunk > g.m || g.two_digit) chunk = (u32)g.m;    // (the two-digit form writes the part sums themselves: no chunk partials)
  g.chunk = chunk;
  g.nchunks = (u32)((g.m + chunk - 1) / chunk);
  g.npart = (size_t)Wr * g.Q * g.nchunks;
  g.npairs = (size_t)Wr * g.Q;
  return g;
}

// ---- accumulation: heavy runs, run parts, window groups -----------------------------------------------
#ifndef ARK_HEAVY_CHUNK
#define ARK_HEAVY_CHUNK 1024          // entries per wave of msm_heavy_partial_kernel: 16 serial additions per lane + the wave's
                                      // LDS tree (2048 / 64 lanes before: bool 1.85 -> 1.71 ms, u8 1.42 -> 1.21, msm_u8 1.20 -> 0.96
                                      // at 2^20 with the 128-lane combine below; 512 / 256 measured between the two -- profiles/r4_heavy_geometry_ab.txt)
#endif
static constexpr u32 HEAVY_CHUNK = ARK_HEAVY_CHUNK;

// heavy runs: a lane walks its bucket serially (~28 us per entry with two or three waves per SIMD) and
// the heaviest buckets start first; a run is "heavy" when its walk would outlast the kernel's
// throughput-bound duration (entries / 5.5e9 per s).  At 2^24 x 13 windows that is ~1400 entries, so the
// sparse top window (1024 per bucket) still rides along; skewed scalar distributions do not.
struct MsmHeavyGeom {
  size_t mean_load;      // entries per lane (a lane of a prepared set walks W runs)
  u32 forced_thresh;     // 0: computed on the device from the number of non-zero entries (msm_thresh_kernel)
  size_t max_heavy;      // heavy runs there can be: the threshold is never below 64
  size_t max_items;      // their chunks
};
static inline MsmHeavyGeom msm_heavy_geometry(size_t n, const MsmPlan& pl, const MsmKnobs& knobs) {
  MsmHeavyGeom g;
  const size_t total_entries = (size_t)n * pl.W;
  g.mean_load = total_entries / pl.nbuckets();
  g.forced_thresh = (u32)knobs.heavy;
  g.max_heavy = total_entries / 64 + 1;
  g.max_items = total_entries / HEAVY_CHUNK + g.max_heavy + 1;
  return g;
}

// Few slots with long runs (narrow scalars in one or two windows at large n): each run of a plain job is walked by this many
// lanes (msm_accumulate_parts_kernel) until the lanes make two rounds over the chip's resident ones (2 waves x 4 SIMDs x 256
// CUs x 64: measured better than one -- u16 2^24 4.24 -> 3.82 ms, u32 8.85 -> 6.88 --, four / eight rounds no better,
// profiles/r4_narrow_scalars.txt).  widths: the measured width classes, where there are any.
static inline u32 msm_run_parts(size_t n, const MsmPlan& pl, const MsmWidths* widths, const MsmKnobs& knobs) {
  u32 run_parts = 1;
  double expect = (double)n * pl.W;   // sorted entries: from the width classes where they were measured
  if (widths) {
    expect = 0.0;
    for (int k = 1; k < MSM_WIDTH_CLASSES; k++) {
      int need = (MSM_WIDTH_TOP[k] + 1 + pl.c - 1) / pl.c;
      expect += (double)widths->count[k] * (need > pl.W ? pl.W : need);
    }
  }
  const double mean_run = expect / (double)pl.nb;
  while (run_parts < 8 && pl.nb * (size_t)(2 * run_parts) <= knobs.parts_lanes && mean_run >= 32.0 * (2 * run_parts)) run_parts *= 2;
  if (pl.parts) run_parts = pl.parts;   // small plain MSMs: the plan's narrow windows count on split runs (msm_make_plan)
  if (knobs.run_parts) run_parts = (u32)knobs.run_parts;   // test / tuning knob
  return run_parts;
}

// Window groups (msm_enqueue).  The sort is memory / LDS bound and small (8-28 VGPRs per lane), the accumulate kernel is multiply bound,
// uses no LDS and leaves 70 of the 512 registers per SIMD lane free: the two overlap well.  A plain MSM is therefore cut
// into TWO groups of windows: group 0 is sorted and accumulated on `stream`; group 1's sort runs on a side stream UNDER
// group 0's accumulate kernel and its accumulate kernel follows on `stream`.  Measured (profiles/r3_window_groups_ab.txt):
// the sort kernels slow the accumulate kernel they run under by about what they hide up to 2^24 (38.6 against 38.5 ms; 2^20
// 4.27 against 4.14), and win where the sort is a larger share: 2^26 136.4 against 139.7 ms.  ARK_HIP_MSM_GROUPS=1 / =2 force it.
// One group: a prepared set (its windows share one bucket set), a piece of a streamed MSM, few windows, and n < 2^25.
static inline int msm_window_groups(size_t n, const MsmPlan& pl, bool piece, const MsmKnobs& knobs) {
  if (pl.shared || piece || pl.W < 6 || n < ((size_t)1 << 19)) return 1;
  return (knobs.groups == 2 || (knobs.groups != 1 && n >= ((size_t)1 << 25))) ? 2 : 1;
}

}  // namespace arkhip
