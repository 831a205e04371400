// The pass plan of the small-field transform (sfp_fft.cuh) as pure host code: ark_hip_sfp_fft_plan answers from it with no device,
// the enqueue of capi_sfp.hip follows it, and the tests find every seam through it.  DESIGN.md section 27.
//
// A workgroup holds a tile of 2^tile_log elements (32 KiB of LDS) and runs radix-2 stages on it.
//   log n <= tile_log: ONE pass, one workgroup per column: every stage in LDS, the bit-reversed positions written in place.
//   beyond:            every pass takes at most tile_log - seg_log stages, because a tile has to span 2^seg_log neighbours in
//                      the dimension it does NOT transform to move whole 128-byte segments: the strided passes read and write
//                      runs of consecutive low indices, the last pass gathers the 2^seg_log sub-transforms whose outputs are
//                      neighbours after the bit reversal.  The stages are spread evenly over the fewest such passes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace arkhip {

constexpr int SFP_MAX_PASSES = 4;
// Threads per workgroup of a pass: 1024 while the launch has at most SFP_WIDE_BLOCKS workgroups (a short transform lives on the
// latency of its few workgroups), 512 beyond (two more workgroups fit a CU).  Measured: DESIGN.md section 27.
constexpr int SFP_THREADS_WIDE = 1024, SFP_THREADS = 512;
constexpr size_t SFP_WIDE_BLOCKS = 512;
inline int sfp_pass_threads(size_t blocks) { return blocks <= SFP_WIDE_BLOCKS ? SFP_THREADS_WIDE : SFP_THREADS; }
struct SfpPlan {
  int single_log;   // the largest log n one workgroup transforms alone
  int tile_log;     // elements per tile: 2^12 of 8 bytes, 2^13 of 4 bytes
  int seg_log;      // elements per 128-byte segment: 2^4 or 2^5
  int npasses;
  int stages[SFP_MAX_PASSES];
};
// word_bytes: 8 (Goldilocks) or 4; log_n <= 32.  Returns false when log_n needs more than SFP_MAX_PASSES passes.
inline bool sfp_fft_plan(int word_bytes, int log_n, SfpPlan* pl) {
  pl->tile_log = word_bytes == 8 ? 12 : 13;
  pl->seg_log = word_bytes == 8 ? 4 : 5;
  pl->single_log = pl->tile_log;
  for (int& s : pl->stages) s = 0;
  if (log_n <= pl->single_log) {
    pl->npasses = 1;
    pl->stages[0] = log_n;
    return true;
  }
  const int per = pl->tile_log - pl->seg_log;
  pl->npasses = (log_n + per - 1) / per;
  if (pl->npasses > SFP_MAX_PASSES) return false;
  for (int i = 0; i < pl->npasses; i++) pl->stages[i] = log_n / pl->npasses + (i < log_n % pl->npasses ? 1 : 0);
  return true;
}

}  // namespace arkhip
