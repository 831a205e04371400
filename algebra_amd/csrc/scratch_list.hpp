// Which device and pinned buffers of a Context are SCRATCH and which are CACHES -- the one list behind the test hooks
// ark_hip_test_scratch_poison / _report (capi_test.hip) and the static check of tests/test_scratch_list_host.py.
//
// SCRATCH: no call may rely on what an earlier call left there.  The buffers only ever grow and are never cleared, so the
// rule every kernel chain has to keep is "each kernel writes every cell that a later kernel of the same call reads", and a
// kernel writes no byte past what its enqueue asked for (DevBuf::asked).  for_each_scratch visits every such DevBuf,
// for_each_pinned_scratch the page-locked host areas that results and small read-backs are staged in.
//
// CACHES: content that legitimately outlives a call.  They are NOT visited; a poisoned cache would be a wrong answer by
// design.  Each with its key:
//   cache: FftTables::roots, FftTables::roots9, FftTables::small -- the entries of FftWorkspace::tables, per (field, log n,
//          root, form).  `small` is the scratch of the table's two-level build; it stays with its entry and is read only while
//          the entry is built
//   cache: FftWorkspace::tables  (the map of the above)
//   cache: FftWorkspace::powers  per (field, log n, offset, folded constant, form): coset power tables and single constants
//   cache: FftWorkspace::axis_pw  the G-point cross transform's root powers: rebuilt, stream-ordered, by every call from the root it brings
//   cache: BaseCacheEntry::dev  per (curve, host address, length), validated by a hash of the slice's full content on every call
//   cache: PreparedBases::table  a handle the caller owns (ark_hip_msm_bases_prepare .. _free): per-window multiples of its bases
//   cache: CsrSide::csr_ptr, CsrSide::csr_idx, CsrSide::csr_val, CsrSide::csr_work  a handle the caller owns (ark_hip_fr_csr_create .. _free): row_ptr, col_idx, vals and the row plan of M and, when asked for, of M^T
//   cache: SfpWorkspace::sfp_twiddles  the one-word fields' per-stage twiddle tables, per (field, log n, direction)
//   cache: SfpWorkspace::sfp_powers  their two-level coset power tables, per (field, log n, base, folded constant)
//   cache: BatchMulTable::table  a handle the caller owns (ark_hip_batch_mul_table_new .. _free): multiples of its one base
// Locals that live inside one call and are released, or moved into a cache, before it returns (or that only name a buffer
// listed elsewhere):
//   local: tmp  (capi_msm.hip: one unnormalised table row while a prepared set is built)
//   local: tb   (fft.cuh: the FftTables entry under construction; also a reference to an FftWorkspace::tmps entry)
//   local: buf  (fft.cuh: a power table under construction, moved into FftWorkspace::powers)
//   local: b    (fft.cuh: pointer to the DevBuf a power-table request fills)
// FftWorkspace::pw and FftWorkspace::stage are filled by nothing: the coset power tables moved into `powers`, and the
// host-pointer transforms stage their data in Context::stage_a.  Nothing reads them and their capacity stays 0; they are listed
// with the scratch buffers so that any future use starts out under the poison.
//
// The line between "asked for" and "slack" is DevBuf::asked, so every enqueue calls ensure() for what it is about to use even
// where the capacity is known to suffice (the guards in front of those calls only decide whether the streams must drain first).
#pragma once
#include <cstdio>
#include "capi_core.hpp"

namespace arkhip {
namespace capi {

// a rank's host mirror of comm_small (capi_comm.hip: msm_allgather) and the sharded MSM's host block (msm_sharded_sums)
constexpr size_t COMM_PINNED_BYTES = (size_t)(64 + 1) * 36 * 8;
constexpr size_t COMM_SUMS_PINNED_BYTES = sizeof(MsmSumsHeader) * 2 * MAX_DEV + (size_t)1024 * 12 * 32;

// fn(const char* name, DevBuf& buf) for every scratch DevBuf of the context
template <class Fn>
void for_each_scratch(Context& c, Fn&& fn) {
  char name[48];
  for (int l = 0; l < 2; l++) {
    MsmWorkspace& w = c.msm[l];
#define ARK_SCRATCH_LANE(M) (snprintf(name, sizeof name, "msm%d." #M, l), fn((const char*)name, w.M))
    ARK_SCRATCH_LANE(hctr); ARK_SCRATCH_LANE(hlist); ARK_SCRATCH_LANE(hitems); ARK_SCRATCH_LANE(hpart); ARK_SCRATCH_LANE(hfinal);
    ARK_SCRATCH_LANE(keys); ARK_SCRATCH_LANE(part); ARK_SCRATCH_LANE(thist); ARK_SCRATCH_LANE(toff); ARK_SCRATCH_LANE(sorted);
    ARK_SCRATCH_LANE(offsets); ARK_SCRATCH_LANE(sums); ARK_SCRATCH_LANE(buckets);
    ARK_SCRATCH_LANE(lvlS[0]); ARK_SCRATCH_LANE(lvlS[1]); ARK_SCRATCH_LANE(lvlA[0]); ARK_SCRATCH_LANE(lvlA[1]);
    ARK_SCRATCH_LANE(order); ARK_SCRATCH_LANE(ohist); ARK_SCRATCH_LANE(ooff); ARK_SCRATCH_LANE(probe); ARK_SCRATCH_LANE(big);
    ARK_SCRATCH_LANE(parts); ARK_SCRATCH_LANE(nzcnt); ARK_SCRATCH_LANE(cscal); ARK_SCRATCH_LANE(cidx);
#undef ARK_SCRATCH_LANE
  }
#define ARK_SCRATCH_CTX(M) fn(#M, c.M)
  ARK_SCRATCH_CTX(stage_a); ARK_SCRATCH_CTX(stage_b); ARK_SCRATCH_CTX(stage_c);
  ARK_SCRATCH_CTX(gfft_work); ARK_SCRATCH_CTX(gfft_scal); ARK_SCRATCH_CTX(check_work); ARK_SCRATCH_CTX(pointvec_work);
  ARK_SCRATCH_CTX(poly_work); ARK_SCRATCH_CTX(merkle_stage);
  ARK_SCRATCH_CTX(ring_s[0]); ARK_SCRATCH_CTX(ring_s[1]); ARK_SCRATCH_CTX(ring_b[0]); ARK_SCRATCH_CTX(ring_b[1]);
  ARK_SCRATCH_CTX(piece_buckets);
  ARK_SCRATCH_CTX(comm_tmp); ARK_SCRATCH_CTX(comm_small); ARK_SCRATCH_CTX(comm_sums);
  ARK_SCRATCH_CTX(fft.stage); ARK_SCRATCH_CTX(fft.pw);
  ARK_SCRATCH_CTX(sfp.sfp_ping);
#undef ARK_SCRATCH_CTX
  int i = 0;
  for (auto& kv : c.fft.tmps) {   // one ping buffer per stream, in the map's (stable) order
    snprintf(name, sizeof name, "fft.tmps[%d]", i++);
    fn((const char*)name, kv.second);
  }
}

// fn(const char* name, void* p, size_t cap, size_t asked) for every page-locked host area no call may read before writing.
// Areas of a fixed size are asked for whole (asked == cap).
template <class Fn>
void for_each_pinned_scratch(Context& c, Fn&& fn) {
  char name[48];
  for (int l = 0; l < 2; l++) {
    for (int j = 0; j < MSM_JOBS; j++) {
      MsmJob& job = c.msm[l].jobs[j];
      snprintf(name, sizeof name, "msm%d.jobs[%d].pinned", l, j);
      fn((const char*)name, job.pinned, job.pinned_cap, job.pinned_asked);
    }
    snprintf(name, sizeof name, "msm%d.probe_host", l);
    fn((const char*)name, (void*)c.msm[l].probe_host, c.msm[l].probe_host ? (size_t)64 : (size_t)0, c.msm[l].probe_host ? (size_t)64 : (size_t)0);
  }
  fn("comm_pinned", c.comm_pinned, c.comm_pinned ? COMM_PINNED_BYTES : (size_t)0, c.comm_pinned ? COMM_PINNED_BYTES : (size_t)0);
  fn("comm_sums_pinned", c.comm_sums_pinned, c.comm_sums_pinned ? COMM_SUMS_PINNED_BYTES : (size_t)0,
     c.comm_sums_pinned ? COMM_SUMS_PINNED_BYTES : (size_t)0);
  for (int k = 0; k < HostStager::SLOTS; k++) {
    snprintf(name, sizeof name, "stager.pinned[%d]", k);
    fn((const char*)name, c.stager.pinned[k], c.stager.pinned[k] ? HostStager::SLOT_BYTES : (size_t)0,
       c.stager.pinned[k] ? HostStager::SLOT_BYTES : (size_t)0);
  }
}

}  // namespace capi
}  // namespace arkhip
