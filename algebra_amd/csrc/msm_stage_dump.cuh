// The integer stages of one MSM call, run and copied out: K0 (probe), the plan, K0c, K1 / K1n, the partition sort and the
// order pass of every window group, and the heavy-run list -- through the same msm_setup / MsmCall stages msm_enqueue runs.
// Reached through ark_hip_test_msm_sort_stages (capi_test.hip: the test library only); tests/msm_sort_ref.py checks the dump.
// No bases, no accumulation, no job slot: when it returns, nothing of it is in flight.
#pragma once
#include "msm.cuh"

namespace arkhip {

// header words (uint64_t each)
enum {
  MSD_C = 0, MSD_W, MSD_NARROW, MSD_N_CARRIED, MSD_COMPACTED, MSD_NGROUPS, MSD_HB, MSD_LB, MSD_TILE, MSD_NTILES, MSD_NTHIST,
  MSD_STAGE_CAP, MSD_BIG_ON, MSD_SHIFT, MSD_HEAVY_CHUNK, MSD_PART_BIG, MSD_MAX_HEAVY, MSD_MAX_ITEMS, MSD_NOBLK, MSD_NSUMS,
  MSD_LDS_A, MSD_LDS_B, MSD_SCAN_SMALL_MAX, MSD_N_ALL,
  MSD_GROUP0 = 24,   // per group g, at MSD_GROUP0 + 4 g: w0, Wg, nslots, nbk_g
  MSD_HEADER_WORDS = 32
};
// the caller's arrays (u32 words; capacities in words)
enum { MSD_KEYS = 0, MSD_CIDX, MSD_CSCAL, MSD_SORTED, MSD_OFFSETS, MSD_ORDER, MSD_HCTR, MSD_HLIST, MSD_HITEMS, MSD_ARRAYS };

// out == nullptr: the header only (K0 and the plan run, nothing else).  Otherwise out[k] receives
//   keys     [W][n_carried]                               cidx [n_carried], cscal [n_carried][8] (when compacted)
//   sorted   [W][n_carried]: group g from word w0 n_carried; words past a group's offsets[nslots] keep the 0xffffffff they are
//            filled with before the sort
//   offsets  group g's nslots + 1 words from word (w0 << (c-1)) + g      order  group g's nbk_g words from word w0 << (c-1)
//   hctr     16 words                                     hlist / hitems  group 0's entries (3 / 2 words each), then group 1's
// and a capacity that is too small is -2 before anything is written to that array.
template <class C>
int msm_sort_stages(MsmWorkspace& ws, const void* d_scalars, size_t n, int scalars_mont, hipStream_t stream, int sbytes, int sbits,
                    const MsmKnobs& knobs, uint64_t* header, void* const* out, const size_t* cap) {
  typedef XYZZ<typename C::F> Pt;
  std::lock_guard<std::mutex> lock(ws.mu);
  if (!d_scalars || !header || n == 0 || (out && !cap)) return -1;
  if (n >= (1ull << 31)) return -2;
  if (sbytes && ((sbytes != 1 && sbytes != 2 && sbytes != 4 && sbytes != 8) || sbits < 1 || sbits > 8 * sbytes)) return -1;
  const MsmPlan* prepared = nullptr;
  size_t wstride = 0;
  ws.probe_allowed = true;
  MsmSetup<C> su;
  if (int rc = msm_setup<C>(ws, d_scalars, n, scalars_mont, stream, sbytes, sbits, prepared, wstride, nullptr, knobs, su)) return rc;
  if (int rc = ws.launch_resources(su.ngroups == 2)) return rc;
  if (ws.reserve(su.n, su.pl, su.sg, su.rg, su.hg, Pt::BYTES, su.compacted, false, 1u)) return -3;
  MsmJob job;   // not a slot of the workspace: the stages only record timing events in it, and timing is off
  MsmCall<C> call = su.call(ws, job, stream, false, nullptr, 0, d_scalars, scalars_mont, nullptr, nullptr);

  const size_t nc = su.n, W = (size_t)su.pl.W;
  int shift = 0;   // (sort_group's)
  while ((su.hg.mean_load >> shift) >= 64) shift++;
  for (int k = 0; k < MSD_HEADER_WORDS; k++) header[k] = 0;
  header[MSD_C] = (uint64_t)su.pl.c;
  header[MSD_W] = W;
  header[MSD_NARROW] = (uint64_t)su.pl.narrow;
  header[MSD_N_CARRIED] = nc;
  header[MSD_COMPACTED] = su.compacted ? 1 : 0;
  header[MSD_NGROUPS] = (uint64_t)su.ngroups;
  header[MSD_HB] = (uint64_t)su.sg.HB;
  header[MSD_LB] = (uint64_t)su.sg.LB;
  header[MSD_TILE] = su.sg.tile;
  header[MSD_NTILES] = su.sg.ntiles;
  header[MSD_NTHIST] = su.sg.nthist;
  header[MSD_STAGE_CAP] = su.sg.stage_cap;
  header[MSD_BIG_ON] = su.sg.big_on ? 1 : 0;
  header[MSD_SHIFT] = (uint64_t)shift;
  header[MSD_HEAVY_CHUNK] = HEAVY_CHUNK;
  header[MSD_PART_BIG] = PART_BIG;
  header[MSD_MAX_HEAVY] = su.hg.max_heavy;
  header[MSD_MAX_ITEMS] = su.hg.max_items;
  header[MSD_NOBLK] = su.sg.noblk;
  header[MSD_NSUMS] = su.sg.nsums;
  header[MSD_LDS_A] = su.sg.lds_a;
  header[MSD_LDS_B] = su.sg.lds_b;
  header[MSD_SCAN_SMALL_MAX] = SCAN_SMALL_MAX;
  header[MSD_N_ALL] = su.n_all;
  for (int g = 0; g < su.ngroups; g++) {
    const auto& G = call.grp[g];
    uint64_t* h = header + MSD_GROUP0 + 4 * g;
    h[0] = (uint64_t)G.w0;
    h[1] = (uint64_t)G.Wg;
    h[2] = G.nslots;
    h[3] = G.nbk_g;
  }
  if (!out) return 0;

  const size_t nb = su.pl.nb, nbk = su.pl.nbuckets();
  if (cap[MSD_KEYS] < W * nc || cap[MSD_SORTED] < W * nc || cap[MSD_OFFSETS] < nb + (size_t)su.ngroups || cap[MSD_ORDER] < nbk ||
      cap[MSD_HCTR] < 16 || (su.compacted && (cap[MSD_CIDX] < nc || cap[MSD_CSCAL] < nc * 8)))
    return -2;
  for (int k = 0; k < MSD_ARRAYS; k++)
    if (!out[k] && !((k == MSD_CIDX || k == MSD_CSCAL) && !su.compacted)) return -1;

  ARK_HIP_TRY(hipMemsetAsync(ws.sorted.p, 0xff, W * nc * 4, stream));   // what the sort does not write stays recognisable
  if (int rc = call.front(d_scalars, su.n_all, su.pr, sbytes, sbits)) return rc;
  call.find_heavy(call.grp[0], stream);
  if (su.ngroups == 2) {
    ARK_HIP_TRY(hipStreamWaitEvent(stream, ws.grp_ev[1], 0));
    call.find_heavy(call.grp[1], stream);
  }
  ARK_HIP_TRY(hipGetLastError());
  ARK_HIP_TRY(hipStreamSynchronize(stream));
  if (su.ngroups == 2) ARK_HIP_TRY(hipStreamSynchronize(ws.side));

  u32 hctr[16];
  ARK_HIP_TRY(hipMemcpy(hctr, ws.hctr.p, sizeof(hctr), hipMemcpyDeviceToHost));
  size_t nlist = 0, nitems = 0;
  for (int g = 0; g < su.ngroups; g++) {
    // (the device arrays hold max_heavy runs and max_items chunk items: more would mean the kernel wrote past them)
    if (hctr[4 * g + 1] > call.grp[g].max_heavy || hctr[4 * g] > su.hg.max_items) return -2;
    nitems += hctr[4 * g];
    nlist += hctr[4 * g + 1];
  }
  if (cap[MSD_HLIST] < nlist * 3 || cap[MSD_HITEMS] < nitems * 2) return -2;
  for (int k = 0; k < 16; k++) ((u32*)out[MSD_HCTR])[k] = hctr[k];
  ARK_HIP_TRY(hipMemcpy(out[MSD_KEYS], ws.keys.p, W * nc * 4, hipMemcpyDeviceToHost));
  ARK_HIP_TRY(hipMemcpy(out[MSD_SORTED], ws.sorted.p, W * nc * 4, hipMemcpyDeviceToHost));
  if (su.compacted) {
    ARK_HIP_TRY(hipMemcpy(out[MSD_CIDX], ws.cidx.p, nc * 4, hipMemcpyDeviceToHost));
    ARK_HIP_TRY(hipMemcpy(out[MSD_CSCAL], ws.cscal.p, nc * 32, hipMemcpyDeviceToHost));
  }
  u32* hl = (u32*)out[MSD_HLIST];
  u32* hi = (u32*)out[MSD_HITEMS];
  for (int g = 0; g < su.ngroups; g++) {
    const auto& G = call.grp[g];
    ARK_HIP_TRY(hipMemcpy((u32*)out[MSD_OFFSETS] + G.slot0 + (size_t)g, G.offsets, (G.nslots + 1) * 4, hipMemcpyDeviceToHost));
    ARK_HIP_TRY(hipMemcpy((u32*)out[MSD_ORDER] + G.slot0, G.order, G.nbk_g * 4, hipMemcpyDeviceToHost));
    const size_t ne = hctr[4 * g + 1], ni = hctr[4 * g];
    if (ne) ARK_HIP_TRY(hipMemcpy(hl, G.hlist, ne * sizeof(HeavyEntry), hipMemcpyDeviceToHost));
    if (ni) ARK_HIP_TRY(hipMemcpy(hi, G.hitems, ni * sizeof(uint2), hipMemcpyDeviceToHost));
    hl += ne * 3;
    hi += ni * 2;
  }
  return 0;
}

}  // namespace arkhip
