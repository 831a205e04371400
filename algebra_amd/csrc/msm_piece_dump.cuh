// One MSM run as explicit pieces that share one plan and one bucket array (MsmPiece), the way capi_stream.hpp's msm_stream
// runs them -- through the unchanged msm_enqueue / msm_finish -- with the whole bucket array and the counter words copied out
// behind every piece.  Reached through ark_hip_test_msm_pieces (capi_test.hip: the test library only);
// tests/msm_bucket_ref.py checks the dump.  One lane, one stream: pieces here do not alternate lanes or ring slots.
// When it returns, nothing of it is in flight and no job slot is taken.
#pragma once
#include "msm.cuh"

namespace arkhip {

static constexpr int MPD_MAX_PIECES = 16;
// header words (uint64_t each)
enum {
  MPD_C = 0, MPD_W, MPD_NARROW, MPD_NBUCKETS, MPD_PT_BYTES, MPD_NPIECES, MPD_PIECES_RUN, MPD_BAD_PIECE, MPD_L0, MPD_M, MPD_MN,
  MPD_NBITS, MPD_Q, MPD_TWO_DIGIT, MPD_NPAIRS, MPD_LAZY,
  MPD_PIECE0 = 16,   // per piece k, at MPD_PIECE0 + 4 k: HB, LB, n, window groups
  MPD_HEADER_WORDS = MPD_PIECE0 + 4 * MPD_MAX_PIECES
};

// d_bases / d_scalars: the n pairs in device memory; sizes[npieces]: the pieces' pair counts (they sum to n, none is zero);
// plan: the plan of the whole job; d_buckets: plan.nbuckets() XYZZ points; ev: the two events msm_stream alternates.
// hctr_out == nullptr: the header only (nothing is enqueued).  Otherwise piece k's 16 counter words go to hctr_out + 16 k and
// the bucket array behind piece k to buckets_out + k * nbuckets * Pt::BYTES; a capacity (hctr_cap in words, buckets_cap in
// bytes) that is too small is -2 before anything is written.  out_xyz: the result, behind the last piece.
// as_prepared: hand the plan to msm_enqueue as a prepared set's as well -- which it must refuse (-1).
// A scalar out of range in piece k: -4 with header[MPD_BAD_PIECE] = k; no later piece is enqueued.
template <class C>
int msm_piece_dump(MsmWorkspace& ws, const void* d_bases, const void* d_scalars, size_t n, int scalars_mont, hipStream_t stream,
                   const size_t* sizes, int npieces, const MsmPlan& plan, const MsmKnobs& knobs, bool as_prepared, void* d_buckets,
                   hipEvent_t* ev, uint64_t* header, uint32_t* hctr_out, size_t hctr_cap, void* buckets_out, size_t buckets_cap,
                   uint64_t* out_xyz) {
  typedef XYZZ<typename C::F> Pt;
  typedef Affine<typename C::F> Af;
  if (!d_bases || !d_scalars || !sizes || !header || !d_buckets || !ev || npieces < 1 || npieces > MPD_MAX_PIECES) return -1;
  size_t sum = 0;
  for (int k = 0; k < npieces; k++) {
    if (sizes[k] == 0 || sizes[k] >= (1ull << 31)) return -1;
    sum += sizes[k];
  }
  if (sum != n) return -1;
  const size_t nbk = plan.nbuckets();
  const MsmReduceGeom rg =
      msm_reduce_geometry(plan, C::FA::LANES, C::S::BITS, C::FA::LANES == 1 ? msm_resident_lanes<C>() : 0, knobs);
  for (int k = 0; k < MPD_HEADER_WORDS; k++) header[k] = 0;
  header[MPD_C] = (uint64_t)plan.c;
  header[MPD_W] = (uint64_t)plan.W;
  header[MPD_NARROW] = (uint64_t)plan.narrow;
  header[MPD_NBUCKETS] = nbk;
  header[MPD_PT_BYTES] = Pt::BYTES;
  header[MPD_NPIECES] = (uint64_t)npieces;
  header[MPD_BAD_PIECE] = ~0ull;
  header[MPD_L0] = rg.L0;
  header[MPD_M] = rg.m;
  header[MPD_MN] = rg.mn;
  header[MPD_NBITS] = (uint64_t)rg.nbits;
  header[MPD_Q] = rg.Q;
  header[MPD_TWO_DIGIT] = rg.two_digit ? 1 : 0;
  header[MPD_NPAIRS] = rg.npairs;
  header[MPD_LAZY] = knobs.lazy ? 1 : 0;
  for (int k = 0; k < npieces; k++) {
    const MsmSortGeom sg = msm_sort_geometry(sizes[k], plan, knobs);
    uint64_t* h = header + MPD_PIECE0 + 4 * k;
    h[0] = (uint64_t)sg.HB;
    h[1] = (uint64_t)sg.LB;
    h[2] = sizes[k];
    h[3] = (uint64_t)msm_window_groups(sizes[k], plan, true, knobs);
  }
  if (!hctr_out) return 0;
  if (!buckets_out || !out_xyz) return -1;
  if (hctr_cap < (size_t)16 * (size_t)npieces || buckets_cap < (size_t)npieces * nbk * Pt::BYTES) return -2;

  ws.probe_allowed = true;
  size_t off = 0;
  for (int k = 0; k < npieces; off += sizes[k], k++) {
    const MsmPiece piece{&plan, d_buckets, k == 0, k + 1 == npieces, k == 0 ? nullptr : ev[(k - 1) & 1], ev[k & 1]};
    const int slot = msm_enqueue<C>(ws, (const char*)d_bases + off * Af::BYTES, 0, as_prepared ? &plan : nullptr,
                                    (const char*)d_scalars + off * 32, sizes[k], scalars_mont, stream, false, 0, 0, &piece, &knobs);
    if (slot < 0) {
      (void)hipStreamSynchronize(stream);   // an error behind the first launch: whatever was enqueued has run out
      return slot;
    }
    const int rc = msm_finish<C>(ws, slot, out_xyz, nullptr);   // waits for the piece and frees the slot, whatever it returns
    header[MPD_PIECES_RUN] = (uint64_t)(k + 1);
    if (rc) {
      if (rc == -4) header[MPD_BAD_PIECE] = (uint64_t)k;
      (void)hipStreamSynchronize(stream);
      return rc;
    }
    ARK_HIP_TRY(hipStreamSynchronize(stream));
    ARK_HIP_TRY(hipMemcpy(hctr_out + 16 * (size_t)k, ws.hctr.p, 64, hipMemcpyDeviceToHost));
    ARK_HIP_TRY(hipMemcpy((char*)buckets_out + (size_t)k * nbk * Pt::BYTES, d_buckets, nbk * Pt::BYTES, hipMemcpyDeviceToHost));
  }
  return 0;
}

}  // namespace arkhip
