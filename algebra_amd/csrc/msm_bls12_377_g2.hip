// Instantiation of the MSM pipeline, the fixed-base batch multiplication, the point-array and point-vector kernels for BLS12_377_G2 (one TU per curve so
// the five heavy template expansions compile in parallel).
#include "msm.cuh"
#include "msm_stage_dump.cuh"
#include "msm_piece_dump.cuh"
#include "batchmul.cuh"
#include "devops.cuh"
#include "gfft.cuh"
#include "pointcheck.cuh"
#include "pointcodec.cuh"
#include "pointvec.cuh"
#include "internal.hpp"
namespace arkhip {
int msm_enqueue_BLS12_377_G2(MsmWorkspace& ws, const void* d_points, size_t wstride, const MsmPlan* prepared, const void* d_scalars,
                   size_t n, int mont, hipStream_t stream, bool timing, int sbytes, int sbits, const MsmPiece* piece) {
  return msm_enqueue<BLS12_377_G2>(ws, d_points, wstride, prepared, d_scalars, n, mont, stream, timing, sbytes, sbits, piece);
}
int msm_sort_stages_BLS12_377_G2(MsmWorkspace& ws, const void* d_scalars, size_t n, int mont, hipStream_t stream, int sbytes, int sbits,
                   const MsmKnobs& knobs, uint64_t* header, void* const* out, const size_t* cap) {
  return msm_sort_stages<BLS12_377_G2>(ws, d_scalars, n, mont, stream, sbytes, sbits, knobs, header, out, cap);
}
int msm_piece_dump_BLS12_377_G2(MsmWorkspace& ws, const void* d_bases, const void* d_scalars, size_t n, int mont, hipStream_t stream,
                   const size_t* sizes, int npieces, const MsmPlan& plan, const MsmKnobs& knobs, bool as_prepared, void* d_buckets,
                   hipEvent_t* ev, uint64_t* header, uint32_t* hctr_out, size_t hctr_cap, void* buckets_out, size_t buckets_cap,
                   uint64_t* out_xyz) {
  return msm_piece_dump<BLS12_377_G2>(ws, d_bases, d_scalars, n, mont, stream, sizes, npieces, plan, knobs, as_prepared, d_buckets, ev, header,
                        hctr_out, hctr_cap, buckets_out, buckets_cap, out_xyz);
}
int msm_finish_BLS12_377_G2(MsmWorkspace& ws, int slot, uint64_t* out_xyz, MsmTimings* tm) {
  return msm_finish<BLS12_377_G2>(ws, slot, out_xyz, tm);
}
int msm_sum_ranks_BLS12_377_G2(const void* d_blocks, int world, size_t block_bytes, uint32_t npairs, void* d_out, hipStream_t stream) {
  return msm_sum_ranks<BLS12_377_G2>(d_blocks, world, block_bytes, npairs, d_out, stream);
}
int msm_fold_sums_BLS12_377_G2(const MsmSumsHeader& h, const void* h_sums, uint64_t* out_xyz) { return msm_fold_sums<BLS12_377_G2>(h, h_sums, out_xyz); }
void msm_sample_widths_BLS12_377_G2(const void* h_scalars, size_t n, int mont, MsmWidths* out) {
  msm_sample_widths_host<typename BLS12_377_G2::S>(h_scalars, n, mont, out);
}
int msm_prepare_BLS12_377_G2(const void* d_bases, size_t n, const MsmPlan& pl, void* d_table, void* d_tmp, hipStream_t stream) {
  return msm_prepare_table<BLS12_377_G2>(d_bases, n, pl, d_table, d_tmp, stream);
}
int batchmul_build_BLS12_377_G2(const void* h_base_affine, int window, void* d_scratch, void* d_table, hipStream_t stream) {
  return batchmul_build<BLS12_377_G2>(h_base_affine, window, d_scratch, d_table, stream);
}
size_t batchmul_build_scratch_BLS12_377_G2(int window) { return batchmul_build_scratch<BLS12_377_G2>(window); }
int batchmul_run_BLS12_377_G2(const void* d_table, int window, const void* d_scalars, size_t n, int mont, void* d_tmp, void* d_out, hipStream_t s) {
  return batchmul_run<BLS12_377_G2>(d_table, window, d_scalars, n, mont, d_tmp, d_out, s);
}
int sw_add_affine_BLS12_377_G2(const void* in, void* out, size_t n, const void* d_delta, hipStream_t s) {
  return sw_add_affine_launch<BLS12_377_G2>(in, out, n, d_delta, s);
}
int sw_normalize_batch_BLS12_377_G2(const void* in, void* out, size_t n, hipStream_t s) {
  return sw_normalize_batch_launch<BLS12_377_G2>(in, out, n, s);
}
int sw_check_BLS12_377_G2(const void* in, size_t n, size_t base, int checks, int method, void* d_status, void* d_out, hipStream_t s) {
  return sw_check_launch<BLS12_377_G2>(in, n, base, checks, method, d_status, d_out, s);
}
int sw_decompress_BLS12_377_G2(const void* d_bytes, size_t n, size_t base, int validate, int method, void* d_points, void* d_status, void* d_out,
                     hipStream_t s) {
  return sw_decompress_launch<BLS12_377_G2>(d_bytes, n, base, validate, method, d_points, d_status, d_out, s);
}
int sw_compress_BLS12_377_G2(const void* d_points, size_t n, void* d_bytes, hipStream_t s) { return sw_compress_launch<BLS12_377_G2>(d_points, n, d_bytes, s); }
int sw_vec_mul_BLS12_377_G2(const void* d_points, int form, const void* d_scalars, size_t kstride, int mont, size_t n, void* d_out, void* d_tab,
                    size_t slab, hipStream_t s) {
  return pv_chain_launch<BLS12_377_G2, 1>(d_points, nullptr, form, d_scalars, kstride, PvImm<1>{}, mont, n, d_out, d_tab, slab, s);
}
int sw_vec_fold_BLS12_377_G2(const void* d_lo, const void* d_hi, int form, const uint64_t* a4, const uint64_t* b4, int mont, size_t n, void* d_out,
                     void* d_tab, size_t slab, hipStream_t s) {
  const PvImm<2> imm = pv_imm2(a4, b4);
  return pv_chain_launch<BLS12_377_G2, 2>(d_lo, d_hi, form, nullptr, 0, imm, mont, n, d_out, d_tab, slab, s);
}
int sw_vec_add_BLS12_377_G2(const void* d_a, const void* d_b, int negate_b, size_t n, void* d_out, hipStream_t s) {
  return pv_add_launch<BLS12_377_G2>(d_a, d_b, negate_b, n, d_out, s);
}
int gfft_run_BLS12_377_G2(void* d_jac, int k, const uint32_t* d_roots, const uint32_t* d_pre, const uint32_t* d_post, void* d_work, hipStream_t s) {
  return gfft_run<BLS12_377_G2>(d_jac, k, d_roots, d_pre, d_post, d_work, s);
}
size_t gfft_work_bytes_BLS12_377_G2(int k) { return gfft_work_bytes<BLS12_377_G2>(k); }
}  // namespace arkhip
