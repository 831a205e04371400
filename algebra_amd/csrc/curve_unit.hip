// Instantiation of the MSM pipeline, the fixed-base batch multiplication, the point-array and point-vector kernels and the group
// FFT for one curve: compiled once per curve with -DARK_UNIT_CURVE=<name> (one object per curve so the five heavy template
// expansions compile in parallel).  CurveOpsOf is the one implementation of CurveOps (internal.hpp).
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
#ifndef ARK_UNIT_CURVE
#error "compile with -DARK_UNIT_CURVE=BLS12_381_G1 (or another curve of curves.cuh)"
#endif
#define ARK_CAT2(a, b) a##b
#define ARK_CAT(a, b) ARK_CAT2(a, b)
namespace arkhip {
namespace {
template <class C>
struct CurveOpsOf final : CurveOps {
  int msm_enqueue(MsmWorkspace& ws, const void* d_points, size_t wstride, const MsmPlan* prepared, const void* d_scalars, size_t n,
                  int mont, hipStream_t stream, bool timing, int sbytes, int sbits, const MsmPiece* piece) const override {
    return arkhip::msm_enqueue<C>(ws, d_points, wstride, prepared, d_scalars, n, mont, stream, timing, sbytes, sbits, piece);
  }
  int msm_sort_stages(MsmWorkspace& ws, const void* d_scalars, size_t n, int mont, hipStream_t stream, int sbytes, int sbits,
                      const MsmKnobs& knobs, uint64_t* header, void* const* out, const size_t* cap) const override {
    return arkhip::msm_sort_stages<C>(ws, d_scalars, n, mont, stream, sbytes, sbits, knobs, header, out, cap);
  }
  int msm_piece_dump(MsmWorkspace& ws, const void* d_bases, const void* d_scalars, size_t n, int mont, hipStream_t stream,
                     const size_t* sizes, int npieces, const MsmPlan& plan, const MsmKnobs& knobs, bool as_prepared, void* d_buckets,
                     hipEvent_t* ev, uint64_t* header, uint32_t* hctr_out, size_t hctr_cap, void* buckets_out, size_t buckets_cap,
                     uint64_t* out_xyz) const override {
    return arkhip::msm_piece_dump<C>(ws, d_bases, d_scalars, n, mont, stream, sizes, npieces, plan, knobs, as_prepared, d_buckets, ev,
                                     header, hctr_out, hctr_cap, buckets_out, buckets_cap, out_xyz);
  }
  int msm_finish(MsmWorkspace& ws, int slot, uint64_t* out_xyz, MsmTimings* tm) const override {
    return arkhip::msm_finish<C>(ws, slot, out_xyz, tm);
  }
  int msm_sum_ranks(const void* d_blocks, int world, size_t block_bytes, uint32_t npairs, void* d_out,
                    hipStream_t stream) const override {
    return arkhip::msm_sum_ranks<C>(d_blocks, world, block_bytes, npairs, d_out, stream);
  }
  int msm_fold_sums(const MsmSumsHeader& h, const void* h_sums, uint64_t* out_xyz) const override {
    return arkhip::msm_fold_sums<C>(h, h_sums, out_xyz);
  }
  void msm_sample_widths(const void* h_scalars, size_t n, int mont, MsmWidths* out) const override {
    msm_sample_widths_host<typename C::S>(h_scalars, n, mont, out);
  }
  int msm_prepare(const void* d_bases, size_t n, const MsmPlan& pl, void* d_table, void* d_tmp, hipStream_t stream) const override {
    return msm_prepare_table<C>(d_bases, n, pl, d_table, d_tmp, stream);
  }
  int batchmul_build(const void* h_base_affine, int window, void* d_scratch, void* d_table, hipStream_t stream) const override {
    return arkhip::batchmul_build<C>(h_base_affine, window, d_scratch, d_table, stream);
  }
  size_t batchmul_build_scratch(int window) const override { return arkhip::batchmul_build_scratch<C>(window); }
  int batchmul_run(const void* d_table, int window, const void* d_scalars, size_t n, int mont, void* d_tmp, void* d_out,
                   hipStream_t s) const override {
    return arkhip::batchmul_run<C>(d_table, window, d_scalars, n, mont, d_tmp, d_out, s);
  }
  int sw_add_affine(const void* in, void* out, size_t n, const void* d_delta, hipStream_t s) const override {
    return sw_add_affine_launch<C>(in, out, n, d_delta, s);
  }
  int sw_normalize_batch(const void* in, void* out, size_t n, hipStream_t s) const override {
    return sw_normalize_batch_launch<C>(in, out, n, s);
  }
  int sw_check(const void* in, size_t n, size_t base, int checks, int method, void* d_status, void* d_out,
               hipStream_t s) const override {
    return sw_check_launch<C>(in, n, base, checks, method, d_status, d_out, s);
  }
  int sw_decompress(const void* d_bytes, size_t n, size_t base, int validate, int method, void* d_points, void* d_status, void* d_out,
                    hipStream_t s) const override {
    return sw_decompress_launch<C>(d_bytes, n, base, validate, method, d_points, d_status, d_out, s);
  }
  int sw_compress(const void* d_points, size_t n, void* d_bytes, hipStream_t s) const override {
    return sw_compress_launch<C>(d_points, n, d_bytes, s);
  }
  int sw_vec_mul(const void* d_points, int form, const void* d_scalars, size_t kstride, int mont, size_t n, void* d_out, void* d_tab,
                 size_t slab, hipStream_t s) const override {
    return pv_chain_launch<C, 1>(d_points, nullptr, form, d_scalars, kstride, PvImm<1>{}, mont, n, d_out, d_tab, slab, s);
  }
  int sw_vec_fold(const void* d_lo, const void* d_hi, int form, const uint64_t* a4, const uint64_t* b4, int mont, size_t n,
                  void* d_out, void* d_tab, size_t slab, hipStream_t s) const override {
    const PvImm<2> imm = pv_imm2(a4, b4);
    return pv_chain_launch<C, 2>(d_lo, d_hi, form, nullptr, 0, imm, mont, n, d_out, d_tab, slab, s);
  }
  int sw_vec_add(const void* d_a, const void* d_b, int negate_b, size_t n, void* d_out, hipStream_t s) const override {
    return pv_add_launch<C>(d_a, d_b, negate_b, n, d_out, s);
  }
  int gfft_run(void* d_jac, int k, const uint32_t* d_roots, const uint32_t* d_pre, const uint32_t* d_post, void* d_work,
               hipStream_t s) const override {
    return arkhip::gfft_run<C>(d_jac, k, d_roots, d_pre, d_post, d_work, s);
  }
  size_t gfft_work_bytes(int k) const override { return arkhip::gfft_work_bytes<C>(k); }
};
}  // namespace
const CurveOps& ARK_CAT(curve_ops_, ARK_UNIT_CURVE)() {
  static const CurveOpsOf<ARK_UNIT_CURVE> ops;
  return ops;
}
}  // namespace arkhip
