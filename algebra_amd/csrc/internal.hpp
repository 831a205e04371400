// Internal glue between the per-curve / per-field translation units (curve_unit.hip, field_unit.hip: one object per name) and
// the C ABI (capi_*.hip): one interface of device operations per curve, one per scalar field.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace arkhip {
struct MsmWorkspace;
struct MsmTimings;
struct MsmPlan;
struct MsmKnobs;
struct MsmPiece;
struct MsmSumsHeader;
struct MsmWidths;
struct FftWorkspace;
struct FftTimings;
struct PolyPowers;
struct MlePoint;
struct FrConst;
struct SumcheckRound;
struct SumcheckProve;
struct FrLincomb;
struct CsrView;
struct FrLookup;
struct GateTerms;

// The device operations of one curve.  curve_unit.hip implements every member once, as a template over the curve; a member that
// is missing there, or whose signature differs, does not compile.  capi_core.hpp: curve_ops(id).
struct CurveOps {
  virtual int msm_enqueue(MsmWorkspace& ws, const void* d_points, size_t wstride, const MsmPlan* prepared, const void* d_scalars,
                          size_t n, int mont, hipStream_t stream, bool timing, int sbytes, int sbits,
                          const MsmPiece* piece) const = 0;
  virtual int msm_finish(MsmWorkspace& ws, int slot, uint64_t* out_xyz, MsmTimings* tm) const = 0;
  virtual int msm_sort_stages(MsmWorkspace& ws, const void* d_scalars, size_t n, int mont, hipStream_t stream, int sbytes,
                              int sbits, const MsmKnobs& knobs, uint64_t* header, void* const* out, const size_t* cap) const = 0;
  virtual int msm_piece_dump(MsmWorkspace& ws, const void* d_bases, const void* d_scalars, size_t n, int mont, hipStream_t stream,
                             const size_t* sizes, int npieces, const MsmPlan& plan, const MsmKnobs& knobs, bool as_prepared,
                             void* d_buckets, hipEvent_t* ev, uint64_t* header, uint32_t* hctr_out, size_t hctr_cap,
                             void* buckets_out, size_t buckets_cap, uint64_t* out_xyz) const = 0;
  virtual int msm_sum_ranks(const void* d_blocks, int world, size_t block_bytes, uint32_t npairs, void* d_out,
                            hipStream_t stream) const = 0;
  virtual int msm_fold_sums(const MsmSumsHeader& h, const void* h_sums, uint64_t* out_xyz) const = 0;
  virtual void msm_sample_widths(const void* h_scalars, size_t n, int mont, MsmWidths* out) const = 0;
  virtual int msm_prepare(const void* d_bases, size_t n, const MsmPlan& pl, void* d_table, void* d_tmp, hipStream_t stream) const = 0;
  virtual int batchmul_build(const void* h_base_affine, int window, void* d_scratch, void* d_table, hipStream_t stream) const = 0;
  virtual size_t batchmul_build_scratch(int window) const = 0;
  virtual int batchmul_run(const void* d_table, int window, const void* d_scalars, size_t n, int mont, void* d_tmp, void* d_out,
                           hipStream_t s) const = 0;
  virtual int sw_add_affine(const void* d_in, void* d_out, size_t n, const void* d_delta, hipStream_t s) const = 0;
  virtual int sw_normalize_batch(const void* d_in, void* d_out, size_t n, hipStream_t s) const = 0;
  virtual int sw_check(const void* d_in, size_t n, size_t base, int checks, int method, void* d_status, void* d_out,
                       hipStream_t s) const = 0;
  virtual int sw_decompress(const void* d_bytes, size_t n, size_t base, int validate, int method, void* d_points, void* d_status,
                            void* d_out, hipStream_t s) const = 0;
  virtual int sw_compress(const void* d_points, size_t n, void* d_bytes, hipStream_t s) const = 0;
  virtual int sw_vec_mul(const void* d_points, int form, const void* d_scalars, size_t kstride, int mont, size_t n, void* d_out,
                         void* d_tab, size_t slab, hipStream_t s) const = 0;
  virtual int sw_vec_fold(const void* d_lo, const void* d_hi, int form, const uint64_t* a4, const uint64_t* b4, int mont, size_t n,
                          void* d_out, void* d_tab, size_t slab, hipStream_t s) const = 0;
  virtual int sw_vec_add(const void* d_a, const void* d_b, int negate_b, size_t n, void* d_out, hipStream_t s) const = 0;
  virtual int gfft_run(void* d_jac, int k, const uint32_t* d_roots, const uint32_t* d_pre, const uint32_t* d_post, void* d_work,
                       hipStream_t s) const = 0;
  virtual size_t gfft_work_bytes(int k) const = 0;
};

// The device operations of one scalar field, implemented once in field_unit.hip.  capi_core.hpp: field_ops(id).
struct FieldOps {
  virtual int fft_run(FftWorkspace& ws, void* d_data, int k, const uint64_t* root4, const uint64_t* pre4, const uint64_t* post4,
                      const uint64_t* postc4, int zlog, hipStream_t stream, FftTimings* tm) const = 0;
  virtual int field_op(int op, const void* d_a, const void* d_b, void* d_r, size_t n, hipStream_t s) const = 0;
  virtual int fr_scale(const void* d_a, const uint64_t* k4, void* d_r, size_t n, hipStream_t s) const = 0;
  virtual int fr_div(const void* d_num, const void* d_den, void* d_r, size_t n, hipStream_t s) const = 0;
  virtual int poly_tile_value(const void* d_src, size_t n, const PolyPowers& pw, void* d_vals, hipStream_t s) const = 0;
  virtual int poly_tile_divide(const void* d_src, size_t n, const PolyPowers& pw, const void* d_carries, void* d_dst, void* d_rem,
                               hipStream_t s) const = 0;
  virtual int poly_vanishing(const void* d_p, size_t n, size_t m, void* d_q, void* d_r, hipStream_t s) const = 0;
  virtual int poly_lagrange(const uint64_t* a4, const uint64_t* c4, const uint64_t* w4, const uint64_t* wstep4, int onehot,
                            void* d_out, size_t n, size_t lanes, hipStream_t s) const = 0;
  virtual int fr_inner_product(const void* d_a, const void* d_b, size_t n, void* d_partials, void* d_out, hipStream_t s) const = 0;
  virtual int mle_fold(const void* d_src, int log_n, int w, const MlePoint& pt, void* d_dst, hipStream_t s) const = 0;
  virtual int mle_relabel(const void* d_src, size_t n, int a, int b, int k, void* d_dst, hipStream_t s) const = 0;
  virtual int fr_axpy(const void* d_a, const uint64_t* k4, const void* d_x, void* d_r, size_t n, hipStream_t s) const = 0;
  virtual int mle_eq(const void* d_hi, const FrConst& top, int unit, const MlePoint& pt, int log_n, void* d_dst,
                     hipStream_t s) const = 0;
  virtual int mle_quot(const void* d_src, int log_n, int w, const MlePoint& pt, void* d_quot, void* d_dst, hipStream_t s) const = 0;
  virtual int prod_tree(const void* d_src, int log_n, int w, void* d_dst, hipStream_t s) const = 0;
  virtual int fr_lincomb(const FrLincomb& lc, void* d_out, size_t n, hipStream_t s) const = 0;
  virtual int frac_tree(const void* d_nsrc, const void* d_dsrc, int log_n, int w, void* d_ndst, void* d_ddst,
                        hipStream_t s) const = 0;
  virtual int fr_count(const void* d_indices, size_t n, void* d_out, size_t table_len, hipStream_t s) const = 0;
  virtual int fr_lookup(const FrLookup& lk, hipStream_t s) const = 0;
  virtual int sumcheck_round(const SumcheckRound& rd, hipStream_t s) const = 0;
  virtual int sumcheck_prove(const SumcheckProve& pv, hipStream_t s) const = 0;
  virtual int scan_tile_total(int op, const void* d_src, size_t n, void* d_totals, hipStream_t s) const = 0;
  virtual int scan_tile(int op, const void* d_src, size_t n, const void* d_carries, int exclusive, void* d_dst, void* d_total,
                        hipStream_t s) const = 0;
  virtual int ratio_tile(const void* d_num, const void* d_den, size_t n, const void* d_cn, const void* d_cdi, const void* d_icd,
                         void* d_out, void* d_last, hipStream_t s) const = 0;
  virtual int gate_sum_of_products(const GateTerms& tm, void* d_out, size_t n, hipStream_t s) const = 0;
  virtual int csr_stream(const CsrView& m, const void* d_x, void* d_y, hipStream_t s) const = 0;
  virtual int csr_long(const CsrView& m, const void* d_x, void* d_partials, void* d_y, hipStream_t s) const = 0;
  virtual int merkle_leaves(const void* d_data, uint64_t count, size_t stride, size_t n, void* d_tree, int perm,
                            hipStream_t s) const = 0;
  virtual int fft_roots(FftWorkspace& ws, int k, const uint64_t* root4, hipStream_t s, const uint32_t** out) const = 0;
  virtual int fft_scalars(FftWorkspace& ws, const uint64_t* base4, const uint64_t* mul4, size_t count, void* d_out,
                          hipStream_t s) const = 0;
  virtual int fft_axis(FftWorkspace& ws, const void* d_src, void* d_dst, unsigned G, size_t cols, const uint64_t* root4,
                       hipStream_t s) const = 0;
  virtual int fft_axis_prepare(FftWorkspace& ws, unsigned G, const uint64_t* root4, hipStream_t s, const uint32_t** pw) const = 0;
  virtual int fft_axis_launch(const void* d_src, void* d_dst, unsigned G, size_t stride, size_t cols, const uint32_t* pw,
                              hipStream_t s) const = 0;
};

// the only per-name symbols: one accessor per object of curve_unit.hip / field_unit.hip
const CurveOps& curve_ops_BN254_G1();
const CurveOps& curve_ops_BLS12_381_G1();
const CurveOps& curve_ops_BLS12_377_G1();
const CurveOps& curve_ops_BLS12_377_G2();
const CurveOps& curve_ops_BLS12_381_G2();
const FieldOps& field_ops_BN254_FR();
const FieldOps& field_ops_BLS12_381_FR();
const FieldOps& field_ops_BLS12_377_FR();
}  // namespace arkhip
