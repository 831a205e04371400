// Instantiation of the radix-2 FFT and the pointwise field kernels and the polynomial, multilinear and sumcheck kernels for BN254_FR.
#include "fft.cuh"
#include "devops.cuh"
#include "polyops.cuh"
#include "mle.cuh"
#include "mle_open.cuh"
#include "grand_product.cuh"
#include "fraction_sum.cuh"
#include "sumcheck.cuh"
#include "internal.hpp"
namespace arkhip {
int fft_run_BN254_FR(FftWorkspace& ws, void* d_data, int k, const uint64_t* root4, const uint64_t* pre4, const uint64_t* post4,
               const uint64_t* postc4, int zlog, hipStream_t stream, FftTimings* tm) {
  return fft_run_device<BN254_FR>(ws, d_data, k, root4, pre4, post4, postc4, zlog, stream, tm);
}
int field_op_BN254_FR(int op, const void* a, const void* b, void* r, size_t n, hipStream_t s) {
  return field_op_launch<Fp<BN254_FR>, true>(op, a, b, r, n, s);
}
int fft_roots_BN254_FR(FftWorkspace& ws, int k, const uint64_t* root4, hipStream_t s, const uint32_t** out) {
  return fft_roots_run<BN254_FR>(ws, k, root4, s, out);
}
int fft_scalars_BN254_FR(FftWorkspace& ws, const uint64_t* base4, const uint64_t* mul4, size_t count, void* d_out, hipStream_t s) {
  return fft_scalars_run<BN254_FR>(ws, base4, mul4, count, d_out, s);
}
int fr_div_BN254_FR(const void* num, const void* den, void* r, size_t n, hipStream_t s) {
  return fr_div_launch<Fp<BN254_FR>>(num, den, r, n, s);
}
int fr_scale_BN254_FR(const void* a, const uint64_t* k4, void* r, size_t n, hipStream_t s) {
  return fr_scale_launch<Fp<BN254_FR>>(a, k4, r, n, s);
}
int poly_tile_value_BN254_FR(const void* src, size_t n, const PolyPowers& pw, void* vals, hipStream_t s) {
  return poly_tile_value_launch<Fp<BN254_FR>>(src, n, pw, vals, s);
}
int poly_tile_divide_BN254_FR(const void* src, size_t n, const PolyPowers& pw, const void* carries, void* dst, void* rem, hipStream_t s) {
  return poly_tile_divide_launch<Fp<BN254_FR>>(src, n, pw, carries, dst, rem, s);
}
int poly_vanishing_BN254_FR(const void* p, size_t n, size_t m, void* q, void* r, hipStream_t s) {
  return poly_vanishing_launch<Fp<BN254_FR>>(p, n, m, q, r, s);
}
int poly_lagrange_BN254_FR(const uint64_t* a4, const uint64_t* c4, const uint64_t* w4, const uint64_t* wstep4, int onehot, void* out,
                       size_t n, size_t lanes, hipStream_t s) {
  return poly_lagrange_launch<Fp<BN254_FR>>(a4, c4, w4, wstep4, onehot, out, n, lanes, s);
}
int fr_inner_product_BN254_FR(const void* a, const void* b, size_t n, void* partials, void* out, hipStream_t s) {
  return fr_inner_product_launch<Fp<BN254_FR>>(a, b, n, partials, out, s);
}
int mle_fold_BN254_FR(const void* src, int log_n, int w, const MlePoint& pt, void* dst, hipStream_t s) {
  return mle_fold_launch<Fp<BN254_FR>>(src, log_n, w, pt, dst, s);
}
int mle_relabel_BN254_FR(const void* src, size_t n, int a, int b, int k, void* dst, hipStream_t s) {
  return mle_relabel_launch<Fp<BN254_FR>>(src, n, a, b, k, dst, s);
}
int fr_axpy_BN254_FR(const void* a, const uint64_t* k4, const void* x, void* r, size_t n, hipStream_t s) {
  return fr_axpy_launch<Fp<BN254_FR>>(a, k4, x, r, n, s);
}
int mle_eq_BN254_FR(const void* hi, const FrConst& top, int unit, const MlePoint& pt, int log_n, void* dst, hipStream_t s) {
  return mle_eq_launch<Fp<BN254_FR>>(hi, top, unit, pt, log_n, dst, s);
}
int mle_quot_BN254_FR(const void* src, int log_n, int w, const MlePoint& pt, void* quot, void* dst, hipStream_t s) {
  return mle_quot_launch<Fp<BN254_FR>>(src, log_n, w, pt, quot, dst, s);
}
int prod_tree_BN254_FR(const void* src, int log_n, int w, void* dst, hipStream_t s) {
  return prod_tree_launch<Fp<BN254_FR>>(src, log_n, w, dst, s);
}
int fr_lincomb_BN254_FR(const FrLincomb& lc, void* out, size_t n, hipStream_t s) { return fr_lincomb_launch<Fp<BN254_FR>>(lc, out, n, s); }
int frac_tree_BN254_FR(const void* nsrc, const void* dsrc, int log_n, int w, void* ndst, void* ddst, hipStream_t s) {
  return frac_tree_launch<Fp<BN254_FR>>(nsrc, dsrc, log_n, w, ndst, ddst, s);
}
int fr_count_BN254_FR(const void* indices, size_t n, void* out, size_t table_len, hipStream_t s) {
  return fr_count_launch<Fp<BN254_FR>>(indices, n, out, table_len, s);
}
int sumcheck_round_BN254_FR(const SumcheckRound& rd, hipStream_t s) { return sumcheck_round_launch<Fp<BN254_FR>>(rd, s); }
int fft_axis_BN254_FR(FftWorkspace& ws, const void* d_src, void* d_dst, unsigned G, size_t cols, const uint64_t* root4, hipStream_t s) {
  return fft_axis_run<BN254_FR>(ws, d_src, d_dst, G, cols, root4, s);
}
int fft_axis_prepare_BN254_FR(FftWorkspace& ws, unsigned G, const uint64_t* root4, hipStream_t s, const uint32_t** pw) {
  std::lock_guard<std::mutex> lock(ws.mu);
  return fft_axis_prepare<BN254_FR>(ws, G, root4, s, pw);
}
int fft_axis_launch_BN254_FR(const void* d_src, void* d_dst, unsigned G, size_t stride, size_t cols, const uint32_t* pw, hipStream_t s) {
  return fft_axis_launch<BN254_FR>(d_src, d_dst, G, stride, cols, pw, s);
}
}  // namespace arkhip
