// Instantiation of the radix-2 FFT, the pointwise field kernels and the polynomial, multilinear, sumcheck, lookup, gate-expression and Merkle-leaf kernels for one
// scalar field: compiled once per field with -DARK_UNIT_FIELD=<name>.  FieldOpsOf is the one implementation of FieldOps
// (internal.hpp).
#include "fft.cuh"
#include "devops.cuh"
#include "polyops.cuh"
#include "prefixscan.cuh"
#include "spmv.cuh"
#include "mle.cuh"
#include "mle_open.cuh"
#include "grand_product.cuh"
#include "fraction_sum.cuh"
#include "lookup.cuh"
#include "sumcheck.cuh"
#include "gateexpr.cuh"
#include "merkle.cuh"
#include "internal.hpp"
#ifndef ARK_UNIT_FIELD
#error "compile with -DARK_UNIT_FIELD=BLS12_381_FR (or another scalar field of params.hpp)"
#endif
#define ARK_CAT2(a, b) a##b
#define ARK_CAT(a, b) ARK_CAT2(a, b)
namespace arkhip {
namespace {
template <class F>
struct FieldOpsOf final : FieldOps {
  int fft_run(FftWorkspace& ws, void* d_data, int k, const uint64_t* root4, const uint64_t* pre4, const uint64_t* post4,
              const uint64_t* postc4, int zlog, hipStream_t stream, FftTimings* tm) const override {
    return fft_run_device<F>(ws, d_data, k, root4, pre4, post4, postc4, zlog, stream, tm);
  }
  int field_op(int op, const void* a, const void* b, void* r, size_t n, hipStream_t s) const override {
    return field_op_launch<Fp<F>, true>(op, a, b, r, n, s);
  }
  int fft_roots(FftWorkspace& ws, int k, const uint64_t* root4, hipStream_t s, const uint32_t** out) const override {
    return fft_roots_run<F>(ws, k, root4, s, out);
  }
  int fft_scalars(FftWorkspace& ws, const uint64_t* base4, const uint64_t* mul4, size_t count, void* d_out,
                  hipStream_t s) const override {
    return fft_scalars_run<F>(ws, base4, mul4, count, d_out, s);
  }
  int fr_div(const void* num, const void* den, void* r, size_t n, hipStream_t s) const override {
    return fr_div_launch<Fp<F>>(num, den, r, n, s);
  }
  int fr_scale(const void* a, const uint64_t* k4, void* r, size_t n, hipStream_t s) const override {
    return fr_scale_launch<Fp<F>>(a, k4, r, n, s);
  }
  int poly_tile_value(const void* src, size_t n, const PolyPowers& pw, void* vals, hipStream_t s) const override {
    return poly_tile_value_launch<Fp<F>>(src, n, pw, vals, s);
  }
  int poly_tile_divide(const void* src, size_t n, const PolyPowers& pw, const void* carries, void* dst, void* rem,
                       hipStream_t s) const override {
    return poly_tile_divide_launch<Fp<F>>(src, n, pw, carries, dst, rem, s);
  }
  int poly_vanishing(const void* p, size_t n, size_t m, void* q, void* r, hipStream_t s) const override {
    return poly_vanishing_launch<Fp<F>>(p, n, m, q, r, s);
  }
  int poly_lagrange(const uint64_t* a4, const uint64_t* c4, const uint64_t* w4, const uint64_t* wstep4, int onehot, void* out,
                    size_t n, size_t lanes, hipStream_t s) const override {
    return poly_lagrange_launch<Fp<F>>(a4, c4, w4, wstep4, onehot, out, n, lanes, s);
  }
  int fr_inner_product(const void* a, const void* b, size_t n, void* partials, void* out, hipStream_t s) const override {
    return fr_inner_product_launch<Fp<F>>(a, b, n, partials, out, s);
  }
  int mle_fold(const void* src, int log_n, int w, const MlePoint& pt, void* dst, hipStream_t s) const override {
    return mle_fold_launch<Fp<F>>(src, log_n, w, pt, dst, s);
  }
  int mle_relabel(const void* src, size_t n, int a, int b, int k, void* dst, hipStream_t s) const override {
    return mle_relabel_launch<Fp<F>>(src, n, a, b, k, dst, s);
  }
  int fr_axpy(const void* a, const uint64_t* k4, const void* x, void* r, size_t n, hipStream_t s) const override {
    return fr_axpy_launch<Fp<F>>(a, k4, x, r, n, s);
  }
  int mle_eq(const void* hi, const FrConst& top, int unit, const MlePoint& pt, int log_n, void* dst, hipStream_t s) const override {
    return mle_eq_launch<Fp<F>>(hi, top, unit, pt, log_n, dst, s);
  }
  int mle_quot(const void* src, int log_n, int w, const MlePoint& pt, void* quot, void* dst, hipStream_t s) const override {
    return mle_quot_launch<Fp<F>>(src, log_n, w, pt, quot, dst, s);
  }
  int prod_tree(const void* src, int log_n, int w, void* dst, hipStream_t s) const override {
    return prod_tree_launch<Fp<F>>(src, log_n, w, dst, s);
  }
  int fr_lincomb(const FrLincomb& lc, void* out, size_t n, hipStream_t s) const override {
    return fr_lincomb_launch<Fp<F>>(lc, out, n, s);
  }
  int frac_tree(const void* nsrc, const void* dsrc, int log_n, int w, void* ndst, void* ddst, hipStream_t s) const override {
    return frac_tree_launch<Fp<F>>(nsrc, dsrc, log_n, w, ndst, ddst, s);
  }
  int fr_count(const void* indices, size_t n, void* out, size_t table_len, hipStream_t s) const override {
    return fr_count_launch<Fp<F>>(indices, n, out, table_len, s);
  }
  int fr_lookup(const FrLookup& lk, hipStream_t s) const override { return fr_lookup_launch<Fp<F>>(lk, s); }
  int sumcheck_round(const SumcheckRound& rd, hipStream_t s) const override { return sumcheck_round_launch<Fp<F>>(rd, s); }
  int sumcheck_prove(const SumcheckProve& pv, hipStream_t s) const override { return sumcheck_prove_run<Fp<F>>(pv, s); }
  int scan_tile_total(int op, const void* src, size_t n, void* totals, hipStream_t s) const override {
    return scan_tile_total_launch<Fp<F>>(op, src, n, totals, s);
  }
  int scan_tile(int op, const void* src, size_t n, const void* carries, int exclusive, void* dst, void* total,
                hipStream_t s) const override {
    return scan_tile_launch<Fp<F>>(op, src, n, carries, exclusive, dst, total, s);
  }
  int ratio_tile(const void* num, const void* den, size_t n, const void* cn, const void* cdi, const void* icd, void* out, void* last,
                 hipStream_t s) const override {
    return ratio_tile_launch<Fp<F>>(num, den, n, cn, cdi, icd, out, last, s);
  }
  int gate_sum_of_products(const GateTerms& tm, void* out, size_t n, hipStream_t s) const override {
    return gate_sum_of_products_launch<Fp<F>>(tm, out, n, s);
  }
  int csr_stream(const CsrView& m, const void* x, void* y, hipStream_t s) const override { return csr_stream_launch<Fp<F>>(m, x, y, s); }
  int csr_long(const CsrView& m, const void* x, void* partials, void* y, hipStream_t s) const override {
    return csr_long_launch<Fp<F>>(m, x, partials, y, s);
  }
  int merkle_leaves(const void* data, uint64_t count, size_t stride, size_t n, void* tree, int perm, hipStream_t s) const override {
    return merkle_leaves_fr_launch<Fp<F>>(data, count, stride, n, tree, perm, s);
  }
  int fft_axis(FftWorkspace& ws, const void* d_src, void* d_dst, unsigned G, size_t cols, const uint64_t* root4,
               hipStream_t s) const override {
    return fft_axis_run<F>(ws, d_src, d_dst, G, cols, root4, s);
  }
  int fft_axis_prepare(FftWorkspace& ws, unsigned G, const uint64_t* root4, hipStream_t s, const uint32_t** pw) const override {
    std::lock_guard<std::mutex> lock(ws.mu);
    return arkhip::fft_axis_prepare<F>(ws, G, root4, s, pw);
  }
  int fft_axis_launch(const void* d_src, void* d_dst, unsigned G, size_t stride, size_t cols, const uint32_t* pw,
                      hipStream_t s) const override {
    return arkhip::fft_axis_launch<F>(d_src, d_dst, G, stride, cols, pw, s);
  }
};
}  // namespace
const FieldOps& ARK_CAT(field_ops_, ARK_UNIT_FIELD)() {
  static const FieldOpsOf<ARK_UNIT_FIELD> ops;
  return ops;
}
}  // namespace arkhip
