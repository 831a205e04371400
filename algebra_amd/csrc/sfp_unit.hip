// Instantiation of the small-field transform, pointwise, extension-field and fold kernels for one one-word field: compiled once per field with
// -DARK_UNIT_SFIELD=<name>.  SmallFieldOpsOf is the one implementation of SmallFieldOps (sfp_internal.hpp).
#include "sfp_fft.cuh"
#include "sfp_fri.cuh"
#include "sfp_internal.hpp"
#ifndef ARK_UNIT_SFIELD
#error "compile with -DARK_UNIT_SFIELD=GOLDILOCKS (or BABYBEAR, KOALABEAR)"
#endif
#define ARK_CAT2(a, b) a##b
#define ARK_CAT(a, b) ARK_CAT2(a, b)
namespace arkhip {
namespace {
template <class Cfg>
struct SmallFieldOpsOf final : SmallFieldOps {
  int fft(const SfpFftArgs& f, hipStream_t s) const override { return sfp_fft_run<Cfg>(f, s); }
  int twiddles(void* d_out, int k, const SfpPow32& root_pows, hipStream_t s) const override {
    return sfp_twiddles_run<Cfg>(d_out, k, root_pows, s);
  }
  int powers(void* d_hi, void* d_lo, size_t nhi, int lo_bits, const SfpPow32& g_pows, uint64_t scale, hipStream_t s) const override {
    return sfp_powers_run<Cfg>(d_hi, d_lo, nhi, lo_bits, g_pows, scale, s);
  }
  int vec_op(int op, const void* a, const void* b, uint64_t k, void* r, size_t n, hipStream_t s) const override {
    return sfp_vec_launch<Cfg>(op, a, b, k, r, n, s);
  }
  int xvec_op(int op, const void* a, size_t sa, const void* b, size_t sb, const SfpxConst& k, void* r, size_t sr, size_t n,
              hipStream_t s) const override {
    return sfpx_vec_launch<Cfg>(op, a, sa, b, sb, k, r, sr, n, s);
  }
  int xcombine(const void* cols, size_t count, size_t stride, size_t rows, const SfpCombineArgs& ar, void* out, size_t so,
               int accumulate, hipStream_t s) const override {
    return sfpx_combine_launch<Cfg>(cols, count, stride, rows, ar, out, so, accumulate, s);
  }
  int xfold(const SfpFoldArgs& f, int log_arity, hipStream_t s) const override { return sfpx_fold_launch<Cfg>(f, log_arity, s); }
};
}  // namespace
const SmallFieldOps& ARK_CAT(sfp_ops_, ARK_UNIT_SFIELD)() {
  static const SmallFieldOpsOf<ARK_UNIT_SFIELD> ops;
  return ops;
}
}  // namespace arkhip
