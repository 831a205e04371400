// Internal glue between the per-field units of the one-word fields (sfp_unit.hip: one object per name) and their C ABI
// (capi_sfp.hip), as internal.hpp is for the curves and the four-limb scalar fields.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace arkhip {
struct SfpFftArgs;
struct SfpPow32;
struct SfpxConst;
struct SfpCombineArgs;
struct SfpFoldArgs;

// The device operations of one one-word field (sfp.cuh), implemented once in sfp_unit.hip.  capi_sfp.hip: sfp_ops(id).
struct SmallFieldOps {
  virtual int fft(const SfpFftArgs& f, hipStream_t s) const = 0;
  virtual int twiddles(void* d_out, int k, const SfpPow32& root_pows, hipStream_t s) const = 0;
  virtual int powers(void* d_hi, void* d_lo, size_t nhi, int lo_bits, const SfpPow32& g_pows, uint64_t scale,
                     hipStream_t s) const = 0;
  virtual int vec_op(int op, const void* d_a, const void* d_b, uint64_t k, void* d_r, size_t n, hipStream_t s) const = 0;
  // the extension field over it (sfp_fri.cuh): pointwise SFPX_OP_*, the combination of columns, the FRI fold
  virtual int xvec_op(int op, const void* d_a, size_t stride_a, const void* d_b, size_t stride_b, const SfpxConst& k, void* d_r,
                      size_t stride_r, size_t n, hipStream_t s) const = 0;
  virtual int xcombine(const void* d_cols, size_t count, size_t stride, size_t rows, const SfpCombineArgs& ar, void* d_out,
                       size_t stride_out, int accumulate, hipStream_t s) const = 0;
  virtual int xfold(const SfpFoldArgs& f, int log_arity, hipStream_t s) const = 0;
};
const SmallFieldOps& sfp_ops_GOLDILOCKS();
const SmallFieldOps& sfp_ops_BABYBEAR();
const SmallFieldOps& sfp_ops_KOALABEAR();
}  // namespace arkhip
