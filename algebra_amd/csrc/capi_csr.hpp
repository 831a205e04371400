// The CSR handle of capi_csr.hip (ark_hip_fr_csr), shared with the test hook that reads it back (capi_test.hip).
#pragma once
#include "capi_core.hpp"

namespace arkhip {
namespace capi {
// one side of a handle on the device: M, or M^T in the same form.  Caches the caller owns (scratch_list.hpp).
struct CsrSide {
  size_t rows = 0, cols = 0, nnz = 0;
  size_t n_stream = 0, n_chunk = 0, n_lrow = 0;
  DevBuf csr_ptr;    // rows + 1 words
  DevBuf csr_idx;    // nnz words
  DevBuf csr_val;    // nnz elements
  DevBuf csr_work;   // the plan: [stream blocks | chunks | long rows] (csr_plan.hpp)
  void release() {
    csr_ptr.release();
    csr_idx.release();
    csr_val.release();
    csr_work.release();
  }
};
struct CsrHandle {   // ark_hip_fr_csr
  int field = -1;
  int logical = -1;  // device it lives on
  bool has_t = false;
  CsrSide side[2];   // M, M^T
};
}  // namespace capi
}  // namespace arkhip
