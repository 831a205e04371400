// The raw-limb TEST kernels of one scalar field (lazytest.cuh: the FpL ops and the Fft29 ops of the carry-free FFT pass;
// relaxtest.cuh: the relaxed saturated-limb ops of the default FFT pass): compiled once per field with -DARK_TEST_FIELD=<name> and linked into libark_hip_test.so only.
// TestFieldOpsOf is the one implementation of TestFieldOps (testops_api.hpp).
#define ARK_LAZYTEST_FFT 1
#include "lazytest.cuh"
#include "relaxtest.cuh"
#include "transcript.cuh"
#include "lookup_hash.hpp"
#include "testops_api.hpp"
#ifndef ARK_TEST_FIELD
#error "compile with -DARK_TEST_FIELD=BLS12_381_FR (or another scalar field of params.hpp)"
#endif
#define ARK_CAT2(a, b) a##b
#define ARK_CAT(a, b) ARK_CAT2(a, b)
namespace arkhip {
namespace {
template <class F>
__global__ void __launch_bounds__(64) transcript_reduce_test_kernel(const u32* words, char* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) transcript_reduce512<F>(words).store(out);
}
template <class F>
__global__ void __launch_bounds__(64) transcript_challenge_test_kernel(u32* msg, const char* elements, u32 count, char* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (u32 i = 0; i < count; i++) transcript_put_element<F>(msg, i, F::load(elements + (size_t)i * F::BYTES));
  transcript_challenge_words<F>(msg, count).store(out);
}
template <class F>
struct TestFieldOpsOf final : TestFieldOps {
  int lazy_raw_op(int op, int k, int h, const void* in, void* out, size_t n, hipStream_t s) const override {
    return lazytest::lazy_raw_op_launch<F, true, void>(op, k, h, in, out, n, s);
  }
  int relaxed_raw_op(int op, const void* in, void* out, size_t n, hipStream_t s) const override {
    return relaxtest::relaxed_raw_op_launch<F, 0>(op, in, out, n, s);
  }
  int transcript_reduce(const void* words, void* out, hipStream_t s) const override {
    hipLaunchKernelGGL((transcript_reduce_test_kernel<Fp<F>>), dim3(1), dim3(64), 0, s, (const u32*)words, (char*)out);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  }
  int transcript_challenge(void* msg, const void* elements, unsigned count, void* out, hipStream_t s) const override {
    hipLaunchKernelGGL((transcript_challenge_test_kernel<Fp<F>>), dim3(1), dim3(64), 0, s, (u32*)msg, (const char*)elements, count, (char*)out);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  }
  uint32_t lookup_slot(const uint32_t* words8, unsigned capacity_log) const override {
    static_assert(Fp<F>::N == 8, "the hash takes the element's eight words");
    return lookup_home_slot(words8, capacity_log);
  }
};
}  // namespace
const TestFieldOps& ARK_CAT(test_field_ops_, ARK_TEST_FIELD)() {
  static const TestFieldOpsOf<ARK_TEST_FIELD> ops;
  return ops;
}
}  // namespace arkhip
