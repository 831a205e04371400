// The device-arithmetic TEST kernels of one curve (testops.cuh): compiled once per curve with -DARK_TEST_CURVE=<name> and linked
// into libark_hip_test.so only -- the shipped libark_hip.so contains neither these kernels nor their entry points.
#include "devops.cuh"
#include "testops.cuh"
#include "lazytest.cuh"
#include "relaxtest.cuh"
#include "s30test.cuh"
#include "pointcodec.cuh"
#include "internal.hpp"
#ifndef ARK_TEST_CURVE
#error "compile with -DARK_TEST_CURVE=BLS12_381_G1 (or another curve of curves.cuh)"
#endif
#define ARK_CAT2(a, b) a##b
#define ARK_CAT(a, b) ARK_CAT2(a, b)
namespace arkhip {
int ARK_CAT(test_basefield_op_, ARK_TEST_CURVE)(int op, const void* a, const void* b, void* r, size_t n, hipStream_t s) {
  return field_op_launch<ARK_TEST_CURVE::F, false>(op, a, b, r, n, s);
}
int ARK_CAT(test_point_op_, ARK_TEST_CURVE)(int kind, const void* acc, const void* other, void* out, size_t n, hipStream_t s) {
  return test_point_op_launch<ARK_TEST_CURVE>(kind, acc, other, out, n, s);
}
// the square root in the coordinate field (pointcodec.cuh), reachable with inputs that no curve point gives
int ARK_CAT(test_coord_sqrt_, ARK_TEST_CURVE)(const void* in, void* out, void* ok, size_t n, hipStream_t s) {
  return coord_sqrt_launch<ARK_TEST_CURVE>(in, out, ok, n, s);
}
// raw-limb hooks (lazytest.cuh): a G1 unit serves the FpL ops of its base field, a G2 unit the Fp2L ops over it
int ARK_CAT(test_lazy_raw_op_, ARK_TEST_CURVE)(int op, int k, int h, const void* in, void* out, size_t n, hipStream_t s) {
  typedef LazyK<ARK_TEST_CURVE> K;
  if constexpr (K::LANES == 1) return lazytest::lazy_raw_op_launch<typename K::P, false, void>(op, k, h, in, out, n, s);
  else return lazytest::lazy_raw_op_launch<typename K::P, false, typename K::FL>(op, k, h, in, out, n, s);
}
int ARK_CAT(test_lazy_acc_op_, ARK_TEST_CURVE)(int kind, const void* acc, const void* other, void* out, size_t n, hipStream_t s) {
  return lazytest::lazy_acc_op_launch<ARK_TEST_CURVE>(kind, acc, other, out, n, s);
}
// raw-digit hook of the signed 30-bit form (s30test.cuh): served by the G1 unit whose accumulate kernel runs on it, -1 elsewhere
int ARK_CAT(test_s30_raw_op_, ARK_TEST_CURVE)(int op, const void* in, void* out, size_t n, hipStream_t s) {
  return s30test::s30_raw_op_launch<ARK_TEST_CURVE>(op, in, out, n, s);
}
// raw-limb hooks of the relaxed saturated-limb arithmetic (relaxtest.cuh): a G1 unit serves the Fp ops of its base field, a G2
// unit the Fp2 / Fp2Half ops over it
int ARK_CAT(test_relaxed_raw_op_, ARK_TEST_CURVE)(int op, const void* in, void* out, size_t n, hipStream_t s) {
  typedef ARK_TEST_CURVE::FA FA;
  return relaxtest::relaxed_raw_op_launch<FA::P, relaxtest::NegBetaOf<FA>::v>(op, in, out, n, s);
}
int ARK_CAT(test_relaxed_acc_op_, ARK_TEST_CURVE)(int kind, const void* acc, const void* other, void* out, size_t n, hipStream_t s) {
  return relaxtest::relaxed_acc_op_launch<ARK_TEST_CURVE>(kind, acc, other, out, n, s);
}
}  // namespace arkhip
