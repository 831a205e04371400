// The device-arithmetic TEST kernels of one curve (testops.cuh): compiled once per curve with -DARK_TEST_CURVE=<name> and linked
// into libark_hip_test.so only -- the shipped libark_hip.so contains neither these kernels nor their entry points.
// TestCurveOpsOf is the one implementation of TestCurveOps (testops_api.hpp).
#include "devops.cuh"
#include "testops.cuh"
#include "lazytest.cuh"
#include "relaxtest.cuh"
#include "s30test.cuh"
#include "pointcodec.cuh"
#include "testops_api.hpp"
#ifndef ARK_TEST_CURVE
#error "compile with -DARK_TEST_CURVE=BLS12_381_G1 (or another curve of curves.cuh)"
#endif
#define ARK_CAT2(a, b) a##b
#define ARK_CAT(a, b) ARK_CAT2(a, b)
namespace arkhip {
namespace {
template <class C>
struct TestCurveOpsOf final : TestCurveOps {
  int basefield_op(int op, const void* a, const void* b, void* r, size_t n, hipStream_t s) const override {
    return field_op_launch<typename C::F, false>(op, a, b, r, n, s);
  }
  int point_op(int kind, const void* acc, const void* other, void* out, size_t n, hipStream_t s) const override {
    return test_point_op_launch<C>(kind, acc, other, out, n, s);
  }
  int coord_sqrt(const void* in, void* out, void* ok, size_t n, hipStream_t s) const override {
    return coord_sqrt_launch<C>(in, out, ok, n, s);
  }
  int lazy_raw_op(int op, int k, int h, const void* in, void* out, size_t n, hipStream_t s) const override {
    typedef LazyK<C> K;
    if constexpr (K::LANES == 1) return lazytest::lazy_raw_op_launch<typename K::P, false, void>(op, k, h, in, out, n, s);
    else return lazytest::lazy_raw_op_launch<typename K::P, false, typename K::FL>(op, k, h, in, out, n, s);
  }
  int lazy_acc_op(int kind, const void* acc, const void* other, void* out, size_t n, hipStream_t s) const override {
    return lazytest::lazy_acc_op_launch<C>(kind, acc, other, out, n, s);
  }
  int s30_raw_op(int op, const void* in, void* out, size_t n, hipStream_t s) const override {
    return s30test::s30_raw_op_launch<C>(op, in, out, n, s);
  }
  int relaxed_raw_op(int op, const void* in, void* out, size_t n, hipStream_t s) const override {
    typedef typename C::FA FA;
    return relaxtest::relaxed_raw_op_launch<typename FA::P, relaxtest::NegBetaOf<FA>::v>(op, in, out, n, s);
  }
  int relaxed_acc_op(int kind, const void* acc, const void* other, void* out, size_t n, hipStream_t s) const override {
    return relaxtest::relaxed_acc_op_launch<C>(kind, acc, other, out, n, s);
  }
};
}  // namespace
const TestCurveOps& ARK_CAT(test_curve_ops_, ARK_TEST_CURVE)() {
  static const TestCurveOpsOf<ARK_TEST_CURVE> ops;
  return ops;
}
}  // namespace arkhip
