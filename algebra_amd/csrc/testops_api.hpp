// TEST ONLY: the device-arithmetic hooks of one curve / one scalar field, as interfaces between capi_test.hip and the test
// units (testops_curve.hip, testops_field.hip: one object per name, linked into libark_hip_test.so only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace arkhip {
// raw-limb hooks (lazytest.cuh, relaxtest.cuh): a scalar field's unit serves its FpL / Fft29 / relaxed Fp ops; a G1 unit serves
// those of its base field, a G2 unit the Fp2L / Fp2 / Fp2Half ops over it.  -1: not an op of this unit.
struct TestRawOps {
  virtual int lazy_raw_op(int op, int k, int h, const void* d_in, void* d_out, size_t n, hipStream_t s) const = 0;
  virtual int relaxed_raw_op(int op, const void* d_in, void* d_out, size_t n, hipStream_t s) const = 0;
};
struct TestFieldOps : TestRawOps {
  // the transcript of transcript.cuh in a one-lane kernel: the 512-bit reduction alone (16 words -> one element), and the whole
  // challenge (d_msg: transcript_words(count) words with the state in front, d_elements: count Montgomery elements;
  // d_out: the element; the new state replaces d_msg's first eight words)
  virtual int transcript_reduce(const void* d_words16, void* d_out, hipStream_t s) const = 0;
  virtual int transcript_challenge(void* d_msg, const void* d_elements, unsigned count, void* d_out, hipStream_t s) const = 0;
  // host only: the home slot of one element (eight 32-bit words) in a lookup table of 2^capacity_log slots (lookup_hash.hpp)
  virtual uint32_t lookup_slot(const uint32_t* words8, unsigned capacity_log) const = 0;
};
struct TestCurveOps : TestRawOps {
  virtual int basefield_op(int op, const void* d_a, const void* d_b, void* d_r, size_t n, hipStream_t s) const = 0;
  virtual int point_op(int kind, const void* d_acc, const void* d_other, void* d_out, size_t n, hipStream_t s) const = 0;
  // the square root in the coordinate field (pointcodec.cuh), reachable with inputs that no curve point gives
  virtual int coord_sqrt(const void* d_in, void* d_out, void* d_ok, size_t n, hipStream_t s) const = 0;
  virtual int lazy_acc_op(int kind, const void* d_acc, const void* d_other, void* d_out, size_t n, hipStream_t s) const = 0;
  // raw-digit hook of the signed 30-bit form (s30test.cuh): served by the G1 unit whose accumulate kernel runs on it, -1 elsewhere
  virtual int s30_raw_op(int op, const void* d_in, void* d_out, size_t n, hipStream_t s) const = 0;
  virtual int relaxed_acc_op(int kind, const void* d_acc, const void* d_other, void* d_out, size_t n, hipStream_t s) const = 0;
};

const TestCurveOps& test_curve_ops_BN254_G1();
const TestCurveOps& test_curve_ops_BLS12_381_G1();
const TestCurveOps& test_curve_ops_BLS12_377_G1();
const TestCurveOps& test_curve_ops_BLS12_377_G2();
const TestCurveOps& test_curve_ops_BLS12_381_G2();
const TestFieldOps& test_field_ops_BN254_FR();
const TestFieldOps& test_field_ops_BLS12_381_FR();
const TestFieldOps& test_field_ops_BLS12_377_FR();
}  // namespace arkhip
