// TEST HOOKS ONLY (libark_hip_test.so, tests/lazy_raw_host.hip): the raw-limb interface to the carry-free arithmetic of
// fp28.cuh / fp28x2.cuh / fft.cuh (Fft29) and to the accumulators of ec28.cuh / ec28x2.cuh in their parked layout.
//
// Operands and results cross the ABI as RAW W-bit limbs (u32[L] per element), not as canonical words, so that a test
// chooses the representation -- a semi-normalised operand, an add_lazy sum, a value of j p + c -- and sees the limbs that
// come out.  One call = one op on n lanes: lane t reads `arity` slots of L words at in[(t * arity + j) * L] and writes one
// slot of L + 1 words at out[t * (L + 1)] (word L: the op's boolean result, 0 where it has none).  The Fp2L ops own a
// lane PAIR per element (even lane c0, odd lane c1), so that the DPP partner exchange is what runs.
//
// THE TABLE below lists every (op, template parameters) the dispatcher of lazytest.cuh instantiates.  Template parameters
// are exactly those of the call sites in ec28.cuh, ec28x2.cuh, fp28x2.cuh, fft.cuh and devops.cuh (tests/
// test_lazy_model_host.py searches those files and fails when a call-site parameter is missing here); three functions no
// product kernel calls today (negsub, cond_neg_semi, is_zero_mod_p) carry the parameter tests/lazy_host_check.hip uses.
// Anything else is ARK_HIP_ERR_ARG.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace arkhip {
namespace lazytest {

enum Op : int {
  MUL = 0, SQR = 1, SOP2 = 2, SOP4 = 3, ADD_LAZY = 4, SUB = 5, SUB_SEMI = 6, SUB_SWEEP = 7, SUB_OP = 8, SUB_B_2C_NORM = 9,
  NEGSUB = 10, NEG = 11, NEG_SEMI = 12, COND_NEG_SEMI = 13, SHR_MOD = 14, TO_CANONICAL_BITS = 15, IS_ZERO_OR_P = 16,
  IS_ZERO_MOD_P = 17, UNPACK32 = 18, UNPACK32_SHL = 19, PACK32 = 20,
  // Fft29 (the three scalar fields)
  FFT_FIRST = 30, FFT_DIF = 30, FFT_REDUCE_SWEEP = 31, FFT_SWEEP = 32, FFT_CANON = 33, FFT_COND_SUB_P = 34,
  // Fp2L, one element per lane pair (BLS12-381 Fq: beta = -1; BLS12-377 Fq: beta = -5)
  X2_FIRST = 40, X2_MUL = 40, X2_SQR = 41, X2_MUL_SUB = 42, X2_REDUCE_SMALL = 43, X2_TO_CANONICAL = 44, X2_BETA_NEG = 45,
  X2_BOTH = 46, X2_SUB_SWEEP = 47, X2_SUB_B_2C_NORM = 48, X2_FROM_CANONICAL = 49
};

struct Row {
  int op;
  const char* name;
  int arity;     // input slots per lane
  int nk;        // template-parameter tuples instantiated (0: the function has none)
  int k[6], h[6];
};
// shr_mod<K>: the call sites pass K = SH of the field (8 for 14 x 28 bits, 5 for 9 x 29 bits); the dispatcher takes k = SH only
constexpr Row TABLE[] = {
    {MUL, "mul", 2, 0, {}, {}},
    {SQR, "sqr", 1, 0, {}, {}},
    {SOP2, "sop2", 4, 0, {}, {}},
    {SOP4, "sop4", 8, 0, {}, {}},
    {ADD_LAZY, "add_lazy", 2, 0, {}, {}},
    {SUB, "sub", 2, 1, {0}, {}},
    {SUB_SEMI, "sub_semi", 2, 3, {2, 3, 6}, {}},           // 6 directly; 2, 3, 6 through sub_op where SEMI2
    {SUB_SWEEP, "sub_sweep", 2, 5, {2, 3, 4, 6, 8}, {}},   // 2, 4, 8: Fp2L::sub_sweep; 2, 3, 6 through sub_op where !SEMI2
    {SUB_OP, "sub_op", 2, 3, {2, 3, 6}, {}},
    {SUB_B_2C_NORM, "sub_b_2c_norm", 3, 1, {4}, {}},
    {NEGSUB, "negsub", 2, 1, {4}, {}},                     // no product call site
    {NEG, "neg", 1, 1, {2}, {}},
    {NEG_SEMI, "neg_semi", 1, 1, {2}, {}},
    {COND_NEG_SEMI, "cond_neg_semi", 2, 1, {2}, {}},       // no product call site; slot 1 word 0: the condition
    {SHR_MOD, "shr_mod", 1, 2, {5, 8}, {}},
    {TO_CANONICAL_BITS, "to_canonical_bits", 1, 0, {}, {}},
    {IS_ZERO_OR_P, "is_zero_or_p", 1, 0, {}, {}},
    {IS_ZERO_MOD_P, "is_zero_mod_p", 1, 0, {}, {}},        // no product call site
    {UNPACK32, "unpack32", 1, 0, {}, {}},
    {UNPACK32_SHL, "unpack32_shl", 1, 0, {}, {}},
    {PACK32, "pack32", 1, 0, {}, {}},
    {FFT_DIF, "dif", 2, 3, {4, 7, 2}, {1, 2, 1}},
    {FFT_REDUCE_SWEEP, "reduce_sweep", 1, 0, {}, {}},
    {FFT_SWEEP, "sweep", 1, 0, {}, {}},
    {FFT_CANON, "canon", 1, 0, {}, {}},
    {FFT_COND_SUB_P, "cond_sub_p", 1, 0, {}, {}},
    {X2_MUL, "x2_mul", 2, 5, {2, 4, 6, 8, 10}, {}},          // KA
    {X2_SQR, "x2_sqr", 1, 4, {2, 4, 6, 10}, {}},             // KW; flag word: the `zero` out-parameter
    {X2_MUL_SUB, "x2_mul_sub", 4, 1, {4}, {2}},              // <KA, KY>
    {X2_REDUCE_SMALL, "x2_reduce_small", 1, 0, {}, {}},
    {X2_TO_CANONICAL, "x2_to_canonical", 1, 0, {}, {}},
    {X2_BETA_NEG, "x2_beta_neg", 1, 5, {2, 4, 6, 8, 10}, {}},   // every KA / KW above
    {X2_BOTH, "x2_both", 1, 0, {}, {}},                      // slot word 0: this lane's boolean; flag word: both(mine)
    {X2_SUB_SWEEP, "x2_sub_sweep", 2, 3, {2, 4, 8}, {}},
    {X2_SUB_B_2C_NORM, "x2_sub_b_2c_norm", 3, 1, {4}, {}},
    {X2_FROM_CANONICAL, "x2_from_canonical", 1, 0, {}, {}},
};
constexpr int NROWS = (int)(sizeof(TABLE) / sizeof(TABLE[0]));

inline const Row* row_of(int op) {
  for (int i = 0; i < NROWS; i++)
    if (TABLE[i].op == op) return &TABLE[i];
  return nullptr;
}
inline bool params_ok(int op, int k, int h) {
  const Row* r = row_of(op);
  if (!r) return false;
  if (r->nk == 0) return k == 0 && h == 0;
  for (int i = 0; i < r->nk; i++)
    if (r->k[i] == k && r->h[i] == h) return true;
  return false;
}

// accumulator ops: the accumulator goes in and comes out in the PARKED layout of LazyK::park / unpark (WORDS words per
// bucket), never through from_bucket / to_bucket -- except for the two kinds that ARE those functions
enum AccKind : int {
  ACC_MADD = 0,         // acc += affine base; "equal points" doubles the base (the caller's mdbl)
  ACC_MSUB = 1,         // acc -= affine base
  ACC_MDBL = 2,         // acc = 2 base
  ACC_MDBL_NEG = 3,     // acc = -2 base
  ACC_ADD = 4,          // acc += stored bucket (canonical XYZZ, repacked operand)
  ACC_ADD_ACC = 5,      // acc += parked accumulator
  ACC_DBL = 6,          // acc = 2 acc (xyzz_dbl_lazy / lazy2_dbl); an accumulator at infinity is left as it is
  ACC_FROM_BUCKET = 7,  // canonical XYZZ -> parked
  ACC_TO_BUCKET = 8,    // parked -> canonical XYZZ
  ACC_KINDS = 9
};

}  // namespace lazytest
}  // namespace arkhip
