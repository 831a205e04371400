// TEST HOOKS ONLY (libark_hip_test.so, tests/relaxed_raw_host.hip): the raw-limb interface to the RELAXED arithmetic on saturated
// 32-bit limbs of fp.cuh -- residues kept in [0, 2p), sometimes 2p itself, product operands of up to 2 NEG_BETA p -- and to the
// XYZZ additions of ec.cuh that run on it (xyzz_madd_relaxed, xyzz_add_relaxed, xyzz_canonical).
//
// Operands and results cross the ABI as RAW limbs (u32[N] per element, N = 8 or 12), so that a test chooses the representative
// -- value + p, 2p - y, 2p itself -- and sees the limbs that come out, with no canonical() in between.  One call = one op on n
// lanes: lane t reads `arity` slots of N words at in[(t * arity + j) * N] and writes N + 1 words at out[t * (N + 1)] (word N:
// the op's boolean result, 0 where it has none).  The Fp2 and Fp2Half ops own a lane PAIR per element (even lane: the c0
// components of every operand in its slots, odd lane: the c1 components; n even).  An Fp2Half op fetches its partner's limbs
// through the DPP exchange; an Fp2 op runs whole on each lane of the pair, which then writes its own component.
//
// THE TABLE lists every op served and the fields it is served on: where the function compiles AND a kernel calls it
// (tests/test_relaxed_model_host.py searches the call sites).  Anything else is ARK_HIP_ERR_ARG.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace arkhip {
namespace relaxtest {

// field ids of include/ark_hip.h as bits: BN254_FQ 0, BN254_FR 1, BLS12_381_FQ 2, BLS12_381_FR 3, BLS12_377_FQ 4, BLS12_377_FR 5
constexpr int M_BASE = 0x15;     // the three base fields: 4p <= R, the bucket additions of ec.cuh
constexpr int M_SCALAR = 0x2a;   // the three scalar fields: the FFT butterflies (BLS12-381 Fr: 4p > R)
constexpr int M_ALL = 0x3f;
constexpr int M_EXT = 0x14;      // base fields with a quadratic extension here: BLS12-381 Fq (beta = -1), BLS12-377 Fq (beta = -5)

enum Unit : int { U_FP = 0, U_FP2 = 1, U_HALF = 2 };

enum Op : int {
  MUL_R = 0, SQR_R = 1, MUL_R1 = 2, MUL = 3, ADD_R = 4, ADD_R2 = 5, DBL_R = 6, SUB_R = 7, NEG_R = 8, SOP2_R = 9, SOP2 = 10,
  REDUCE_2P = 11, IS_ZERO_MOD_P = 12, CANONICAL = 13, REDUCE_FULL = 14,
  // Fp2, one element per lane (canonical operands)
  F2_NEG_BETA_TIMES_NEG = 20, F2_MUL = 21, F2_SQR = 22, F2_MUL_KARATSUBA = 23,
  // Fp2Half, one element per lane pair
  H_MUL_R = 30, H_SQR_R = 31, H_SOP2_R = 32, H_BETA_TIMES = 33, H_NEG_R = 34, H_IS_ZERO_MOD_P = 35, H_IS_ZERO = 36,
  H_CANONICAL = 37, H_MUL = 38, H_SQR = 39
};

struct Row {
  int op;
  const char* name;
  int arity;    // input slots per lane
  int unit;
  int fields;   // bit f: served on field f
};
constexpr Row TABLE[] = {
    {MUL_R, "mul_r", 2, U_FP, M_BASE},
    {SQR_R, "sqr_r", 1, U_FP, M_BASE},
    {MUL_R1, "mul_r1", 2, U_FP, M_SCALAR},                 // relaxed x canonical
    {MUL, "mul", 2, U_FP, M_ALL},                          // relaxed x canonical -> canonical (fft.cuh: the last twiddle)
    {ADD_R, "add_r", 2, U_FP, M_BASE},
    {ADD_R2, "add_r2", 2, U_FP, M_SCALAR},
    {DBL_R, "dbl_r", 1, U_FP, M_BASE},
    {SUB_R, "sub_r", 2, U_FP, M_ALL},
    {NEG_R, "neg_r", 1, U_FP, M_BASE},
    {SOP2_R, "sop2_r", 4, U_FP, M_BASE},
    {SOP2, "sop2", 4, U_FP, M_EXT},                        // slot 2: c2, any value up to 6p
    {REDUCE_2P, "reduce_2p", 1, U_FP, M_BASE},
    {IS_ZERO_MOD_P, "is_zero_mod_p", 1, U_FP, M_BASE},     // flag word
    {CANONICAL, "canonical", 1, U_FP, M_ALL},
    {REDUCE_FULL, "reduce_full", 1, U_FP, M_EXT},          // the host form of sop2 brings c2 below p with it
    {F2_NEG_BETA_TIMES_NEG, "neg_beta_times_neg", 1, U_FP2, M_EXT},   // on this lane's own component
    {F2_MUL, "fp2_mul", 2, U_FP2, M_EXT},
    {F2_SQR, "fp2_sqr", 1, U_FP2, M_EXT},
    {F2_MUL_KARATSUBA, "fp2_mul_karatsuba", 2, U_FP2, M_EXT},
    {H_MUL_R, "half_mul_r", 2, U_HALF, M_EXT},
    {H_SQR_R, "half_sqr_r", 1, U_HALF, M_EXT},
    {H_SOP2_R, "half_sop2_r", 4, U_HALF, M_EXT},           // sop4_r<FOLD> with the FOLD of Fp2Half::sop2_r
    {H_BETA_TIMES, "half_beta_times", 1, U_HALF, M_EXT},   // on this lane's own component
    {H_NEG_R, "half_neg_r", 1, U_HALF, M_EXT},
    {H_IS_ZERO_MOD_P, "half_is_zero_mod_p", 1, U_HALF, M_EXT},   // flag word, pair-uniform
    {H_IS_ZERO, "half_is_zero", 1, U_HALF, M_EXT},
    {H_CANONICAL, "half_canonical", 1, U_HALF, M_EXT},
    {H_MUL, "half_mul", 2, U_HALF, M_EXT},
    {H_SQR, "half_sqr", 1, U_HALF, M_EXT},
};
constexpr int NROWS = (int)(sizeof(TABLE) / sizeof(TABLE[0]));

inline const Row* row_of(int op) {
  for (int i = 0; i < NROWS; i++)
    if (TABLE[i].op == op) return &TABLE[i];
  return nullptr;
}
constexpr bool served(int op, int field) {
  for (int i = 0; i < NROWS; i++)
    if (TABLE[i].op == op) return field >= 0 && field < 6 && ((TABLE[i].fields >> field) & 1) != 0;
  return false;
}

// accumulator ops over F = C::FA (Fp for the G1 curves, Fp2Half for G2): XYZZ in and out as raw limbs in the layout of
// XYZZ<C::F> (x | y | zz | zzz, an Fp2 coordinate c0 | c1), whatever representative the test chose
enum AccKind : int {
  ACC_MADD = 0,        // xyzz_madd_relaxed(acc, x2, y2); other: x2 | y2 with y2 AS GIVEN (canonical or 2p - y)
  ACC_ADD = 1,         // xyzz_add_relaxed(acc, other); other: XYZZ, relaxed
  ACC_CANONICAL = 2,   // xyzz_canonical(acc)
  ACC_KINDS = 3
};

}  // namespace relaxtest
}  // namespace arkhip
