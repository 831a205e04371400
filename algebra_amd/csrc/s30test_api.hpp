// TEST HOOKS ONLY: the ops and word counts of the raw-digit interface to the signed 30-bit arithmetic (csrc/s30test.cuh has the
// layout and the dispatcher), beside lazytest_api.hpp's for the 28-bit forms.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace arkhip {
namespace s30test {

enum Op : int {
  MUL = 0,        // 2 slots -> 1 slot
  SQR = 1,        // 1 -> 1
  SOP2 = 2,       // 4 -> 1: a b + c d
  SUB = 3,        // 2 -> 1
  ADD_2B = 4,     // 2 -> 1: a + 2 b
  FROM_CANONICAL_SHL = 5,   // 1 (12 canonical words) -> 1
  TO_CANONICAL = 6,         // 1 -> 1 (12 canonical words)
  MADD = 7,       // parked accumulator (LazySK::park: 4 x 13 digits + the infinity flag) | base x | base y (canonical, 12 words of
                  // a slot each; the sign already on y) -> parked accumulator | 1 when the base equals the accumulated point
  FROM_CANONICAL_U = 8,     // 1 (12 canonical words) -> 1: the unsigned repack of a gathered coordinate
  MADD_ENTRY = 9,    // MADD's input with the base as gathered (y WITHOUT the sign) | 1 for a negative digit -> MADD's output: the
                     // accumulate kernel's own entry (LazySK::madd)
  MUL_SUB = 10,   // 3 -> 1: a b - s inside the product's high columns
  SQR_SUB2 = 11,  // 3 -> 1: a^2 - s - 2 d
  ADD_FULL = 12,      // two stored points A | B (x, y, zz, zzz: 12 canonical words of a slot each) -> A + B as a stored point (4 slots):
                      // the reduction kernels' full addition (xyzz_add_s), A taken up by an empty accumulator, B from memory
  ADD_FULL_ACC = 13,  // the same with B taken up by an accumulator of its own first: accumulator + accumulator
  OPS = 14
};
constexpr int SLOT = 13;
constexpr int in_words(int op) {
  return op == MADD       ? 4 * SLOT + 1 + 2 * SLOT
       : op == MADD_ENTRY ? 4 * SLOT + 1 + 2 * SLOT + 1
       : op == ADD_FULL || op == ADD_FULL_ACC ? 8 * SLOT
                          : SLOT * (op == MUL || op == SUB || op == ADD_2B ? 2 : op == SOP2 ? 4 : op == MUL_SUB || op == SQR_SUB2 ? 3 : 1);
}
constexpr int out_words(int op) {
  return op == MADD || op == MADD_ENTRY ? 4 * SLOT + 2 : op == ADD_FULL || op == ADD_FULL_ACC ? 4 * SLOT : SLOT;
}

}  // namespace s30test
}  // namespace arkhip
