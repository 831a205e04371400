// The raw-digit ops of csrc/s30test.cuh through the header's HOST forms (the portable _c twins of FpS::mul / sqr / sop2): the same
// vector files tests/test_gpu_lazy30.py sends to the device's asm column chains go through this program, and the two answers are
// compared word for word; tests/test_lazy30_model_host.py compares it with the Python model.  Stand-alone, host only.
//   lazy30_raw_host <op> <in file> <out file>      (int32 words, in_words(op) per element in, out_words(op) out)
#include "s30test.cuh"
#include <stdio.h>
#include <stdlib.h>
#include <vector>
using namespace arkhip;
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int op = atoi(argv[1]);
  if (op < 0 || op >= s30test::OPS) return 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  const size_t iw = (size_t)s30test::in_words(op), ow = (size_t)s30test::out_words(op);
  if (bytes < 0 || (size_t)bytes % (iw * 4)) return 4;
  const size_t n = (size_t)bytes / (iw * 4);
  std::vector<i32> in(n * iw + 1), out(n * ow + 1);
  if (fread(in.data(), 4, n * iw, f) != n * iw) return 5;
  fclose(f);
  for (size_t t = 0; t < n; t++) s30test::s30_raw_apply<BLS12_381_G1>(op, in.data() + t * iw, out.data() + t * ow);
  f = fopen(argv[3], "wb");
  if (!f) return 6;
  if (fwrite(out.data(), 4, n * ow, f) != n * ow) return 7;
  fclose(f);
  return 0;
}
