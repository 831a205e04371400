// Host runner of the raw-limb test interface to the relaxed saturated-limb arithmetic (algebra_amd/csrc/relaxtest_api.hpp,
// relaxtest.cuh): reads a vector file of records, runs every record through the HOST forms of fp.cuh / ec.cuh and writes the
// raw results.  The ARK_HD limb functions (add_r, add_r2, dbl_r, sub_r, neg_r, reduce_2p, is_zero_mod_p, canonical,
// reduce_full, neg_beta_times_neg) are the statements the device runs, bit for bit; the host products return CANONICAL values,
// which the test compares as residues.  The same vector files go to the GPU through ark_hip_test_relaxed_raw_op /
// ark_hip_test_relaxed_acc_op.  Built and run by tests/test_relaxed_model_host.py.
//
// record: int32[8] = {kind (0 raw op, 1 accumulator op), field or curve, op, 0, 0, n, input words, output words}, then the input
// words (accumulator ops: the n accumulators, then the n operands).  `--table` prints THE TABLE instead.
#define ARK_RELAXTEST_HOST 1
#include "relaxtest.cuh"
#include <stdio.h>
#include <string>
#include <vector>
using namespace arkhip;
using namespace arkhip::relaxtest;

template <class P, int NEG_BETA>
static bool run_raw(int op, int n, const u32* in, u32* out) {
  const Row* row = row_of(op);
  constexpr int N = P::N;
  if (!row || !served(op, FieldId<P>::v) || row->unit == U_HALF) return false;   // Fp2Half is device code
  for (int t = 0; t < n; t++) {
    u32* o = out + (size_t)t * (N + 1);
    if (row->unit == U_FP) {
      if (!relaxed_raw_apply<P>(op, in + (size_t)t * row->arity * N, o)) return false;
    } else {
      if constexpr (NEG_BETA != 0) {
        const size_t e = (size_t)t & ~(size_t)1;
        if ((n & 1) || !relaxed_raw_apply_fp2<P, NEG_BETA>(op, in + e * row->arity * N, in + (e + 1) * row->arity * N, t & 1, o))
          return false;
      } else {
        return false;
      }
    }
  }
  return true;
}

template <class P>
static bool run_acc(int kind, int n, const u32* in, u32* out) {
  typedef Fp<P> F;
  constexpr int N = P::N;
  if (kind < 0 || kind >= ACC_KINDS) return false;
  const int bw = kind == ACC_MADD ? 2 * N : kind == ACC_ADD ? 4 * N : 0;
  const u32* others = in + (size_t)n * 4 * N;
  for (int t = 0; t < n; t++)
    relaxed_acc_apply<F>(kind, (const char*)(in + (size_t)t * 4 * N), (const char*)(others + (size_t)t * bw),
                         (char*)(out + (size_t)t * 4 * N));
  return true;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--table") {
    for (int i = 0; i < NROWS; i++) {
      const Row& r = TABLE[i];
      printf("%d %s %d %d %d\n", r.op, r.name, r.arity, r.unit, r.fields);
    }
    return 0;
  }
  if (argc != 3) {
    fprintf(stderr, "usage: %s <vectors> <results> | --table\n", argv[0]);
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  int hdr[8];
  int records = 0;
  while (fread(hdr, sizeof(int), 8, fi) == 8) {
    const int kind = hdr[0], id = hdr[1], op = hdr[2], n = hdr[5];
    std::vector<u32> in((size_t)hdr[6]), out((size_t)hdr[7], 0u);
    if (fread(in.data(), 4, in.size(), fi) != in.size()) return 3;
    bool ok = false;
    if (kind == 0) {
      const Row* row = row_of(op);
      const int N = (id == 2 || id == 4) ? 12 : 8;
      if (!row || in.size() != (size_t)n * row->arity * N || out.size() != (size_t)n * (N + 1)) return 4;
      switch (id) {
        case 0: ok = run_raw<BN254_FQ, 0>(op, n, in.data(), out.data()); break;
        case 1: ok = run_raw<BN254_FR, 0>(op, n, in.data(), out.data()); break;
        case 2: ok = run_raw<BLS12_381_FQ, 1>(op, n, in.data(), out.data()); break;
        case 3: ok = run_raw<BLS12_381_FR, 0>(op, n, in.data(), out.data()); break;
        case 4: ok = run_raw<BLS12_377_FQ, 5>(op, n, in.data(), out.data()); break;
        case 5: ok = run_raw<BLS12_377_FR, 0>(op, n, in.data(), out.data()); break;
      }
    } else if (kind == 1) {
      const int N = id == 0 ? 8 : 12;
      const int bw = op == ACC_MADD ? 2 * N : op == ACC_ADD ? 4 * N : 0;
      if (in.size() != (size_t)n * (4 * N + bw) || out.size() != (size_t)n * 4 * N) return 4;
      switch (id) {
        case 0: ok = run_acc<BN254_FQ>(op, n, in.data(), out.data()); break;
        case 1: ok = run_acc<BLS12_381_FQ>(op, n, in.data(), out.data()); break;
        case 2: ok = run_acc<BLS12_377_FQ>(op, n, in.data(), out.data()); break;
      }
    }
    if (!ok) {
      fprintf(stderr, "record %d: kind %d id %d op %d is not served\n", records, kind, id, op);
      return 5;
    }
    if (fwrite(out.data(), 4, out.size(), fo) != out.size()) return 3;
    records++;
  }
  fclose(fi);
  fclose(fo);
  printf("%d records\n", records);
  return 0;
}
