// Host runner of the raw-limb test interface (algebra_amd/csrc/lazytest_api.hpp, lazytest.cuh): reads a vector file of
// records, runs every record through the HOST forms of the carry-free arithmetic (fp28.cuh's portable _c products, the
// differences, Fft29; ec28.cuh's bucket additions on the parked accumulator layout) and writes the raw results.  The same
// vector files go to the GPU through ark_hip_test_lazy_raw_op / ark_hip_test_lazy_acc_op, where the asm forms run, so the
// vectors, their preconditions and the expected results (tests/lazy_model.py) are validated on the CPU first.
// Built and run by tests/test_lazy_model_host.py.
//
// record: int32[8] = {kind (0 raw op, 1 accumulator op), field or curve, op, k, h, n, input words, output words}, then the
// input words (accumulator ops: the n accumulators, then the n operands).  `--table` prints THE TABLE instead.
#define ARK_LAZYTEST_HOST 1
#define ARK_LAZYTEST_FFT 1
#include "lazytest.cuh"
#include <stdio.h>
#include <string>
#include <vector>
using namespace arkhip;
using namespace arkhip::lazytest;

template <class P, bool FFT>
static bool run_raw(int op, int k, int h, int n, const u32* in, u32* out) {
  const Row* row = row_of(op);
  if (!row || !params_ok(op, k, h) || op >= X2_FIRST || (op >= FFT_FIRST && !FFT)) return false;
  constexpr int L = FpL<P>::L;
  for (int t = 0; t < n; t++)
    if (!lazy_raw_apply<P, FFT>(op, k, h, in + (size_t)t * row->arity * L, out + (size_t)t * (L + 1))) return false;
  return true;
}

// the parked layout of LazyK<C, 1>::park: x | y | zz | zzz limbs, then the infinity flag
template <class P> static XYZZL<P> unpark(const u32* w) {
  constexpr int L = FpL<P>::L;
  XYZZL<P> a;
  for (int i = 0; i < L; i++) {
    a.x.l[i] = w[i];
    a.y.l[i] = w[L + i];
    a.zz.l[i] = w[2 * L + i];
    a.zzz.l[i] = w[3 * L + i];
  }
  a.inf = w[4 * L] != 0u;
  return a;
}
template <class P> static void park(const XYZZL<P>& a, u32* w) {
  constexpr int L = FpL<P>::L;
  for (int i = 0; i < L; i++) {
    w[i] = a.x.l[i];
    w[L + i] = a.y.l[i];
    w[2 * L + i] = a.zz.l[i];
    w[3 * L + i] = a.zzz.l[i];
  }
  w[4 * L] = a.inf ? 1u : 0u;
}
template <class P>
static bool run_acc(int kind, int n, const u32* in, u32* out) {
  typedef Fp<P> F;
  constexpr int L = FpL<P>::L, N = P::N, SLOT = 4 * L + 1;
  const int aw = kind == ACC_FROM_BUCKET ? 4 * N : SLOT;
  const int ow = kind == ACC_TO_BUCKET ? 4 * N : SLOT;
  const int bw = kind <= ACC_MDBL_NEG ? 2 * N : kind == ACC_ADD ? 4 * N : kind == ACC_ADD_ACC ? SLOT : 0;
  if (kind < 0 || kind >= ACC_KINDS) return false;
  const u32* others = in + (size_t)n * aw;
  for (int t = 0; t < n; t++) {
    const u32* a = in + (size_t)t * aw;
    const u32* b = others + (size_t)t * bw;
    u32* o = out + (size_t)t * ow;
    XYZZL<P> acc;
    if (kind == ACC_FROM_BUCKET) acc = lazy_from_bucket<P>(XYZZ<F>::load(a));
    else acc = unpark<P>(a);
    if (kind == ACC_MADD || kind == ACC_MSUB) {
      const Affine<F> p = Affine<F>::load(b);
      if (!p.is_zero()) {
        FpL<P> lx, ly;
        lazy_from_affine<P>(p.x, F::cond_neg(p.y, kind == ACC_MSUB), lx, ly);
        if (xyzz_madd_lazy<P>(acc, lx, ly)) {
          XYZZL<P> d;
          xyzz_mdbl_lazy<P>(d, (const char*)b, kind == ACC_MSUB);
          acc = d;
        }
      }
    } else if (kind == ACC_MDBL || kind == ACC_MDBL_NEG) {
      xyzz_mdbl_lazy<P>(acc, (const char*)b, kind == ACC_MDBL_NEG);
    } else if (kind == ACC_ADD) {
      const XYZZOperands<P> q = lazy_operands_of<P>(XYZZ<F>::load(b));
      xyzz_add_lazy<P>(acc, q.x, q.y, q.zz, q.zzz, q.inf);
    } else if (kind == ACC_ADD_ACC) {
      const XYZZL<P> q = unpark<P>(b);
      xyzz_add_lazy<P>(acc, q.x, q.y, q.zz, q.zzz, q.inf);
    } else if (kind == ACC_DBL) {
      if (!acc.inf) xyzz_dbl_lazy<P>(acc);
    } else if (kind == ACC_TO_BUCKET) {
      lazy_to_bucket<P>(acc).store(o);
      continue;
    }
    park<P>(acc, o);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--table") {
    for (int i = 0; i < NROWS; i++) {
      const Row& r = TABLE[i];
      printf("%d %s %d", r.op, r.name, r.arity);
      for (int j = 0; j < r.nk; j++) printf(" %d:%d", r.k[j], r.h[j]);
      printf("\n");
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
    const int kind = hdr[0], id = hdr[1], op = hdr[2], k = hdr[3], h = hdr[4], n = hdr[5];
    std::vector<u32> in((size_t)hdr[6]), out((size_t)hdr[7], 0u);
    if (fread(in.data(), 4, in.size(), fi) != in.size()) return 3;
    bool ok = false;
    if (kind == 0) {
      const Row* row = row_of(op);
      const int L = (id == 2 || id == 4) ? 14 : 9;
      if (!row || in.size() != (size_t)n * row->arity * L || out.size() != (size_t)n * (L + 1)) return 4;
      switch (id) {
        case 0: ok = run_raw<BN254_FQ, false>(op, k, h, n, in.data(), out.data()); break;
        case 1: ok = run_raw<BN254_FR, true>(op, k, h, n, in.data(), out.data()); break;
        case 2: ok = run_raw<BLS12_381_FQ, false>(op, k, h, n, in.data(), out.data()); break;
        case 3: ok = run_raw<BLS12_381_FR, true>(op, k, h, n, in.data(), out.data()); break;
        case 4: ok = run_raw<BLS12_377_FQ, false>(op, k, h, n, in.data(), out.data()); break;
        case 5: ok = run_raw<BLS12_377_FR, true>(op, k, h, n, in.data(), out.data()); break;
      }
    } else if (kind == 1) {
      const int L = id == 0 ? 9 : 14, N = id == 0 ? 8 : 12, SLOT = 4 * L + 1;
      const int aw = op == ACC_FROM_BUCKET ? 4 * N : SLOT, ow = op == ACC_TO_BUCKET ? 4 * N : SLOT;
      const int bw = op <= ACC_MDBL_NEG ? 2 * N : op == ACC_ADD ? 4 * N : op == ACC_ADD_ACC ? SLOT : 0;
      if (in.size() != (size_t)n * (aw + bw) || out.size() != (size_t)n * ow) return 4;
      switch (id) {
        case 0: ok = run_acc<BN254_FQ>(op, n, in.data(), out.data()); break;
        case 1: ok = run_acc<BLS12_381_FQ>(op, n, in.data(), out.data()); break;
        case 2: ok = run_acc<BLS12_377_FQ>(op, n, in.data(), out.data()); break;
      }
    }
    if (!ok) {
      fprintf(stderr, "record %d: kind %d id %d op %d <%d, %d> is not served\n", records, kind, id, op, k, h);
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
