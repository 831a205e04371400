// Host-side check of the differences folded into the products that compute them (algebra_amd/csrc/fp30s.cuh: mul_sub, sqr_sub2;
// ec30s.cuh: xyzz_madd_s under ARK_S30_FUSED_DIFF) against the chain they replace.
//   * inside one program, against the functions that stay: mul_sub(a, b, s) against sub(mul(a, b), s) and sqr_sub2(a, s, d) against
//     sub(sqr(a), add_2b(s, d)), digit for digit, on the class limits (every digit at +-2^29, every sign pattern, an unsigned
//     gathered operand at its limit) and on random operands;
//   * across builds of this file, the default one and -DARK_S30_FUSED_DIFF=0 (the retained chain; 1 and 2: each fusion alone): every
//     accumulator of every chain of additions is written to the file named on the command line, and tests/test_lazy30_fused_host.py
//     compares the files byte for byte.
// Built with -fsanitize=undefined,address on the host code: the portable forms must be free of signed overflow.
#include "lazyk.cuh"
#include "curves.cuh"
#include <stdio.h>
#include <random>
#include <vector>
using namespace arkhip;
typedef BLS12_381_G1 C;
typedef BLS12_381_FQ P;
typedef Fp<P> F;
typedef FpS<P> S;
typedef LazySK<C> K;

static int bad = 0;
#define CHECK(COND, WHAT) do { if (!(COND)) { bad++; if (bad < 12) printf("FAIL %s (line %d)\n", WHAT, __LINE__); } } while (0)

static std::vector<i32> rec;   // the record the builds must agree on
static void put(const S& a) { for (int i = 0; i < S::L; i++) rec.push_back(a.l[i]); }
static void put(const XYZZS<P>& a) {
  rec.push_back(a.inf ? 1 : 0);
  if (!a.inf) { put(a.x); put(a.y); put(a.zz); put(a.zzz); }   // an accumulator at infinity keeps whatever coordinates it had
}
static void put(const XYZZ<F>& b) {
  const F* cs[4] = {&b.x, &b.y, &b.zz, &b.zzz};
  for (const F* f : cs) for (int i = 0; i < P::N; i++) rec.push_back((i32)f->l[i]);
}
static bool same_digits(const S& a, const S& b) {
  for (int i = 0; i < S::L; i++) if (a.l[i] != b.l[i]) return false;
  return true;
}
static bool normalised(const S& a) {   // digits 0..11 in [-2^29, 2^29)
  for (int i = 0; i < S::L - 1; i++) if (a.l[i] < -S::HALF || a.l[i] >= S::HALF) return false;
  return true;
}
static F rnd(std::mt19937_64& g) {
  F a;
  for (int i = 0; i < P::N; i++) a.l[i] = (u32)g();
  a.l[P::N - 1] &= (1u << ((P::BITS - 1) % 32)) - 1;   // < 2^(BITS-1) < p
  return a;
}

// a: a product operand (normalised, or an unsigned gathered coordinate), b, s, d normalised
static void check_ops(const S& a, const S& b, const S& s, const S& d, bool a_unsigned) {
  const S ms = S::mul_sub(a, b, s), want = S::sub(S::mul(a, b), s);
  CHECK(same_digits(ms, want) && normalised(ms), "mul_sub against sub(mul)");
  put(ms);
  if (a_unsigned) return;
  const S q = S::sqr_sub2(a, s, d), qw = S::sub(S::sqr(a), S::add_2b(s, d));
  CHECK(same_digits(q, qw) && normalised(q), "sqr_sub2 against sub(sqr, add_2b)");
  CHECK(same_digits(S::sqr_sub2(a, s, S::zero()), S::mul_sub(a, a, s)), "sqr_sub2 with d = 0 against mul_sub");
  put(q);
}

static void add_entry(XYZZS<P>& acc, const F& x, const F& y, bool neg) {
  Affine<F> p;
  p.x = x;
  p.y = y;
  char raw[2 * F::BYTES];
  x.store(raw);
  y.store(raw + F::BYTES);
  if (K::madd(acc, p, neg)) K::mdbl(acc, raw, neg);
  put(acc);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::mt19937_64 g(37);
  const S one = S::one();
  // ---- random operands -----------------------------------------------------------------------------------------------------
  for (int it = 0; it < 1000; it++) {
    const F a = rnd(g), b = rnd(g), c = rnd(g), d = rnd(g);
    const S ra = S::mul(S::from_canonical_shl(a.l), one), rb = S::mul(S::from_canonical_shl(b.l), one), rc = S::mul(S::from_canonical_shl(c.l), one);
    const S rd = S::mul(S::from_canonical_shl(d.l), one);
    check_ops(ra, rb, rc, rd, false);
    check_ops(S::neg(ra), S::sub(rb, rc), S::neg(rc), S::sub(rd, ra), false);   // negative digits, swept differences
    check_ops(S::from_canonical_u(a.l), rb, S::sub(rc, rd), rd, true);           // U2 - X1 as the kernel forms it
  }
  // ---- the class limits ---------------------------------------------------------------------------------------------------
  {
    std::vector<S> edge;
    auto fill = [&](auto f, i32 top) { S x; for (int i = 0; i < S::L - 1; i++) x.l[i] = f(i); x.l[S::L - 1] = top; edge.push_back(x); };
    const i32 H = S::HALF, TOP = 1 << 23;
    for (i32 top : {TOP, -TOP, 0}) {
      fill([&](int) { return H; }, top);
      fill([&](int) { return -H; }, top);
      fill([&](int i) { return (i & 1) ? H : -H; }, top);
      fill([&](int i) { return (i & 1) ? -H : H; }, top);
      fill([&](int i) { return (i & 1) ? H - 1 : -H; }, top);
    }
    fill([&](int) { return 0; }, 0);
    fill([&](int i) { return i == 0 ? 1 : 0; }, 0);
    fill([&](int i) { return i == 0 ? -1 : 0; }, 0);
    S u;   // an unsigned gathered operand with every digit at its limit
    for (int i = 0; i < S::L - 1; i++) u.l[i] = (1 << 30) - 1;
    u.l[S::L - 1] = (1 << 27) - 1;
    const size_t n = edge.size();
    for (size_t i = 0; i < n; i++)
      for (size_t j = 0; j < n; j++)
        for (size_t k = 0; k < 5; k++) {   // s over the five patterns at each top digit in turn, d over all of them
          const S& s = edge[(5 * ((i + j) % 3) + k) % n];
          check_ops(edge[i], edge[j], s, edge[(i + 3 * j + k + 1) % n], false);
          if (i == 0) check_ops(u, edge[j], s, s, true);
        }
  }
  // ---- runs of additions: the whole chain under this build's ARK_S30_FUSED_DIFF ---------------------------------------------------
  {
    F gx = F::load(GEN_BLS12_381_G1), gy = F::load((const char*)GEN_BLS12_381_G1 + F::BYTES);
    const int NPT = 24;
    F px[NPT], py[NPT];
    XYZZ<F> run = XYZZ<F>::zero();
    for (int k = 0; k < NPT; k++) {
      xyzz_madd<F>(run, gx, gy);
      F zi = F::inverse(run.zzz);
      F zzi = F::sqr(F::mul(run.zz, zi));
      px[k] = F::mul(run.x, zzi);
      py[k] = F::mul(run.y, zi);
    }
    // P P | P -P | P -P Q | P P P | P -P P P, the first entry's digit positive and negative
    for (int k = 0; k < 8; k++)
      for (int sg = 0; sg < 2; sg++) {
        const bool n = sg != 0;
        const int q = (k + 5) % NPT;
        { XYZZS<P> a = K::inf(); add_entry(a, px[k], py[k], n); add_entry(a, px[k], py[k], n); put(K::to_bucket(a)); }
        { XYZZS<P> a = K::inf(); add_entry(a, px[k], py[k], n); add_entry(a, px[k], py[k], !n); put(K::to_bucket(a)); }
        { XYZZS<P> a = K::inf(); add_entry(a, px[k], py[k], n); add_entry(a, px[k], py[k], !n); add_entry(a, px[q], py[q], n); put(K::to_bucket(a)); }
        { XYZZS<P> a = K::inf(); for (int r = 0; r < 3; r++) add_entry(a, px[k], py[k], n); put(K::to_bucket(a)); }
        { XYZZS<P> a = K::inf(); add_entry(a, px[k], py[k], n); add_entry(a, px[k], py[k], !n); add_entry(a, px[k], py[k], n); add_entry(a, px[k], py[k], n); put(K::to_bucket(a)); }
      }
    // random chains; now and then the same point again, its inverse, and a stored bucket reloaded (a streamed MSM's later piece)
    for (int trial = 0; trial < 300; trial++) {
      XYZZS<P> a = K::inf();
      const int len = 1 + g() % 12;
      for (int s = 0; s < len; s++) {
        const int k = g() % NPT;
        const bool n = g() & 1;
        add_entry(a, px[k], py[k], n);
        if (trial % 3 == 0) add_entry(a, px[k], py[k], n);
        if (trial % 7 == 0) add_entry(a, px[k], py[k], !n);
        if (trial % 4 == 1 && s == len / 2) {
          const XYZZ<F> stored = K::to_bucket(a);
          put(stored);
          a = K::from_bucket(stored);
        }
      }
      put(K::to_bucket(a));
    }
  }
  FILE* f = fopen(argv[1], "wb");
  if (!f) return 3;
  if (fwrite(rec.data(), 4, rec.size(), f) != rec.size()) return 4;
  fclose(f);
  printf("BLS12_381_FQ signed30 fused differences=%d: %s (%d bad, %zu words)\n", (int)ARK_S30_FUSED_DIFF, bad ? "FAIL" : "ok", bad, rec.size());
  return bad != 0;
}
