// Host-side check of the unsigned gathered coordinate of the accumulate kernel's mixed addition (algebra_amd/csrc/fp30s.cuh:
// from_canonical_u; ec30s.cuh: s30_from_affine under ARK_S30_UNSIGNED_GATHER) against the path it replaces.
//   * inside one program, against the functions that stay: from_canonical_u against from_canonical_shl (the same value, the same
//     product digits, either operand order), LazySK::madd against xyzz_madd_s on recoded operands;
//   * across two builds of this file, the default one and -DARK_S30_UNSIGNED_GATHER=0 (the retained old path): every product and
//     every accumulator of every chain is written to the file named on the command line, and tests/test_lazy30_diet_host.py
//     compares the two files byte for byte.
// Inputs: random chains of bases with both digit signs, buckets that hold exactly P P, P -P and P -P Q, operands with negative
// digits, the class limits.  Built with -fsanitize=undefined,address on the host code.
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

static std::vector<i32> rec;   // the record the two builds must agree on
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
static bool same_acc(const XYZZS<P>& a, const XYZZS<P>& b) {
  if (a.inf || b.inf) return a.inf == b.inf;
  return same_digits(a.x, b.x) && same_digits(a.y, b.y) && same_digits(a.zz, b.zz) && same_digits(a.zzz, b.zzz);
}
static F rnd(std::mt19937_64& g) {
  F a;
  for (int i = 0; i < P::N; i++) a.l[i] = (u32)g();
  a.l[P::N - 1] &= (1u << ((P::BITS - 1) % 32)) - 1;   // < 2^(BITS-1) < p
  return a;
}

// products on (a, b, c, d): a, b, c product operands (normalised), d any gathered coordinate
static void check_ops(const S& a, const S& b, const S& c, const F& d) {
  const S m = S::mul(a, b), q = S::sqr(a), s = S::sop2(a, b, c, S::neg(a));
  put(m); put(q); put(s);
  CHECK(same_digits(q, S::mul(a, a)), "sqr against mul");
  // the gathered coordinate: unsigned digits in their class, the value and every product of the recoded form
  const S du = S::from_canonical_u(d.l), ds = S::from_canonical_shl(d.l);
  bool cls = du.l[S::L - 1] >= 0 && du.l[S::L - 1] < (1 << 27);
  for (int i = 0; i < S::L - 1; i++) cls = cls && du.l[i] >= 0 && du.l[i] < (1 << 30);
  CHECK(cls, "from_canonical_u class");
  i32 dif[S::L];
  for (int i = 0; i < S::L; i++) dif[i] = du.l[i] - ds.l[i];   // digit-wise in (-2^29, 3 2^29): the value 0
  CHECK(S::sweep<true>(dif).is_zero_digits(), "from_canonical_u value");
  for (const S* y : {&a, &b, &c, &m}) {
    const S pu = S::mul(du, *y), ps = S::mul(ds, *y);
    CHECK(same_digits(pu, ps) && same_digits(S::mul(*y, du), ps), "product of the unsigned operand");
    put(ps);
  }
}

// one entry of a run: LazySK::madd (the kernel's entry) against xyzz_madd_s on RECODED operands (the retained functions)
static void add_entry(XYZZS<P>& acc, XYZZS<P>& old, const F& x, const F& y, bool neg) {
  Affine<F> p;
  p.x = x;
  p.y = y;
  char raw[2 * F::BYTES];
  x.store(raw);
  y.store(raw + F::BYTES);
  if (K::madd(acc, p, neg)) K::mdbl(acc, raw, neg);
  if (xyzz_madd_s<P>(old, S::from_canonical_shl(x.l), S::from_canonical_shl(F::cond_neg(y, neg).l))) xyzz_mdbl_s<P>(old, raw, neg);
  CHECK(same_acc(acc, old), "LazySK::madd against xyzz_madd_s on recoded operands");
  put(acc);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::mt19937_64 g(31);
  // ---- random operands, negative digits ------------------------------------------------------------------------------------
  const S one = S::one();
  for (int it = 0; it < 1500; it++) {
    const F a = rnd(g), b = rnd(g), c = rnd(g), d = rnd(g);
    const S ra = S::mul(S::from_canonical_shl(a.l), one), rb = S::mul(S::from_canonical_shl(b.l), one), rc = S::mul(S::from_canonical_shl(c.l), one);
    check_ops(ra, rb, rc, d);
    check_ops(S::neg(ra), S::sub(rb, rc), S::neg(rc), a);            // negative digits, a swept difference
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
    // gathered coordinates at their limits: p - 1 (the largest), 2^380 - 1 (every digit below the top at 2^30 - 1), 0, 1
    std::vector<F> gat;
    F v = F::zero();
    gat.push_back(v);
    v.l[0] = 1;
    gat.push_back(v);
    for (int i = 0; i < P::N; i++) v.l[i] = P::P[i];
    v.l[0] -= 1;
    gat.push_back(v);
    for (int i = 0; i < P::N; i++) v.l[i] = 0xffffffffu;
    v.l[P::N - 1] = (1u << 28) - 1;
    gat.push_back(v);
    for (size_t i = 0; i < edge.size(); i++)
      for (size_t j = 0; j < edge.size(); j++) check_ops(edge[i], edge[j], edge[(i + 3 * j + 1) % edge.size()], gat[(i + j) % gat.size()]);
  }
  // ---- runs of entries -----------------------------------------------------------------------------------------------------
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
    auto fresh = [] { return K::inf(); };
    // P P | P -P | P -P Q | P P P | P -P P P, each with the first entry's digit positive and negative
    for (int k = 0; k < 8; k++)
      for (int sg = 0; sg < 2; sg++) {
        const bool n = sg != 0;
        const int q = (k + 5) % NPT;
        { XYZZS<P> a = fresh(), o = fresh(); add_entry(a, o, px[k], py[k], n); add_entry(a, o, px[k], py[k], n); put(K::to_bucket(a)); }
        { XYZZS<P> a = fresh(), o = fresh(); add_entry(a, o, px[k], py[k], n); add_entry(a, o, px[k], py[k], !n); put(K::to_bucket(a)); }
        { XYZZS<P> a = fresh(), o = fresh(); add_entry(a, o, px[k], py[k], n); add_entry(a, o, px[k], py[k], !n); add_entry(a, o, px[q], py[q], n); put(K::to_bucket(a)); }
        { XYZZS<P> a = fresh(), o = fresh(); for (int r = 0; r < 3; r++) add_entry(a, o, px[k], py[k], n); put(K::to_bucket(a)); }
        { XYZZS<P> a = fresh(), o = fresh(); add_entry(a, o, px[k], py[k], n); add_entry(a, o, px[k], py[k], !n); add_entry(a, o, px[k], py[k], n); add_entry(a, o, px[k], py[k], n); put(K::to_bucket(a)); }
      }
    // random chains; now and then the same point again, its inverse, and a stored bucket reloaded (a streamed MSM's later piece)
    for (int trial = 0; trial < 300; trial++) {
      XYZZS<P> a = fresh(), o = fresh();
      const int len = 1 + g() % 12;
      for (int s = 0; s < len; s++) {
        const int k = g() % NPT;
        const bool n = g() & 1;
        add_entry(a, o, px[k], py[k], n);
        if (trial % 3 == 0) add_entry(a, o, px[k], py[k], n);
        if (trial % 7 == 0) add_entry(a, o, px[k], py[k], !n);
        if (trial % 4 == 1 && s == len / 2) {
          const XYZZ<F> stored = K::to_bucket(a);
          put(stored);
          a = K::from_bucket(stored);
          o = K::from_bucket(stored);
        }
      }
      put(K::to_bucket(a));
    }
  }
  FILE* f = fopen(argv[1], "wb");
  if (!f) return 3;
  if (fwrite(rec.data(), 4, rec.size(), f) != rec.size()) return 4;
  fclose(f);
  printf("BLS12_381_FQ signed30 unsigned gather=%d: %s (%d bad, %zu words)\n", (int)ARK_S30_UNSIGNED_GATHER, bad ? "FAIL" : "ok", bad, rec.size());
  return bad != 0;
}
