// Host-side check of the signed 13 x 30-bit arithmetic of the plain accumulate kernel (algebra_amd/csrc/fp30s.cuh, ec30s.cuh)
// against the saturated form (fp.cuh / ec.cuh, itself checked against the oracle on the GPU) and, bucket for bucket and word
// for word, against the 28-bit form it replaces (ec28.cuh).  The templates are __host__ __device__: compiled for the host,
// FpS::mul / sqr / sop2 are the portable _c forms.  Inputs are random AND the class-limit vectors: every digit at +-2^29,
// alternating signs, 0, +-1, p - 1, residues at the value bounds of ec30s.cuh.  Built (with -fsanitize=undefined,address: the
// portable forms must be free of signed-overflow undefined behaviour) and run by tests/test_lazy30_host.py.
#include "ec30s.cuh"
#include "curves.cuh"
#include <stdio.h>
#include <random>
#include <vector>
using namespace arkhip;
typedef BLS12_381_FQ P;
typedef Fp<P> F;
typedef FpS<P> S;

static F rnd(std::mt19937_64& g) {
  F a;
  for (int i = 0; i < P::N; i++) a.l[i] = (u32)g();
  a.l[P::N - 1] &= (1u << ((P::BITS - 1) % 32)) - 1;   // < 2^(BITS-1) < p
  return a;
}
static F small(u32 v) {   // the integer v < 2^30 as canonical bits
  F r = F::zero();
  r.l[0] = v;
  return r;
}
// the residue a signed value stands for, as a canonical Fp (radix R): the integer sum l_i 2^(30 i) mod p by Horner over
// canonical additions, subtractions and doublings (independent of every function of fp30s.cuh), then v R = (v R') 2^-6
static F value_of(const S& a) {
  F acc = F::zero();
  for (int i = S::L - 1; i >= 0; i--) {
    for (int b = 0; b < S::W; b++) acc = F::dbl(acc);
    const i64 d = a.l[i];
    // |top digit| may exceed 2^30 nowhere in these tests
    acc = d >= 0 ? F::add(acc, small((u32)d)) : F::sub(acc, small((u32)(-d)));
  }
  for (int k = 0; k < S::SH; k++) {   // halve mod p
    u32 c = 0;
    F x = acc;
    if (x.l[0] & 1) { for (int i = 0; i < P::N; i++) { u64 s = (u64)x.l[i] + P::P[i] + c; x.l[i] = (u32)s; c = (u32)(s >> 32); } }
    for (int i = 0; i < P::N - 1; i++) x.l[i] = (x.l[i] >> 1) | (x.l[i + 1] << 31);
    x.l[P::N - 1] = (x.l[P::N - 1] >> 1) | (c << 31);
    acc = x;
  }
  return acc;
}
static bool normalised(const S& a, i32 top) {   // digits 0..11 in [-2^29, 2^29), |top digit| <= top
  for (int i = 0; i < S::L - 1; i++) if (a.l[i] < -S::HALF || a.l[i] >= S::HALF) return false;
  return a.l[S::L - 1] <= top && a.l[S::L - 1] >= -top;
}
static bool same_digits(const S& a, const S& b) {
  for (int i = 0; i < S::L; i++) if (a.l[i] != b.l[i]) return false;
  return true;
}
static bool same_words(const XYZZ<F>& a, const XYZZ<F>& b) {
  return F::eq(a.x, b.x) && F::eq(a.y, b.y) && F::eq(a.zz, b.zz) && F::eq(a.zzz, b.zzz);
}

static int bad = 0;
#define CHECK(COND, WHAT) do { if (!(COND)) { bad++; if (bad < 12) printf("FAIL %s (line %d)\n", WHAT, __LINE__); } } while (0)

// every product form on (a, b, c, d), values against the saturated field, digits of the three forms against each other
static void check_products(const S& a, const S& b, const S& c, const S& d) {
  const F va = value_of(a), vb = value_of(b), vc = value_of(c), vd = value_of(d);
  const S m = S::mul(a, b), mc = S::mul_c(a, b);
  CHECK(same_digits(m, mc) && normalised(m, 1 << 24), "mul digits");
  CHECK(F::eq(value_of(m), F::mul(va, vb)), "mul value");
  const S q = S::sqr(a), qc = S::sqr_c(a);
  CHECK(same_digits(q, qc) && same_digits(q, S::mul_c(a, a)) && normalised(q, 1 << 24), "sqr digits");
  CHECK(F::eq(value_of(q), F::mul(va, va)), "sqr value");
  const S s = S::sop2(a, b, c, d), sc = S::sop2_c(a, b, c, d);
  CHECK(same_digits(s, sc) && normalised(s, 1 << 24), "sop2 digits");
  CHECK(F::eq(value_of(s), F::add(F::mul(va, vb), F::mul(vc, vd))), "sop2 value");
  CHECK(F::eq(value_of(S::sub(m, q)), F::sub(F::mul(va, vb), F::mul(va, va))) && normalised(S::sub(m, q), 1 << 26), "sub");   // top digits: a^2 of a repacked base reaches 7 p
  CHECK(F::eq(value_of(S::add_2b(m, q)), F::add(F::mul(va, vb), F::dbl(F::mul(va, va)))) && normalised(S::add_2b(m, q), 1 << 26), "add_2b");
  CHECK(F::eq(value_of(S::add(m, q)), F::add(F::mul(va, vb), F::mul(va, va))) && normalised(S::add(m, q), 1 << 26), "add");
  CHECK(F::eq(value_of(S::neg(m)), F::neg(F::mul(va, vb))), "neg");
  CHECK(F::eq(m.to_canonical(), F::mul(va, vb)) && F::eq(s.to_canonical(), value_of(s)), "to_canonical");
  // a product's output is below p in magnitude: zero mod p (an operand is 0 or 2 p) exactly when every digit is zero
  CHECK(S::sub(m, mc).is_zero_digits() && m.is_zero_digits() == F::eq(F::mul(va, vb), F::zero()), "is_zero_digits");
}

int main() {
  std::mt19937_64 g(30);
  // ---- constants --------------------------------------------------------------------------------------------------------
  {
    S p;
    for (int i = 0; i < S::L; i++) p.l[i] = S::S::P[i];
    CHECK(F::eq(value_of(p), F::zero()) && normalised(p, 1 << 21), "digits of p");
    CHECK(F::eq(value_of(S::one()), F::one()) && normalised(S::one(), 1 << 21), "residue 1");
    S kp;
    for (int i = 0; i < S::L; i++) kp.l[i] = S::S::OUT_KP[i];
    CHECK(F::eq(value_of(kp), F::zero()) && same_digits(kp, S::add(S::add(p, p), S::add(p, p))), "OUT_K p");
    CHECK(((u64)S::S::INV * (u64)(u32)P::P[0] + 1) % (1u << 30) == 0, "-p^-1 mod 2^30");
  }
  // ---- random operands: canonical values repacked (below 64 p) and products of them (below 0.61 p) ------------------------
  for (int it = 0; it < 3000; it++) {
    const F a = rnd(g), b = rnd(g), c = rnd(g), d = rnd(g);
    const S sa = S::from_canonical_shl(a.l), sb = S::from_canonical_shl(b.l), sc = S::from_canonical_shl(c.l), sd = S::from_canonical_shl(d.l);
    CHECK(F::eq(value_of(sa), a) && normalised(sa, (1 << 27) + 1), "from_canonical_shl");
    const S one = S::one();
    const S ra = S::mul(sa, one), rb = S::mul(sb, one), rc = S::mul(sc, one), rd = S::mul(sd, one);
    CHECK(F::eq(ra.to_canonical(), a), "repack round trip");
    check_products(sa, rb, rc, rd);      // the base's class times an accumulator coordinate's
    check_products(ra, rb, rc, rd);
    check_products(S::sub(ra, rb), S::sub(rc, rd), S::neg(ra), rd);   // Y3's operand classes
  }
  // ---- class-limit vectors: raw digits -------------------------------------------------------------------------------------
  {
    std::vector<S> edge;
    auto fill = [&](auto f, i32 top) { S x; for (int i = 0; i < S::L - 1; i++) x.l[i] = f(i); x.l[S::L - 1] = top; edge.push_back(x); };
    const i32 H = S::HALF;
    const i32 TOP = 1 << 23;   // |value| < 2.63 p < 2^383: what ec30s.cuh's operands reach
    for (i32 top : {TOP, -TOP, 0}) {
      fill([&](int) { return H; }, top);                          // every digit at +2^29
      fill([&](int) { return -H; }, top);                         // every digit at -2^29
      fill([&](int i) { return (i & 1) ? H : -H; }, top);         // alternating signs
      fill([&](int i) { return (i & 1) ? -H : H; }, top);
      fill([&](int i) { return (i & 1) ? H - 1 : -H; }, top);     // the digits a product's output can really have
    }
    fill([&](int) { return 0; }, 0);                              // 0
    fill([&](int i) { return i == 0 ? 1 : 0; }, 0);               // +1
    fill([&](int i) { return i == 0 ? -1 : 0; }, 0);              // -1
    {
      S pm1;                                                      // p - 1 and 1 - p
      for (int i = 0; i < S::L; i++) pm1.l[i] = S::S::P[i];
      pm1.l[0] -= 1;
      edge.push_back(pm1);
      edge.push_back(S::neg(pm1));
    }
    {
      // residues at the value bounds: +-(2 p), +-(2.5 p) from the digits of p; 63 p + (p - 1) through the repack
      S p, p2, p25;
      for (int i = 0; i < S::L; i++) p.l[i] = S::S::P[i];
      p2 = S::add(p, p);
      i32 h[S::L];
      for (int i = 0; i < S::L; i++) h[i] = 5 * (S::S::P[i] / 2);   // ~2.5 p, digits below 3 2^29
      p25 = S::sweep<true>(h);
      edge.push_back(p2);
      edge.push_back(S::neg(p2));
      edge.push_back(p25);
      edge.push_back(S::neg(p25));
      F top = F::zero();
      for (int i = 0; i < P::N; i++) top.l[i] = P::P[i];
      top.l[0] -= 1;                                               // p - 1: the largest canonical input
      edge.push_back(S::from_canonical_shl(top.l));
    }
    for (size_t i = 0; i < edge.size(); i++)
      for (size_t j = 0; j < edge.size(); j++) {
        const S& a = edge[i];
        const S& b = edge[j];
        const S& c = edge[(i + 3 * j + 1) % edge.size()];
        const S& d = edge[(j + 5 * i + 2) % edge.size()];
        // sop2's column bound asks for top digits below 2^27: all of these have them
        check_products(a, b, c, d);
      }
  }
  // ---- point sequences: what the kernel does with a run of sorted entries, against the saturated form (the same group
  // element) and against the 28-bit form (the same stored bucket, word for word) ---------------------------------------------
  {
    F gx = F::load(GEN_BLS12_381_G1), gy = F::load((const char*)GEN_BLS12_381_G1 + F::BYTES);
    const int NPT = 40;
    F px[NPT], py[NPT];
    XYZZ<F> acc = XYZZ<F>::zero();
    for (int k = 0; k < NPT; k++) {
      xyzz_madd<F>(acc, gx, gy);
      F zi = F::inverse(acc.zzz);
      F zzi = F::sqr(F::mul(acc.zz, zi));
      px[k] = F::mul(acc.x, zzi);
      py[k] = F::mul(acc.y, zi);
    }
    for (int trial = 0; trial < 400; trial++) {
      XYZZ<F> c = XYZZ<F>::zero();
      XYZZL<P> lz;
      lz.inf = true;
      lz.x = lz.y = lz.zz = lz.zzz = FpL<P>::zero();
      XYZZS<P> sz;
      sz.inf = true;
      sz.x = sz.y = sz.zz = sz.zzz = S::zero();
      const int len = 1 + g() % 12;
      for (int s = 0; s < len; s++) {
        const int k = g() % NPT;
        const bool neg = g() & 1;
        auto add_entry = [&](bool ng) {
          const F yy = F::cond_neg(py[k], ng);
          char raw[2 * F::BYTES];
          px[k].store(raw);
          py[k].store(raw + F::BYTES);
          xyzz_madd<F>(c, px[k], yy);
          FpL<P> lx, ly;
          lazy_from_affine<P>(px[k], yy, lx, ly);
          if (xyzz_madd_lazy<P>(lz, lx, ly)) xyzz_mdbl_lazy<P>(lz, raw, ng);
          S sx, sy;
          s30_from_affine<P>(px[k], yy, sx, sy);
          if (xyzz_madd_s<P>(sz, sx, sy)) xyzz_mdbl_s<P>(sz, raw, ng);
          if (!sz.inf) {   // the accumulator invariant's digit classes
            CHECK(normalised(sz.x, 1 << 23) && normalised(sz.y, 1 << 22) && normalised(sz.zz, 1 << 22) && normalised(sz.zzz, 1 << 22), "accumulator digits");
          }
        };
        add_entry(neg);
        if (trial % 3 == 0) add_entry(neg);    // the same point again: the doubling branch
        if (trial % 7 == 0) add_entry(!neg);   // then its inverse: cancels (possibly to infinity, and comes back)
        if (trial % 4 == 1 && s == len / 2) {  // a streamed MSM's later piece: store the bucket, load it back, go on
          const XYZZ<F> stored = s30_to_bucket<P>(sz);
          CHECK(same_words(stored, lazy_to_bucket<P>(lz)), "stored piece differs from the 28-bit form's");
          sz = s30_from_bucket<P>(stored);
          lz = lazy_from_bucket<P>(stored);
        }
      }
      const XYZZ<F> d = s30_to_bucket<P>(sz);
      bool canon = true;
      const F* cs[4] = {&d.x, &d.y, &d.zz, &d.zzz};
      for (const F* f : cs) { F r = F::reduce_once(f->l); if (!F::eq(r, *f)) canon = false; }
      bool same;
      if (c.is_zero() || d.is_zero()) same = c.is_zero() && d.is_zero();
      else same = F::eq(F::mul(c.x, d.zz), F::mul(d.x, c.zz)) && F::eq(F::mul(c.y, d.zzz), F::mul(d.y, c.zzz)) &&
                  F::eq(F::mul(F::sqr(d.zz), d.zz), F::sqr(d.zzz));
      CHECK(same && canon, "point sequence against the saturated form");
      CHECK(same_words(d, lazy_to_bucket<P>(lz)), "stored bucket differs from the 28-bit form's");
    }
  }
  printf("BLS12_381_FQ signed30: %s (%d bad)\n", bad ? "FAIL" : "ok", bad);
  return bad != 0;
}
