// Host-side check of the full addition on 13 signed 30-bit digits (algebra_amd/csrc/ec30s.cuh: xyzz_add_s, the portable _c forms
// of fp30s.cuh) against the 28-bit xyzz_add_lazy (ec28.cuh) it replaces in the reduction, heavy-run and parts kernels.
//   * every sum leaves in the reference's canonical form on both sides and is compared canonical limb for canonical limb: the
//     operations mod p are the same, so the stored values must be;
//   * an accumulator of the signed form enters the 28-bit side through its stored form (s30_to_bucket, lazy_from_bucket): the same
//     residues, whatever digits held them -- this is how accumulators at the limits of the invariant are compared.
// Inputs: sums of multiples of the generator (stored point + stored point, accumulator + accumulator, chains through parked
// accumulators), P + P (the doubling), P + (-P), inf + P, P + inf, inf + inf, the same sums with different denominators,
// accumulators with every digit at +-2^29 and the top digit at the limit of its class against stored coordinates 0, 1, p - 1 and
// 2^380 - 1, random residues.  Built with -fsanitize=undefined,address on the host code.
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
typedef LazySK<C> K;      // the signed form
typedef LazyK<C> K28;     // the 28-bit form

static int bad = 0;
static long checked = 0;
#define CHECK(COND, WHAT) do { checked++; if (!(COND)) { bad++; if (bad < 12) printf("FAIL %s (line %d)\n", WHAT, __LINE__); } } while (0)

static bool same_fe(const F& a, const F& b) {
  for (int i = 0; i < P::N; i++) if (a.l[i] != b.l[i]) return false;
  return true;
}
static bool same_pt(const XYZZ<F>& a, const XYZZ<F>& b) {
  if (a.is_zero() || b.is_zero()) return a.is_zero() == b.is_zero();
  return same_fe(a.x, b.x) && same_fe(a.y, b.y) && same_fe(a.zz, b.zz) && same_fe(a.zzz, b.zzz);
}
static bool canonical(const F& a) {   // below p
  for (int i = P::N - 1; i >= 0; i--) if (a.l[i] != P::P[i]) return a.l[i] < P::P[i];
  return false;
}
static F rnd(std::mt19937_64& g) {
  F a;
  for (int i = 0; i < P::N; i++) a.l[i] = (u32)g();
  a.l[P::N - 1] &= (1u << ((P::BITS - 1) % 32)) - 1;   // < 2^(BITS-1) < p
  return a;
}
// the 28-bit accumulator holding the residues of a signed one
static XYZZL<P> as28(const XYZZS<P>& a) { return a.inf ? K28::inf() : K28::from_bucket(s30_to_bucket<P>(a)); }

// acc + b, b a stored point: xyzz_add_s against xyzz_add_lazy; then the same with b in an accumulator of its own (add_acc on both)
static XYZZ<F> check_add(const XYZZS<P>& acc, const XYZZ<F>& b, const char* what) {
  XYZZS<P> s = acc;
  XYZZL<P> l = as28(acc);
  K::add(s, b);
  K28::add(l, b);
  const XYZZ<F> rs = K::to_bucket(s), rl = K28::to_bucket(l);
  CHECK(same_pt(rs, rl), what);
  CHECK(rs.is_zero() || (canonical(rs.x) && canonical(rs.y) && canonical(rs.zz) && canonical(rs.zzz)), "canonical limbs");
  XYZZS<P> s2 = acc, bs = K::inf();
  XYZZL<P> l2 = as28(acc), bl = K28::inf();
  K::add(bs, b);
  K28::add(bl, b);
  K::add_acc(s2, bs);
  K28::add_acc(l2, bl);
  CHECK(same_pt(K::to_bucket(s2), K28::to_bucket(l2)), what);
  CHECK(same_pt(K::to_bucket(s2), rs), "accumulator + accumulator against accumulator + stored point");
  // through a parked slot
  i32 slot[K::WORDS];
  K::park(bs, slot);
  XYZZS<P> s3 = acc;
  K::add_acc(s3, K::unpark(slot));
  CHECK(same_pt(K::to_bucket(s3), rs), "parked operand");
  return rs;
}
static XYZZS<P> taken(const XYZZ<F>& a) {
  XYZZS<P> s = K::inf();
  K::add(s, a);
  return s;
}

int main() {
  std::mt19937_64 g(47);
  F gx = F::load(GEN_BLS12_381_G1), gy = F::load((const char*)GEN_BLS12_381_G1 + F::BYTES);
  const int NPT = 24;
  F px[NPT], py[NPT];
  XYZZ<F> mult[NPT];   // k G as the saturated formulas leave it: a denominator that is not one
  {
    XYZZ<F> run = XYZZ<F>::zero();
    for (int k = 0; k < NPT; k++) {
      xyzz_madd<F>(run, gx, gy);
      mult[k] = run;
      F zi = F::inverse(run.zzz);
      F zzi = F::sqr(F::mul(run.zz, zi));
      px[k] = F::mul(run.x, zzi);
      py[k] = F::mul(run.y, zi);
    }
  }
  auto affine_pt = [&](int k, bool neg) {
    XYZZ<F> b = XYZZ<F>::zero();
    xyzz_madd<F>(b, px[k], F::cond_neg(py[k], neg));
    return b;
  };
  auto negated = [](XYZZ<F> b) { b.y = F::cond_neg(b.y, true); return b; };
  const XYZZ<F> inf = XYZZ<F>::zero();
  // ---- the special cases, every pair of multiples -----------------------------------------------------------------------------
  check_add(K::inf(), inf, "inf + inf");
  for (int i = 0; i < NPT; i++) {
    check_add(K::inf(), mult[i], "inf + P");
    check_add(taken(mult[i]), inf, "P + inf");
    CHECK(!check_add(taken(mult[i]), mult[i], "P + P: doubling").is_zero(), "doubling is a point");
    CHECK(check_add(taken(mult[i]), negated(mult[i]), "P + (-P)").is_zero(), "P + (-P) is infinity");
    // the same point under two denominators: (k G as a sum) against (k G affine)
    CHECK(!check_add(taken(mult[i]), affine_pt(i, false), "P + P, different denominators").is_zero(), "doubling is a point");
    CHECK(check_add(taken(affine_pt(i, true)), mult[i], "-P + P, different denominators").is_zero(), "infinity");
    for (int j = 0; j < NPT; j++)
      if (i != j) check_add(taken(mult[i]), (i + j) & 1 ? mult[j] : affine_pt(j, (j & 2) != 0), "P + Q");
  }
  // ---- chains: mixed additions, full additions and a reload, as the heavy-run kernels and the LDS trees mix them -------------------
  for (int trial = 0; trial < 200; trial++) {
    XYZZS<P> s = K::inf();
    XYZZL<P> l = K28::inf();
    const int len = 1 + g() % 10;
    for (int t = 0; t < len; t++) {
      const int k = g() % NPT;
      const bool n = g() & 1;
      if (g() % 3 == 0) {
        Affine<F> p;
        p.x = px[k];
        p.y = py[k];
        char raw[2 * F::BYTES];
        p.x.store(raw);
        p.y.store(raw + F::BYTES);
        if (K::madd(s, p, n)) K::mdbl(s, raw, n);
        if (K28::madd(l, p, n)) K28::mdbl(l, raw, n);
      } else {
        const XYZZ<F> b = n ? negated(mult[k]) : mult[k];
        check_add(s, b, "chain");
        K::add(s, b);
        K28::add(l, b);
      }
      CHECK(same_pt(K::to_bucket(s), K28::to_bucket(l)), "chain: stored value");
      if (trial % 5 == 2 && t == len / 2) s = K::from_bucket(K::to_bucket(s));
    }
  }
  // ---- accumulators at the limits of the invariant (|x| < 2.02, |y| < 0.61, |zz|, |zzz| < 1 in units of p) against stored -----------
  // ---- coordinates at theirs: field values only, the addition is arithmetic ---------------------------------------------------
  {
    const double PTOP = 1704209.9;   // p / 2^360
    auto lim = [&](double units, int pat, int sign) {
      S x;
      for (int i = 0; i < S::L - 1; i++) {
        const i32 H = S::HALF;
        x.l[i] = sign * (pat == 0 ? H : pat == 1 ? ((i & 1) ? H : -H) : ((i & 1) ? -H : H - 1));
      }
      x.l[S::L - 1] = sign * (i32)(units * PTOP);
      return x;
    };
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
    gat.push_back(rnd(g));
    int n = 0;
    for (int pat = 0; pat < 3; pat++)
      for (int sx = -1; sx <= 1; sx += 2)
        for (int sy = -1; sy <= 1; sy += 2)
          for (int sz = -1; sz <= 1; sz += 2) {
            XYZZS<P> a;
            a.inf = false;
            a.x = lim(2.02, pat, sx);
            a.y = lim(0.61, pat, sy);
            a.zz = lim(0.999, pat, sz);
            a.zzz = lim(0.999, (pat + 1) % 3, -sz);
            for (size_t i = 0; i < gat.size(); i++)
              for (size_t j = 0; j < gat.size(); j++) {
                XYZZ<F> b;
                b.x = gat[i];
                b.y = gat[j];
                b.zz = gat[(i + j + n) % gat.size()];
                b.zzz = gat[(i + 2 * j + n + 1) % gat.size()];
                if (b.zz.is_zero()) b.zz = gat[2];   // zz = 0 is the identity, checked above
                check_add(a, b, "class limits");
                n++;
              }
          }
  }
  // ---- random residues (no curve behind them) ----------------------------------------------------------------------------------
  for (int it = 0; it < 400; it++) {
    XYZZ<F> a, b;
    a.x = rnd(g); a.y = rnd(g); a.zz = rnd(g); a.zzz = rnd(g);
    b.x = rnd(g); b.y = rnd(g); b.zz = rnd(g); b.zzz = rnd(g);
    check_add(taken(a), b, "random residues");
    check_add(K::from_bucket(a), b, "random residues, reloaded accumulator");
  }
  // ---- buckets of one, two and three entries through the mixed addition, mixed with the full one -----------------------------------
  for (int k = 0; k < NPT; k++)
    for (int sg = 0; sg < 4; sg++) {
      const int q = (k + 7) % NPT, r = (k + 11) % NPT;
      const int second[4] = {q, k, k, q};              // another point, the same point (doubling), its inverse, another point
      const bool n1 = sg & 1, n2 = sg == 2 ? !n1 : n1;
      Affine<F> p1, p2, p3;
      p1.x = px[k]; p1.y = py[k];
      p2.x = px[second[sg]]; p2.y = py[second[sg]];
      p3.x = px[r]; p3.y = py[r];
      char raw[2 * F::BYTES];
      p2.x.store(raw);
      p2.y.store(raw + F::BYTES);
      XYZZS<P> s = K::inf();
      XYZZL<P> l = K28::inf();
      K::madd(s, p1, n1);
      K28::madd(l, p1, n1);
      CHECK(same_pt(K::to_bucket(s), K28::to_bucket(l)), "one entry");
      check_add(s, mult[q], "one entry + a sum");
      const bool eq = K::madd(s, p2, n2);
      CHECK(eq == (sg == 1), "equal points");
      if (eq) K::mdbl(s, raw, n2);
      if (K28::madd(l, p2, n2)) K28::mdbl(l, raw, n2);
      CHECK(s.inf == (sg == 2), "infinity");
      CHECK(same_pt(K::to_bucket(s), K28::to_bucket(l)), "two entries");
      check_add(s, mult[r], "two entries + a sum");
      K::madd(s, p3, n1);
      K28::madd(l, p3, n1);
      CHECK(same_pt(K::to_bucket(s), K28::to_bucket(l)), "three entries");
    }
  printf("BLS12_381_FQ signed30 full addition: %s (%d bad of %ld checks)\n", bad ? "FAIL" : "ok", bad, checked);
  return bad != 0;
}
