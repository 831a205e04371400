// The mixed addition of the bucket-accumulation kernel on 13 signed 30-bit digits (fp30s.cuh): the formulas and special
// cases of xyzz_madd_lazy (ec28.cuh; bucket.rs:168-238, madd-2008-s), 3055 multiply-adds per addition instead of 3542 (3103 with the
// differences folded into the products).
//
// Bases and buckets live in HBM in the reference's canonical form (radix 2^384).  A gathered coordinate enters by repacking
// only (FpS::from_canonical_u: the residue itself in radix 2^390, in [0, 64 p)); buckets leave through FpS::to_canonical.
//
// Residues are SIGNED and unreduced: a difference is a digit-wise subtraction and one signed carry sweep, nothing adds a
// multiple of p -- and where a product computes the minuend and nothing else reads it (P = U2 - X1, R = S2 - Y1, X3 = R^2 - PPP -
// 2 Q), the subtrahend's digits leave inside the product's high columns instead (FpS::mul_sub, FpS::sqr_sub2; ARK_S30_FUSED_DIFF):
// the same digits without the subtraction and its sweep, one multiply-add per digit (48 in all); only t = Q - X3 keeps a sweep.
// Every product operand is normalised (digits 0..11 in [-2^29, 2^29]) -- but for the gathered coordinate, which is unsigned beside a
// normalised operand -- which is what the column bounds of fp30s.cuh ask for.  Bounds in the comments are |value| in units of p,
// with R' / p > 629.9 and a product's
// |a b| / R' + 0.5001;  the accumulator invariant is
//     |x| < 2.02,  |y| < 0.61,  |zz|, |zzz| < 1          (all n)
// re-derived exactly by tests/lazy30_model.py.
//
// "Is this difference zero mod p" is asked of the SQUARE that follows it, as in ec28.cuh: PP = P^2 is a product's output,
// |PP| < p and its digits are the unique balanced ones, so PP = 0 mod p exactly when every digit is zero.
//
// The FULL addition of the reduction, heavy-run and parts-sum kernels (xyzz_add_s, with its doubling xyzz_dbl_s; the formulas and
// special cases of xyzz_add_lazy) lives on the same digits and the same invariant, so accumulators pass between the two additions
// freely: 10 products + 2 squares + one two-product sum = 10 * 338 + 2 * 260 + 507 = 4407 multiply-adds (+ 48 for the three
// differences folded into their products) instead of the 28-bit form's 5110.  Both of its operands are sums, so its bounds are its
// own: stated at the routine, re-derived exactly by tests/lazy30_add_model.py.
#pragma once
#include "ec28.cuh"
#include "fp30s.cuh"

// 1 (default): a gathered coordinate enters unsigned; 0: recoded to signed digits, the kernel as it first shipped (A/B builds)
#ifndef ARK_S30_UNSIGNED_GATHER
#define ARK_S30_UNSIGNED_GATHER 1
#endif
// Differences folded into the product that computes them (FpS::mul_sub, FpS::sqr_sub2): bit 0: P = U2 - X1 and R = S2 - Y1,
// bit 1: X3 = R^2 - PPP - 2 Q.  3 (default): both; 0: every difference digit-wise with its own carry sweep, the chain as it was
// (A/B builds; 1 and 2 measure each fusion alone).  The digits are the same under every setting.
#ifndef ARK_S30_FUSED_DIFF
#define ARK_S30_FUSED_DIFF 3
#endif

namespace arkhip {

template <class P>
struct XYZZS {
  FpS<P> x, y, zz, zzz;
  bool inf;
};

// a gathered base (canonical limbs; the digit's sign already applied to y) as product operands: values in [0, 64).  Each is ONE
// operand of U2 = x2 zz, of S2 = y2 zzz or of the first point's product by one, whose other operand is normalised, and of
// nothing else: it stays unsigned (FpS::from_canonical_u) and skips the signed recoding -- a carry add, a sign-extending extract
// and a carry per digit, 98 vector instructions per addition.  U2, S2 and everything after them are digit for digit what the
// recoded operand gives (tests/lazy30_diet_host_check.hip, tests/test_gpu_lazy30_diet.py).
template <class P>
ARK_HD void s30_from_affine(const Fp<P>& x, const Fp<P>& y, FpS<P>& xs, FpS<P>& ys) {
#if ARK_S30_UNSIGNED_GATHER
  xs = FpS<P>::from_canonical_u(x.l);
  ys = FpS<P>::from_canonical_u(y.l);
#else
  xs = FpS<P>::from_canonical_shl(x.l);
  ys = FpS<P>::from_canonical_shl(y.l);
#endif
}
// stored bucket -> accumulator: repack, then one product with the residue 1 per coordinate: < 64 / 629.9 + 0.5001 < 0.602
template <class P>
ARK_HD XYZZS<P> s30_from_bucket(const XYZZ<Fp<P>>& b) {
  typedef FpS<P> F;
  XYZZS<P> r;
  r.inf = b.is_zero();
  const F one = F::one();
  r.x = F::mul(F::from_canonical_shl(b.x.l), one);
  r.y = F::mul(F::from_canonical_shl(b.y.l), one);
  r.zz = F::mul(F::from_canonical_shl(b.zz.l), one);
  r.zzz = F::mul(F::from_canonical_shl(b.zzz.l), one);
  return r;
}
// accumulator -> bucket in the reference's canonical form (|coordinate| < 2.02 < OUT_K = 4)
template <class P>
ARK_HD XYZZ<Fp<P>> s30_to_bucket(const XYZZS<P>& a) {
  if (a.inf) return XYZZ<Fp<P>>::zero();
  XYZZ<Fp<P>> r;
  r.x = a.x.to_canonical();
  r.y = a.y.to_canonical();
  r.zz = a.zz.to_canonical();
  r.zzz = a.zzz.to_canonical();
  return r;
}
// acc = 2 (+-) base at `src`: rare (duplicate bases), so it goes through the 28-bit doubling and the canonical form, which
// keeps the hot loop's registers free of it; expanded in place (ARK_COLD_HD), no call frame
template <class P>
ARK_COLD_HD void xyzz_mdbl_s(XYZZS<P>& acc, const char* src, bool neg) {
  XYZZL<P> d;
  xyzz_mdbl_lazy<P>(d, src, neg);
  acc = s30_from_bucket<P>(lazy_to_bucket<P>(d));
}

// acc += (x2, y2): a non-identity base from s30_from_affine.  Returns true when the base EQUALS the accumulated point: the
// caller then replaces the accumulator by the doubling of the base (xyzz_mdbl_s), as with xyzz_madd_lazy.
template <class P>
ARK_HD bool xyzz_madd_s(XYZZS<P>& acc, const FpS<P>& x2, const FpS<P>& y2) {
  typedef FpS<P> F;
  if (acc.inf) {
    const F one = F::one();
    acc.x = F::mul(x2, one);                          // < 64 * 1 / 629.9 + 0.5001 < 0.602 (n)
    acc.y = F::mul(y2, one);                          // < 0.602 (n)
    acc.zz = one;                                     // in [0, 1) (n)
    acc.zzz = one;
    acc.inf = false;
    return false;
  }
#if ARK_S30_FUSED_DIFF & 1
  // U2 = x2 zz and S2 = y2 zzz (< 64 * 1 / 629.9 + 0.5001 < 0.602) have no other consumer: X1 and Y1 leave inside the high columns
  const F pd = F::mul_sub(x2, acc.zz, acc.x);         // P = U2 - X1: < 0.602 + 2.02 < 2.63 (n: the columns' own digits)
  const F rd = F::mul_sub(y2, acc.zzz, acc.y);        // R = S2 - Y1: < 0.602 + 0.61 < 1.22 (n)
#else
  const F u2 = F::mul(x2, acc.zz);                    // < 64 * 1 / 629.9 + 0.5001 < 0.602 (n)
  const F s2 = F::mul(y2, acc.zzz);                   // < 0.602 (n)
  const F pd = F::sub(u2, acc.x);                     // P = U2 - X1: < 0.602 + 2.02 < 2.63 (n, swept)
  const F rd = F::sub(s2, acc.y);                     // R = S2 - Y1: < 0.602 + 0.61 < 1.22 (n, swept)
#endif
  const F pp = F::sqr(pd);                            // < 2.63^2 / 629.9 + 0.5001 < 0.5111 (n): |PP| < p, the zero test is exact
  if (pp.is_zero_digits()) {                          // P = 0 mod p: same x -- doubling or infinity (bucket.rs:176-200)
    if (F::sqr(rd).is_zero_digits()) return true;     // R = 0 mod p as well (|R^2 / R'| < 0.5025): the same point
    acc.inf = true;
    return false;
  }
  const F ppp = F::mul(pd, pp);                       // < 2.63 * 0.5111 / 629.9 + 0.5001 < 0.5023 (n)
  const F q = F::mul(acc.x, pp);                      // < 2.02 * 0.5111 / 629.9 + 0.5001 < 0.5018 (n)
#if ARK_S30_FUSED_DIFF & 2
  // R^2 (< 0.5025) and PPP + 2 Q (< 1.506) have no other consumer: a high column takes - ppp_i - 2 q_i, at most 3 2^29 more
  const F x3 = F::sqr_sub2(rd, ppp, q);               // R^2 - PPP - 2 Q: < 0.5025 + 1.506 < 2.009 (n: the columns' own digits)
#else
  const F e = F::add_2b(ppp, q);                      // PPP + 2 Q: < 1.506 (n, swept; digits before the sweep <= 3 2^29)
  const F x3 = F::sub(F::sqr(rd), e);                 // R^2 - PPP - 2 Q: < 0.5025 + 1.506 < 2.009 (n, swept)
#endif
  const F t = F::sub(q, x3);                          // Q - X3: < 2.511 (n, swept)
  // Y3 = R (Q - X3) - Y1 PPP as ONE sum of two products: (1.22 * 2.511 + 0.61 * 0.5023) / 629.9 + 0.5001 < 0.506.
  // All four operands n with top digits below 2^23 (|value| < 2.63 p < 2^383): the 26-term column of fp30s.cuh.
  acc.y = F::sop2(rd, t, F::neg(acc.y), ppp);
  acc.zz = F::mul(acc.zz, pp);                        // < 1 * 0.5111 / 629.9 + 0.5001 < 0.501 (n)
  acc.zzz = F::mul(acc.zzz, ppp);                     // < 0.501 (n)
  acc.x = x3;
  return false;
}

// ---- full addition (the reduction, heavy-run and parts kernels; ARK_REDUCE_S30 in lazyk.cuh) ------------------------------------------
// a stored point (canonical limbs) as the operand b of xyzz_add_s: values in [0, 64).  Every coordinate of b meets NORMALISED
// operands only (x2 ZZ1, y2 ZZZ1, X1 zz2, Y1 zzz2, ZZ1 zz2, ZZZ1 zzz2, or the residue 1 when the accumulator is empty) and is
// read by nothing but products: it stays unsigned, as a gathered base does (the exception at the top of fp30s.cuh).
template <class P>
ARK_HD XYZZS<P> s30_operands_of(const XYZZ<Fp<P>>& b) {
  typedef FpS<P> F;
  XYZZS<P> r;
  r.inf = b.is_zero();
#if ARK_S30_UNSIGNED_GATHER
  r.x = F::from_canonical_u(b.x.l);
  r.y = F::from_canonical_u(b.y.l);
  r.zz = F::from_canonical_u(b.zz.l);
  r.zzz = F::from_canonical_u(b.zzz.l);
#else
  r.x = F::from_canonical_shl(b.x.l);
  r.y = F::from_canonical_shl(b.y.l);
  r.zz = F::from_canonical_shl(b.zz.l);
  r.zzz = F::from_canonical_shl(b.zzz.l);
#endif
  return r;
}
// acc = 2 acc for an accumulator that is not at infinity (dbl-2008-s-1, a = 0; bucket.rs:112-146), as xyzz_dbl_lazy does it on 28-bit
// limbs: X3 and Y3 from (X1, Y1) alone, ZZ3 = V ZZ1, ZZZ3 = W ZZZ1.  Rare (equal sums meeting), expanded in place (ARK_COLD_HD), no call
// frame.  On the digits themselves, NOT through the canonical form and the 28-bit doubling as xyzz_mdbl_s goes: that round trip, inlined
// with the accumulator and the other operand alive, was the widest point of every kernel that adds (msm_reduce_level_kernel 256 VGPRs
// instead of 213; msm_heavy_combine_kernel 256 + 2 AGPRs, one wave per SIMD instead of two).  Bounds from the invariant:
//   U = 2 Y1 < 1.22 (n, swept),  V = U^2 < 0.5025,  W = U V < 0.5011,  S = X1 V < 0.5018,  XX = X1^2 < 0.5066,  M = 3 XX < 1.52 (n, swept)
//   X3 = M^2 - 2 S < 1.508,  t = S - X3 < 2.01,  Y3 = M t - W Y1 < 0.5055,  ZZ3 = V ZZ1, ZZZ3 = W ZZZ1 < 0.501       (n)
template <class P>
ARK_COLD_HD void xyzz_dbl_s(XYZZS<P>& acc) {
  typedef FpS<P> F;
  const F u = F::add(acc.y, acc.y);
  const F v = F::sqr(u);
  const F w = F::mul(u, v);
  const F s = F::mul(acc.x, v);
  const F xx = F::sqr(acc.x);
  const F m = F::add_2b(xx, xx);                      // digits before the sweep <= 3 2^29
  const F x3 = F::sqr_sub2(m, F::zero(), s);          // M^2 - 2 S
  const F t = F::sub(s, x3);
  acc.y = F::sop2(m, t, F::neg(w), acc.y);            // M (S - X3) - W Y1
  acc.zz = F::mul(v, acc.zz);
  acc.zzz = F::mul(w, acc.zzz);
  acc.x = x3;
}
// acc += b: the formulas and special cases of xyzz_add_lazy (ec28.cuh; add-2008-s, bucket.rs:256-337).  b is another accumulator
// (inside the invariant) or a stored point from s30_operands_of (values in [0, 64), unsigned digits).  Bounds, |value| in units
// of p, from the invariant |x| < 2.02, |y| < 0.61, |zz|, |zzz| < 1 with b at 64 (re-derived exactly by tests/lazy30_add_model.py):
//   U1 = X1 ZZ2 < 2.02 * 64 / 629.9 + 0.5001 < 0.706,  S1 = Y1 ZZZ2 < 0.61 * 64 / 629.9 + 0.5001 < 0.563            (n)
//   P = X2 ZZ1 - U1 < 0.602 + 0.706 < 1.308,  R = Y2 ZZZ1 - S1 < 0.602 + 0.563 < 1.165     (n: the high columns' own digits)
//   PP < 1.308^2 / 629.9 + 0.5001 < 0.5029,  PPP < 0.5012,  Q = U1 PP < 0.5007,  R^2 / R' < 0.5023                      (n)
//   X3 = R^2 - PPP - 2 Q < 2.006,  t = Q - X3 < 2.507,  Y3 = R t - S1 PPP < 0.5053                                     (n)
//   ZZ1 ZZ2, ZZZ1 ZZZ2 < 0.602,  ZZ3, ZZZ3 < 0.5006                                                                  (n)
// which is the invariant again; an empty accumulator takes b through one product by one per coordinate (< 0.602).  Equal points
// (P = R = 0 mod p) double the accumulator in place (xyzz_dbl_s), opposite ones leave infinity.
template <class P>
ARK_HD void xyzz_add_s(XYZZS<P>& acc, const XYZZS<P>& b) {
  typedef FpS<P> F;
  if (b.inf) return;
  if (acc.inf) {
    const F one = F::one();
    acc.x = F::mul(b.x, one);
    acc.y = F::mul(b.y, one);
    acc.zz = F::mul(b.zz, one);
    acc.zzz = F::mul(b.zzz, one);
    acc.inf = false;
    return;
  }
  const F u1 = F::mul(acc.x, b.zz);
  const F s1 = F::mul(acc.y, b.zzz);
  const F pd = F::mul_sub(b.x, acc.zz, u1);           // P = U2 - U1: U2 has no other consumer
  const F rd = F::mul_sub(b.y, acc.zzz, s1);          // R = S2 - S1
  const F pp = F::sqr(pd);                            // |PP| < p: the zero test is exact
  if (pp.is_zero_digits()) {                          // P = 0 mod p: the same x -- doubling or infinity (bucket.rs:279-290)
    if (F::sqr(rd).is_zero_digits()) {
      xyzz_dbl_s<P>(acc);
    } else {
      acc.inf = true;
    }
    return;
  }
  const F ppp = F::mul(pd, pp);
  const F q = F::mul(u1, pp);
  const F x3 = F::sqr_sub2(rd, ppp, q);               // R^2 - PPP - 2 Q
  const F t = F::sub(q, x3);                          // Q - X3 (n, swept)
  acc.y = F::sop2(rd, t, F::neg(s1), ppp);            // R (Q - X3) - S1 PPP: four normalised operands, top digits below 2^23
  acc.zz = F::mul(F::mul(acc.zz, b.zz), pp);
  acc.zzz = F::mul(F::mul(acc.zzz, b.zzz), ppp);
  acc.x = x3;
}

}  // namespace arkhip
