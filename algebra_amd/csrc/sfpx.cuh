// Extension fields over the one-word fields of sfp.cuh, and the FRI fold of one row: the reference's own tower models over
// SmallFp<P> (ff/src/fields/models/fp2.rs, fp4.rs, quadratic_extension.rs).
//   Goldilocks:            Fp2 = Fp[u] / (u^2 - 7),                                degree D = 2
//   BabyBear / KoalaBear:  Fp4 = Fp2[v] / (v^2 - u), Fp2 = Fp[u] / (u^2 - W),      degree D = 4, W = 11 / 3
// An element is its D components in the order CanonicalSerialize writes them: c0, c1 for Fp2 and c0.c0, c0.c1, c1.c0, c1.c1 for
// Fp4, each a stored Montgomery word of the base field.  With X = v the quartic field is Fp[X] / (X^4 - W) and (a0, a1, b0, b1)
// is a0 + b0 X + a1 X^2 + b1 X^3.  Every function takes and returns canonical words, on the host and on the device alike: the
// host entries of capi_fri.hip and the kernels of sfp_fri.cuh run the same code.  Products are the schoolbook tower on canonical
// base-field products: no lazy sums, so no bound to keep.  DESIGN.md section 30.
#pragma once
#include "sfp.cuh"

namespace arkhip {

template <class Cfg>
struct SfpXCfg;
template <>
struct SfpXCfg<GOLDILOCKS> { static constexpr int D = 2; static constexpr uint64_t W = 7; };
template <>
struct SfpXCfg<BABYBEAR> { static constexpr int D = 4; static constexpr uint64_t W = 11; };
template <>
struct SfpXCfg<KOALABEAR> { static constexpr int D = 4; static constexpr uint64_t W = 3; };

template <class Cfg>
struct SFpX {
  using F = SFp<Cfg>;
  using T = typename Cfg::T;
  static constexpr int D = SfpXCfg<Cfg>::D;
  static constexpr T W_MONT = (T)sfp_mulmod(SfpXCfg<Cfg>::W, Cfg::R1, Cfg::P);       // the non-residue, as stored
  static constexpr T HALF_UP = (T)((Cfg::P + 1) / 2);
  struct E { T c[D]; };

  __host__ __device__ static inline E zero() {
    E r;
#pragma unroll
    for (int k = 0; k < D; k++) r.c[k] = 0;
    return r;
  }
  __host__ __device__ static inline E one() {
    E r = zero();
    r.c[0] = F::ONE;
    return r;
  }
  __host__ __device__ static inline E from_base(T x) {
    E r = zero();
    r.c[0] = x;
    return r;
  }
  __host__ __device__ static inline bool is_zero(const E& a) {
    T o = 0;
#pragma unroll
    for (int k = 0; k < D; k++) o |= a.c[k];
    return o == 0;
  }
  __host__ __device__ static inline E add(const E& a, const E& b) {
    E r;
#pragma unroll
    for (int k = 0; k < D; k++) r.c[k] = F::add(a.c[k], b.c[k]);
    return r;
  }
  __host__ __device__ static inline E sub(const E& a, const E& b) {
    E r;
#pragma unroll
    for (int k = 0; k < D; k++) r.c[k] = F::sub(a.c[k], b.c[k]);
    return r;
  }
  __host__ __device__ static inline E neg(const E& a) {
    E r;
#pragma unroll
    for (int k = 0; k < D; k++) r.c[k] = F::neg(a.c[k]);
    return r;
  }
  __host__ __device__ static inline E mul_base(const E& a, T s) {
    E r;
#pragma unroll
    for (int k = 0; k < D; k++) r.c[k] = F::mul(a.c[k], s);
    return r;
  }
  // x / 2 of a stored word: halving is linear, so it commutes with the Montgomery factor.  Odd words take (x + p) / 2 without
  // the sum leaving the word
  __host__ __device__ static inline T half(T x) { return (T)((x >> 1) + ((x & 1) ? HALF_UP : (T)0)); }
  __host__ __device__ static inline E halve(const E& a) {
    E r;
#pragma unroll
    for (int k = 0; k < D; k++) r.c[k] = half(a.c[k]);
    return r;
  }

  // ---- the quadratic level Fp[u] / (u^2 - W) on two words ----
  __host__ __device__ static inline void mul2(const T* a, const T* b, T* r) {
    const T v0 = F::mul(a[0], b[0]), v1 = F::mul(a[1], b[1]);
    const T x = F::add(F::mul(a[0], b[1]), F::mul(a[1], b[0]));
    r[0] = F::add(v0, F::mul(v1, W_MONT));
    r[1] = x;
  }
  __host__ __device__ static inline void mul2_by_u(const T* a, T* r) {   // (a0 + a1 u) u = W a1 + a0 u
    const T t = F::mul(a[1], W_MONT);
    r[1] = a[0];
    r[0] = t;
  }
  __host__ __device__ static inline void inv2(const T* a, T* r) {   // by the norm a0^2 - W a1^2: one base inversion, 0 -> 0
    const T nrm = F::sub(F::sqr(a[0]), F::mul(F::sqr(a[1]), W_MONT));
    const T ni = F::inv(nrm);
    r[0] = F::mul(a[0], ni);
    r[1] = F::neg(F::mul(a[1], ni));
  }

  __host__ __device__ static inline E mul(const E& a, const E& b) {
    E r;
    if constexpr (D == 2) {
      mul2(a.c, b.c, r.c);
    } else {
      // (c0 + c1 v)(d0 + d1 v) = c0 d0 + u c1 d1 + (c0 d1 + c1 d0) v
      T v0[2], v1[2], v1u[2], x0[2], x1[2];
      mul2(a.c, b.c, v0);
      mul2(a.c + 2, b.c + 2, v1);
      mul2_by_u(v1, v1u);
      mul2(a.c, b.c + 2, x0);
      mul2(a.c + 2, b.c, x1);
      r.c[0] = F::add(v0[0], v1u[0]);
      r.c[1] = F::add(v0[1], v1u[1]);
      r.c[2] = F::add(x0[0], x1[0]);
      r.c[3] = F::add(x0[1], x1[1]);
    }
    return r;
  }
  __host__ __device__ static inline E sqr(const E& a) { return mul(a, a); }
  // by the norm down the tower: one base inversion; zero maps to zero
  __host__ __device__ static inline E inv(const E& a) {
    E r;
    if constexpr (D == 2) {
      inv2(a.c, r.c);
    } else {
      // norm = c0^2 - u c1^2 in Fp2; a^-1 = (c0 - c1 v) / norm
      T s0[2], s1[2], s1u[2], nrm[2], ni[2], t[2];
      mul2(a.c, a.c, s0);
      mul2(a.c + 2, a.c + 2, s1);
      mul2_by_u(s1, s1u);
      nrm[0] = F::sub(s0[0], s1u[0]);
      nrm[1] = F::sub(s0[1], s1u[1]);
      inv2(nrm, ni);
      mul2(a.c, ni, r.c);
      mul2(a.c + 2, ni, t);
      r.c[2] = F::neg(t[0]);
      r.c[3] = F::neg(t[1]);
    }
    return r;
  }
  __host__ __device__ static inline E pow(E a, uint64_t e) {
    E r = one();
    for (; e; e >>= 1, a = sqr(a))
      if (e & 1) r = mul(r, a);
    return r;
  }
};

// What the fold needs besides the row: the roots zinv[e] = zeta^-e, e < 4, zeta = w^(n / 2^a) of order 2^a (entries behind
// 2^(a-1) are unused), as stored.
struct SfpFoldRoots { uint64_t zinv[4]; };

// The fold of one row at log-arity A: v[j] = f[i + j n / 2^A], t = (2 h w^i)^-1, beta the challenge.  A successive 2-folds in
// registers; level l pairs v[j] and v[j + 2^(A-1-l)], whose position in the level's layer is i + j n / 2^A, so its twiddle is
// t_l * zeta^-(j << l); the next level's t is 2 t^2 and its challenge beta^2.
//   g = (x + y) / 2 + beta (x - y) (2 h w^pos)^-1
template <class Cfg, int A>
__host__ __device__ inline typename SFpX<Cfg>::E sfpx_fold_row(typename SFpX<Cfg>::E* v, typename Cfg::T t, const SfpFoldRoots& roots,
                                                              typename SFpX<Cfg>::E beta) {
  using X = SFpX<Cfg>;
  using F = SFp<Cfg>;
  using T = typename Cfg::T;
#pragma unroll
  for (int l = 0; l < A; l++) {
    const int half = 1 << (A - 1 - l);
#pragma unroll
    for (int j = 0; j < half; j++) {
      const T tw = j == 0 ? t : F::mul(t, (T)roots.zinv[j << l]);
      const typename X::E s = X::add(v[j], v[j + half]);
      const typename X::E d = X::mul_base(X::sub(v[j], v[j + half]), tw);
      v[j] = X::add(X::halve(s), X::mul(beta, d));
    }
    if (l + 1 < A) {
      const T t2 = F::sqr(t);
      t = F::add(t2, t2);
      beta = X::sqr(beta);
    }
  }
  return v[0];
}

}  // namespace arkhip
