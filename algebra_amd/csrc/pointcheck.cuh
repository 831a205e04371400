// Base-set validation: is every point of an array a field-element pair, on the curve, and in the prime-order subgroup?
//
// Every MSM entry is correct only for bases in the prime-order subgroup (the digit fold s -> r - s relies on r P = O).  The
// reference establishes that at deserialisation with two predicates:
//   Affine::is_on_curve                                   ec/src/models/short_weierstrass/affine.rs:146-157
//   SWCurveConfig::is_in_correct_subgroup_assuming_on_curve   ec/src/models/short_weierstrass/mod.rs:82-90
//     default: double_and_add_affine(P, r).is_zero(); overrides: curves/bn254/src/curves/g1.rs:59 (cofactor one: true),
//     curves/bls12_381/src/curves/g1.rs:69-85 (endomorphism; Scott, eprint 2021/1130 section 6), g2.rs:75.
// sw_check_point is ONE host/device function: the kernel below, the host twin behind ark_hip_test_host_sw_check and a
// stand-alone host program all run the same code.
//
// status = the first stage that fails:
//   0  passed every requested stage
//   1  a coordinate is not a field element (some Fp component, read as an integer, is >= p).  The field arithmetic is
//      undefined for such limbs (its host and device forms may even disagree), so this stage runs under EVERY mask and
//      nothing further is computed for the point.
//   2  not on the curve: y^2 != x^3 + b.  The identity (0, 0) passes, as is_on_curve does for is_zero().
//   3  [r] P != O
// checks: bit 0 = stage 2, bit 1 = stage 3 (with bit 1 alone: "assuming on curve", as in the reference).
// method: 1 = double-and-add over the bits of r (every curve); 2 = phi(P) == -[x^2] P, BLS12-381 G1 only; 0 = auto.
#pragma once
#include "curves.cuh"
#include "check_consts.hpp"

namespace arkhip {

enum { SW_CHECK_ON_CURVE = 1, SW_CHECK_SUBGROUP = 2 };
enum { SW_STATUS_OK = 0, SW_STATUS_NOT_REDUCED = 1, SW_STATUS_OFF_CURVE = 2, SW_STATUS_OFF_SUBGROUP = 3 };
// What method 0 means on BLS12-381 G1: the endomorphism test, faster than the ladder over r in the same run
// (profiles/check_bases.json).  Every other curve has the ladder over r only.
#ifndef ARK_SW_CHECK_AUTO_ENDO
#define ARK_SW_CHECK_AUTO_ENDO 1
#endif

template <class C> struct CheckK;
template <> struct CheckK<BN254_G1> : CHECK_BN254_G1 {};
template <> struct CheckK<BLS12_381_G1> : CHECK_BLS12_381_G1 {};
template <> struct CheckK<BLS12_377_G1> : CHECK_BLS12_377_G1 {};
template <> struct CheckK<BLS12_377_G2> : CHECK_BLS12_377_G2 {};
template <> struct CheckK<BLS12_381_G2> : CHECK_BLS12_381_G2 {};

// a < p as integers (the limbs of a field element in memory)
template <class P>
ARK_HD bool fe_is_reduced(const Fp<P>& a) {
  u32 borrow = 0;
#pragma unroll
  for (int i = 0; i < P::N; i++) {
    u32 bo;
    (void)__builtin_subc(a.l[i], (u32)P::P[i], borrow, &bo);
    borrow = bo;
  }
  return borrow != 0;
}
template <class P, int NB>
ARK_HD bool fe_is_reduced(const Fp2<P, NB>& a) {
  const bool r0 = fe_is_reduced(a.c0), r1 = fe_is_reduced(a.c1);
  return r0 && r1;
}
// COEFF_B of the curve (check_consts.hpp: one row per Fp component)
template <class K, class P>
ARK_HD void load_coeff_b(Fp<P>& r) {
#pragma unroll
  for (int i = 0; i < P::N; i++) r.l[i] = K::B[0][i];
}
template <class K, class P, int NB>
ARK_HD void load_coeff_b(Fp2<P, NB>& r) {
#pragma unroll
  for (int i = 0; i < P::N; i++) {
    r.c0.l[i] = K::B[0][i];
    r.c1.l[i] = K::B[1][i];
  }
}

// y^2 == x^3 + b, the identity passes                                         affine.rs:146-157
template <class C>
ARK_HD bool sw_is_on_curve(const Affine<typename C::F>& p) {
  typedef typename C::F F;
  typedef CheckK<C> K;
  if (p.is_zero()) return true;
  F b;
  load_coeff_b<K>(b);
  return F::eq(F::sqr(p.y), F::add(F::mul(F::sqr(p.x), p.x), b));
}

// [r] P == O for a point that is not the identity, by the reference's default (mod.rs:82-90): left-to-right
// double-and-add on an XYZZ accumulator.  The scalar is a per-curve constant, so which iterations add is the same for
// every lane and the branch is wave-uniform; the loop stays rolled (one doubling, one mixed addition in the code).  The
// mixed addition keeps its equal / opposite / identity branches: for a point of small order the accumulator meets +-P
// in the middle of the ladder.  endo (BLS12-381 G1): the same loop over x^2, then phi(P) == -[x^2] P with
// phi(x, y) = (beta x, y):  acc.x == beta x zz,  acc.y == -y zzz,  acc != O.
template <class C>
ARK_HD bool sw_in_subgroup(const Affine<typename C::F>& p, bool endo) {
  typedef typename C::F F;
  typedef CheckK<C> K;
  if constexpr (K::COFACTOR_ONE) {
    return true;   // every curve point is in the subgroup (bn254 g1.rs:59)
  } else {
    int top = K::R_BITS;
    if constexpr (K::HAS_ENDO) {
      if (endo) top = K::X2_BITS;
    }
    XYZZ<F> acc{p.x, p.y, F::one(), F::one()};   // the top bit
#pragma unroll 1
    for (int i = top - 2; i >= 0; i--) {
      acc = xyzz_dbl<F>(acc);
      u32 w = K::R[i >> 5];
      if constexpr (K::HAS_ENDO) {
        if (endo) w = K::X2[i >> 5];
      }
      if ((w >> (i & 31)) & 1u) xyzz_madd<F>(acc, p.x, p.y);
    }
    if constexpr (K::HAS_ENDO) {
      if (endo) {
        if (acc.is_zero()) return false;   // phi(P) is not the identity
        F beta;
#pragma unroll
        for (int i = 0; i < F::N; i++) beta.l[i] = K::ENDO_BETA[i];
        const bool ex = F::eq(acc.x, F::mul(F::mul(beta, p.x), acc.zz));
        const bool ey = F::eq(acc.y, F::mul(F::neg(p.y), acc.zzz));
        return ex && ey;
      }
    }
    return acc.is_zero();
  }
}

template <class C>
ARK_HD u32 sw_check_point(const Affine<typename C::F>& p, int checks, int method) {
  typedef CheckK<C> K;
  const bool rx = fe_is_reduced(p.x), ry = fe_is_reduced(p.y);
  if (!(rx && ry)) return SW_STATUS_NOT_REDUCED;
  if ((checks & SW_CHECK_ON_CURVE) && !sw_is_on_curve<C>(p)) return SW_STATUS_OFF_CURVE;
  if ((checks & SW_CHECK_SUBGROUP) && !p.is_zero()) {
    const bool endo = K::HAS_ENDO && (method == 2 || (method == 0 && ARK_SW_CHECK_AUTO_ENDO));
    if (!sw_in_subgroup<C>(p, endo)) return SW_STATUS_OFF_SUBGROUP;
  }
  return SW_STATUS_OK;
}

// One lane per point.  status (may be null): one byte per point.  out: four 64-bit words the caller initialises to
// {all ones, 0, 0, 0}: out[0] = smallest index (base + i) with a non-zero status, out[1..3] = points with status 1, 2, 3.
// Counts and the first bad lane are reduced in LDS; a workgroup that found something issues one atomic per non-zero word.
template <class C>
__global__ void __launch_bounds__(128) sw_check_kernel(const char* __restrict__ in, size_t n, size_t base, int checks, int method,
                                                       unsigned char* __restrict__ status, unsigned long long* out) {
  typedef typename C::F F;
  __shared__ u32 s_cnt[3];
  __shared__ u32 s_first;
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 3) s_first = 0xffffffffu;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  u32 st = SW_STATUS_OK;
  if (i < n) {
    st = sw_check_point<C>(Affine<F>::load(in + i * Affine<F>::BYTES), checks, method);
    if (status) status[i] = (unsigned char)st;
  }
  if (st != SW_STATUS_OK) {
    atomicAdd(&s_cnt[st - 1], 1u);
    atomicMin(&s_first, threadIdx.x);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const u32 c = s_cnt[threadIdx.x];
    if (c) atomicAdd(&out[1 + threadIdx.x], (unsigned long long)c);
  }
  if (threadIdx.x == 3 && s_first != 0xffffffffu)
    atomicMin(&out[0], (unsigned long long)(base + (size_t)blockIdx.x * blockDim.x + s_first));
}

template <class C>
int sw_check_launch(const void* d_in, size_t n, size_t base, int checks, int method, void* d_status, void* d_out, hipStream_t s) {
  if (n == 0) return 0;
  const size_t blocks = (n + 127) / 128;
  if (blocks > 0x7fffffffull) return -2;   // ARK_HIP_ERR_SIZE
  hipLaunchKernelGGL((sw_check_kernel<C>), dim3((unsigned)blocks), dim3(128), 0, s, (const char*)d_in, n, base, checks, method,
                     (unsigned char*)d_status, (unsigned long long*)d_out);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// the host twin: sw_check_point on the calling thread, no device involved
template <class C>
void sw_check_host(const uint64_t* xy, size_t n, int checks, int method, unsigned char* status) {
  typedef typename C::F F;
  for (size_t i = 0; i < n; i++)
    status[i] = (unsigned char)sw_check_point<C>(Affine<F>::load((const char*)xy + i * Affine<F>::BYTES), checks, method);
}

}  // namespace arkhip
