// TEST HOOKS ONLY: the dispatcher and kernels behind relaxtest_api.hpp (which see for the layout and THE TABLE of what is served).
// relaxed_raw_apply and relaxed_raw_apply_fp2 are __host__ __device__: compiled for the device, the products are the asm column
// chains the kernels run and return RELAXED limbs; compiled for the host (tests/relaxed_raw_host.hip) the ARK_HD limb functions
// are the same statements and the products return canonical values -- the same vector files go through both.  The kernels index
// memory by lane only.
#pragma once
#include "curves.cuh"
#include "relaxtest_api.hpp"
#include <type_traits>

namespace arkhip {
namespace relaxtest {

template <class P> struct FieldId;
template <> struct FieldId<BN254_FQ> { static constexpr int v = 0; };
template <> struct FieldId<BN254_FR> { static constexpr int v = 1; };
template <> struct FieldId<BLS12_381_FQ> { static constexpr int v = 2; };
template <> struct FieldId<BLS12_381_FR> { static constexpr int v = 3; };
template <> struct FieldId<BLS12_377_FQ> { static constexpr int v = 4; };
template <> struct FieldId<BLS12_377_FR> { static constexpr int v = 5; };

// 0 for a prime field (a G1 unit), NEG_BETA for the lane-pair field of a G2 unit
template <class F> struct NegBetaOf { static constexpr int v = 0; };
template <class P, int NEG_BETA> struct NegBetaOf<Fp2Half<P, NEG_BETA>> { static constexpr int v = NEG_BETA; };

#define ARK_RT_OP(OPV, EXPR)                         \
  case OPV:                                          \
    if constexpr (served(OPV, FID)) { EXPR; }        \
    else ok = false;                                 \
    break;

// one Fp op on one lane; false: the op is not served on this field
template <class P>
ARK_HD bool relaxed_raw_apply(int op, const u32* in, u32* out) {
  typedef Fp<P> F;
  constexpr int N = F::N;
  constexpr int FID = FieldId<P>::v;
  auto ld = [&](int j) {
    F x;
#pragma unroll
    for (int i = 0; i < N; i++) x.l[i] = in[j * N + i];
    return x;
  };
  F r = F::zero();
  u32 flag = 0;
  bool ok = true;
  switch (op) {
    ARK_RT_OP(MUL_R, r = F::mul_r(ld(0), ld(1)))
    ARK_RT_OP(SQR_R, r = F::sqr_r(ld(0)))
    ARK_RT_OP(MUL_R1, r = F::mul_r1(ld(0), ld(1)))
    ARK_RT_OP(MUL, r = F::mul(ld(0), ld(1)))
    ARK_RT_OP(ADD_R, r = F::add_r(ld(0), ld(1)))
    ARK_RT_OP(ADD_R2, r = F::add_r2(ld(0), ld(1)))
    ARK_RT_OP(DBL_R, r = F::dbl_r(ld(0)))
    ARK_RT_OP(SUB_R, r = F::sub_r(ld(0), ld(1)))
    ARK_RT_OP(NEG_R, r = F::neg_r(ld(0)))
    ARK_RT_OP(SOP2_R, r = F::sop2_r(ld(0), ld(1), ld(2), ld(3)))
    ARK_RT_OP(SOP2, r = F::sop2(ld(0), ld(1), ld(2), ld(3)))
    ARK_RT_OP(REDUCE_2P, r = F::reduce_2p(ld(0).l))
    ARK_RT_OP(IS_ZERO_MOD_P, flag = ld(0).is_zero_mod_p() ? 1u : 0u)
    ARK_RT_OP(CANONICAL, r = ld(0).canonical())
    ARK_RT_OP(REDUCE_FULL, r = F::reduce_full(ld(0)))
    default: ok = false;
  }
#pragma unroll
  for (int i = 0; i < N; i++) out[i] = r.l[i];
  out[N] = flag;
  return ok;
}

// one Fp2 op, whole on this lane: c0 of slot j at in0[j * N], c1 at in1[j * N]; writes component `comp` of the result
template <class P, int NEG_BETA>
ARK_HD bool relaxed_raw_apply_fp2(int op, const u32* in0, const u32* in1, int comp, u32* out) {
  typedef Fp2<P, NEG_BETA> F2;
  typedef Fp<P> B;
  constexpr int N = B::N;
  auto ld = [&](int j) {
    F2 x;
#pragma unroll
    for (int i = 0; i < N; i++) {
      x.c0.l[i] = in0[j * N + i];
      x.c1.l[i] = in1[j * N + i];
    }
    return x;
  };
  F2 r = F2::zero();
  bool ok = true;
  switch (op) {
    case F2_NEG_BETA_TIMES_NEG: {
      const F2 x = ld(0);
      r.c0 = F2::neg_beta_times_neg(x.c0);
      r.c1 = F2::neg_beta_times_neg(x.c1);
      break;
    }
    case F2_MUL: r = F2::mul(ld(0), ld(1)); break;
    case F2_SQR: r = F2::sqr(ld(0)); break;
    case F2_MUL_KARATSUBA: r = F2::mul_karatsuba(ld(0), ld(1)); break;
    default: ok = false;
  }
#pragma unroll
  for (int i = 0; i < N; i++) out[i] = comp ? r.c1.l[i] : r.c0.l[i];
  out[N] = 0;
  return ok;
}

// XYZZ in the memory layout of XYZZ<F>, raw limbs in and out (XYZZ::load / store copy bits)
template <class F>
ARK_HD void relaxed_acc_apply(int kind, const char* acc_in, const char* other, char* out) {
  XYZZ<F> acc = XYZZ<F>::load(acc_in);
  if (kind == ACC_MADD) {
    const Affine<F> p = Affine<F>::load(other);
    xyzz_madd_relaxed<F>(acc, p.x, p.y);
  } else if (kind == ACC_ADD) {
    xyzz_add_relaxed<F>(acc, XYZZ<F>::load(other));
  } else {
    acc = xyzz_canonical<F>(acc);
  }
  acc.store(out);
}

#ifndef ARK_RELAXTEST_HOST   // (the host program stops here: Fp2Half and the kernels are device code)
template <class H>
ARK_DEV void relaxed_raw_apply_half(int op, const u32* in, u32* out) {
  typedef typename H::B B;
  constexpr int N = H::N;
  auto ld = [&](int j) {
    H x;
#pragma unroll
    for (int i = 0; i < N; i++) x.v.l[i] = in[j * N + i];
    return x;
  };
  B r = B::zero();
  u32 flag = 0;
  switch (op) {
    case H_MUL_R: r = H::mul_r(ld(0), ld(1)).v; break;
    case H_SQR_R: r = H::sqr_r(ld(0)).v; break;
    case H_SOP2_R: r = H::sop2_r(ld(0), ld(1), ld(2), ld(3)).v; break;
    case H_BETA_TIMES: r = H::beta_times(ld(0).v); break;
    case H_NEG_R: r = H::neg_r(ld(0)).v; break;
    case H_IS_ZERO_MOD_P: flag = ld(0).is_zero_mod_p() ? 1u : 0u; break;
    case H_IS_ZERO: flag = ld(0).is_zero() ? 1u : 0u; break;
    case H_CANONICAL: r = ld(0).canonical().v; break;
    case H_MUL: r = H::mul(ld(0), ld(1)).v; break;
    case H_SQR: r = H::sqr(ld(0)).v; break;
    default: break;   // (the launcher lets only the ops above through)
  }
#pragma unroll
  for (int i = 0; i < N; i++) out[i] = r.l[i];
  out[N] = flag;
}

// NEG_BETA = 0: a prime-field unit (the Fp ops); otherwise a G2 unit (Fp2 and Fp2Half ops, n even: lanes retire in pairs)
template <class P, int NEG_BETA>
__global__ void __launch_bounds__(128) relaxed_raw_op_kernel(int op, int unit, int arity, const u32* __restrict__ in,
                                                             u32* __restrict__ out, size_t n) {
  constexpr int N = P::N;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  u32 o[N + 1];
  if constexpr (NEG_BETA == 0) {
    relaxed_raw_apply<P>(op, in + t * (size_t)arity * N, o);
  } else {
    if (unit == U_HALF) {
      relaxed_raw_apply_half<Fp2Half<P, NEG_BETA>>(op, in + t * (size_t)arity * N, o);
    } else {
      const size_t e = t & ~(size_t)1;
      relaxed_raw_apply_fp2<P, NEG_BETA>(op, in + e * (size_t)arity * N, in + (e + 1) * (size_t)arity * N, (int)(t & 1), o);
    }
  }
#pragma unroll
  for (int i = 0; i <= N; i++) out[t * (N + 1) + i] = o[i];
}

// -1: the op does not belong to this unit or is not served on its field (nothing is launched)
template <class P, int NEG_BETA>
int relaxed_raw_op_launch(int op, const void* in, void* out, size_t n, hipStream_t s) {
  const Row* row = row_of(op);
  if (!row || !served(op, FieldId<P>::v)) return -1;
  if ((row->unit == U_FP) != (NEG_BETA == 0)) return -1;
  if (NEG_BETA != 0 && (n & 1)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL((relaxed_raw_op_kernel<P, NEG_BETA>), dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, op, row->unit,
                     row->arity, (const u32*)in, (u32*)out, n);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// one lane (G2: one lane pair) per accumulator
template <class C>
__global__ void __launch_bounds__(128) relaxed_acc_op_kernel(int kind, const char* __restrict__ acc_in,
                                                             const char* __restrict__ other, char* __restrict__ out, size_t n) {
  typedef typename C::FA F;
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / F::LANES;
  if (i >= n) return;
  const size_t ob = kind == ACC_MADD ? Affine<F>::BYTES : kind == ACC_ADD ? XYZZ<F>::BYTES : 0;
  relaxed_acc_apply<F>(kind, acc_in + i * XYZZ<F>::BYTES, other + i * ob, out + i * XYZZ<F>::BYTES);
}

template <class C>
int relaxed_acc_op_launch(int kind, const void* acc, const void* other, void* out, size_t n, hipStream_t s) {
  if (kind < 0 || kind >= ACC_KINDS) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL((relaxed_acc_op_kernel<C>), dim3((unsigned)((n * C::FA::LANES + 127) / 128)), dim3(128), 0, s, kind,
                     (const char*)acc, (const char*)other, (char*)out, n);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
#endif  // ARK_RELAXTEST_HOST

}  // namespace relaxtest
}  // namespace arkhip
