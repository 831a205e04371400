// TEST HOOKS ONLY: the dispatcher and kernels behind lazytest_api.hpp (which see for the layout and THE TABLE of what is
// instantiated).  lazy_raw_apply is __host__ __device__: compiled for the device, FpL::mul / sqr / sop2 / sop4 are the asm
// column chains the MSM kernels run; compiled for the host (tests/lazy_raw_host.hip) they are the portable _c forms -- the same
// vector files go through both.  The kernels index memory by lane only.
#pragma once
#include "curves.cuh"
#include "fp28.cuh"
#include "lazyk.cuh"
#include "lazytest_api.hpp"
#include <type_traits>
#ifdef ARK_LAZYTEST_FFT
#include "fft.cuh"
#endif

namespace arkhip {
namespace lazytest {

#define ARK_LT_K(KV, EXPR) \
  case KV: {               \
    constexpr int K = KV;  \
    r = EXPR;              \
    break;                 \
  }

// one FpL / Fft29 op on one lane; false: (op, k, h) is not in THE TABLE
template <class P, bool FFT>
ARK_HD bool lazy_raw_apply(int op, int k, int h, const u32* in, u32* out) {
  typedef FpL<P> F;
  constexpr int LL = F::L;
  auto ld = [&](int j) {
    F x;
#pragma unroll
    for (int i = 0; i < LL; i++) x.l[i] = in[j * LL + i];
    return x;
  };
  F r = F::zero();
  u32 flag = 0;
  bool ok = true;
  switch (op) {
    case MUL: r = F::mul(ld(0), ld(1)); break;
    case SQR: r = F::sqr(ld(0)); break;
    case SOP2: r = F::sop2(ld(0), ld(1), ld(2), ld(3)); break;
    case SOP4: r = F::sop4(ld(0), ld(1), ld(2), ld(3), ld(4), ld(5), ld(6), ld(7)); break;
    case ADD_LAZY: r = F::add_lazy(ld(0), ld(1)); break;
    case SUB:
      switch (k) {
        ARK_LT_K(0, F::template sub<K>(ld(0), ld(1)))
        default: ok = false;
      }
      break;
    case SUB_SEMI:
      switch (k) {
        ARK_LT_K(2, F::template sub_semi<K>(ld(0), ld(1)))
        ARK_LT_K(3, F::template sub_semi<K>(ld(0), ld(1)))
        ARK_LT_K(6, F::template sub_semi<K>(ld(0), ld(1)))
        default: ok = false;
      }
      break;
    case SUB_SWEEP:
      switch (k) {
        ARK_LT_K(2, F::template sub_sweep<K>(ld(0), ld(1)))
        ARK_LT_K(3, F::template sub_sweep<K>(ld(0), ld(1)))
        ARK_LT_K(4, F::template sub_sweep<K>(ld(0), ld(1)))
        ARK_LT_K(6, F::template sub_sweep<K>(ld(0), ld(1)))
        ARK_LT_K(8, F::template sub_sweep<K>(ld(0), ld(1)))
        default: ok = false;
      }
      break;
    case SUB_OP:
      switch (k) {
        ARK_LT_K(2, F::template sub_op<K>(ld(0), ld(1)))
        ARK_LT_K(3, F::template sub_op<K>(ld(0), ld(1)))
        ARK_LT_K(6, F::template sub_op<K>(ld(0), ld(1)))
        default: ok = false;
      }
      break;
    case SUB_B_2C_NORM:
      switch (k) {
        ARK_LT_K(4, F::template sub_b_2c_norm<K>(ld(0), ld(1), ld(2)))
        default: ok = false;
      }
      break;
    case NEGSUB:
      switch (k) {
        ARK_LT_K(4, F::template negsub<K>(ld(0), ld(1)))
        default: ok = false;
      }
      break;
    case NEG:
      switch (k) {
        ARK_LT_K(2, F::template neg<K>(ld(0)))
        default: ok = false;
      }
      break;
    case NEG_SEMI:
      switch (k) {
        ARK_LT_K(2, F::template neg_semi<K>(ld(0)))
        default: ok = false;
      }
      break;
    case COND_NEG_SEMI:
      switch (k) {
        ARK_LT_K(2, F::template cond_neg_semi<K>(ld(0), in[LL] != 0u))
        default: ok = false;
      }
      break;
    case SHR_MOD:
      if (k == F::SH) r = ld(0).template shr_mod<F::SH>();
      else ok = false;
      break;
    case TO_CANONICAL_BITS: {
      const Fp<P> c = ld(0).to_canonical_bits();
#pragma unroll
      for (int i = 0; i < P::N; i++) r.l[i] = c.l[i];
      break;
    }
    case IS_ZERO_OR_P: flag = ld(0).is_zero_or_p() ? 1u : 0u; break;
    case IS_ZERO_MOD_P: flag = ld(0).is_zero_mod_p() ? 1u : 0u; break;
    case UNPACK32: r = F::unpack32(in); break;
    case UNPACK32_SHL: r = F::unpack32_shl(in); break;
    case PACK32: {
      u32 w[P::N];
      ld(0).pack32(w);
#pragma unroll
      for (int i = 0; i < P::N; i++) r.l[i] = w[i];
      break;
    }
    default:
#ifdef ARK_LAZYTEST_FFT
      if constexpr (FFT) {
        typedef Fft29<P> A;
        switch (op) {
          case FFT_DIF:
            if (k == 4 && h == 1) r = A::template dif<4, 1>(ld(0), ld(1));
            else if (k == 7 && h == 2) r = A::template dif<7, 2>(ld(0), ld(1));
            else if (k == 2 && h == 1) r = A::template dif<2, 1>(ld(0), ld(1));
            else ok = false;
            break;
          case FFT_REDUCE_SWEEP: r = A::reduce_sweep(ld(0)); break;
          case FFT_SWEEP: r = A::sweep(ld(0)); break;
          case FFT_CANON: r = A::canon(ld(0)); break;
          case FFT_COND_SUB_P: r = A::cond_sub_p(ld(0)); break;
          default: ok = false;
        }
        break;
      }
#endif
      ok = false;
  }
#pragma unroll
  for (int i = 0; i < LL; i++) out[i] = r.l[i];
  out[LL] = flag;
  return ok;
}

#ifndef ARK_LAZYTEST_HOST   // (the host program stops here: Fp2L and the kernels are device code)
// the Fp2L ops: this lane's component of every operand in its slots, the partner's fetched by DPP inside the op
template <class FL2>
ARK_DEV bool lazy_raw_apply_x2(int op, int k, int h, const u32* in, u32* out) {
  typedef FL2 F;
  typedef typename F::B B;
  constexpr int LL = F::L;
  auto ld = [&](int j) {
    F x;
#pragma unroll
    for (int i = 0; i < LL; i++) x.v.l[i] = in[j * LL + i];
    return x;
  };
  B r = B::zero();
  u32 flag = 0;
  bool ok = true;
#define ARK_LT_K2(KV, EXPR) ARK_LT_K(KV, (EXPR).v)
  switch (op) {
    case X2_MUL:
      switch (k) {
        ARK_LT_K2(2, F::template mul<K>(ld(0), ld(1)))
        ARK_LT_K2(4, F::template mul<K>(ld(0), ld(1)))
        ARK_LT_K2(6, F::template mul<K>(ld(0), ld(1)))
        ARK_LT_K2(8, F::template mul<K>(ld(0), ld(1)))
        ARK_LT_K2(10, F::template mul<K>(ld(0), ld(1)))
        default: ok = false;
      }
      break;
    case X2_SQR: {
      bool z = false;
      switch (k) {
        ARK_LT_K2(2, F::template sqr<K>(ld(0), &z))
        ARK_LT_K2(4, F::template sqr<K>(ld(0), &z))
        ARK_LT_K2(6, F::template sqr<K>(ld(0), &z))
        ARK_LT_K2(10, F::template sqr<K>(ld(0), &z))
        default: ok = false;
      }
      flag = z ? 1u : 0u;
      break;
    }
    case X2_MUL_SUB:
      if (k == 4 && h == 2) r = F::template mul_sub<4, 2>(ld(0), ld(1), ld(2), ld(3)).v;
      else ok = false;
      break;
    case X2_REDUCE_SMALL: r = F::reduce_small(ld(0)).v; break;
    case X2_TO_CANONICAL: {
      const typename F::M c = ld(0).to_canonical();
#pragma unroll
      for (int i = 0; i < F::P::N; i++) r.l[i] = c.v.l[i];
      break;
    }
    case X2_FROM_CANONICAL: {
      typename F::M m;
#pragma unroll
      for (int i = 0; i < F::P::N; i++) m.v.l[i] = in[i];
      r = F::from_canonical(m).v;
      break;
    }
    case X2_BETA_NEG:
      switch (k) {
        ARK_LT_K(2, F::template beta_neg<K>(ld(0).v))
        ARK_LT_K(4, F::template beta_neg<K>(ld(0).v))
        ARK_LT_K(6, F::template beta_neg<K>(ld(0).v))
        ARK_LT_K(8, F::template beta_neg<K>(ld(0).v))
        ARK_LT_K(10, F::template beta_neg<K>(ld(0).v))
        default: ok = false;
      }
      break;
    case X2_BOTH: flag = F::both(in[0] != 0u) ? 1u : 0u; break;
    case X2_SUB_SWEEP:
      switch (k) {
        ARK_LT_K2(2, F::template sub_sweep<K>(ld(0), ld(1)))
        ARK_LT_K2(4, F::template sub_sweep<K>(ld(0), ld(1)))
        ARK_LT_K2(8, F::template sub_sweep<K>(ld(0), ld(1)))
        default: ok = false;
      }
      break;
    case X2_SUB_B_2C_NORM:
      switch (k) {
        ARK_LT_K2(4, F::template sub_b_2c_norm<K>(ld(0), ld(1), ld(2)))
        default: ok = false;
      }
      break;
    default: ok = false;
  }
#undef ARK_LT_K2
#pragma unroll
  for (int i = 0; i < LL; i++) out[i] = r.l[i];
  out[LL] = flag;
  return ok;
}

// FL2 = void: a prime-field unit (FpL / Fft29 ops); otherwise a G2 unit (the Fp2L ops, n even: lanes retire in pairs)
template <class P, bool FFT, class FL2>
__global__ void __launch_bounds__(128) lazy_raw_op_kernel(int op, int k, int h, int arity, const u32* __restrict__ in,
                                                          u32* __restrict__ out, size_t n) {
  constexpr int LL = FpL<P>::L;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  u32 o[LL + 1];
  if constexpr (std::is_void<FL2>::value) lazy_raw_apply<P, FFT>(op, k, h, in + t * (size_t)arity * LL, o);
  else lazy_raw_apply_x2<FL2>(op, k, h, in + t * (size_t)arity * LL, o);
#pragma unroll
  for (int i = 0; i <= LL; i++) out[t * (LL + 1) + i] = o[i];
}

// -1: the op does not belong to this unit or its parameters are not in THE TABLE (nothing is launched)
template <class P, bool FFT, class FL2>
int lazy_raw_op_launch(int op, int k, int h, const void* in, void* out, size_t n, hipStream_t s) {
  const Row* row = row_of(op);
  if (!row || !params_ok(op, k, h)) return -1;
  constexpr bool X2 = !std::is_void<FL2>::value;
  if ((op >= X2_FIRST) != X2) return -1;
  if (op >= FFT_FIRST && op < X2_FIRST && !FFT) return -1;
  if (op == SHR_MOD && k != FpL<P>::SH) return -1;
  if (X2 && (n & 1)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL((lazy_raw_op_kernel<P, FFT, FL2>), dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, op, k, h,
                     row->arity, (const u32*)in, (u32*)out, n);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// accumulator ops through the parked layout (lazytest_api.hpp: AccKind); one lane (G2: one lane pair) per bucket
template <class C>
__global__ void __launch_bounds__(128) lazy_acc_op_kernel(int kind, const char* __restrict__ acc_in,
                                                          const char* __restrict__ other, char* __restrict__ out, size_t n) {
  typedef LazyK<C> K;
  typedef typename K::FM F;
  typedef XYZZ<F> Pt;
  constexpr size_t SLOT = (size_t)K::WORDS * 4;
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / K::LANES;
  if (i >= n) return;
  typename K::Acc acc;
  if (kind == ACC_FROM_BUCKET) acc = K::from_bucket(Pt::load(acc_in + i * Pt::BYTES));
  else acc = K::unpark(acc_in + i * SLOT);
  if (kind == ACC_MADD || kind == ACC_MSUB) {
    const char* src = other + i * Affine<F>::BYTES;
    const Affine<F> p = Affine<F>::load(src);
    if (!p.is_zero()) {
      if (K::madd(acc, p, kind == ACC_MSUB)) {
        typename K::Acc d;
        K::mdbl(d, src, kind == ACC_MSUB);
        acc = d;
      }
    }
  } else if (kind == ACC_MDBL || kind == ACC_MDBL_NEG) {
    K::mdbl(acc, other + i * Affine<F>::BYTES, kind == ACC_MDBL_NEG);
  } else if (kind == ACC_ADD) {
    K::add(acc, Pt::load(other + i * Pt::BYTES));
  } else if (kind == ACC_ADD_ACC) {
    K::add_acc(acc, K::unpark(other + i * SLOT));
  } else if (kind == ACC_DBL) {
    if (!acc.inf) {
      if constexpr (K::LANES == 1) xyzz_dbl_lazy<typename K::P>(acc);
      else lazy2_dbl<typename K::FL>(acc);
    }
  } else if (kind == ACC_TO_BUCKET) {
    K::to_bucket(acc).store(out + i * Pt::BYTES);
    return;
  }
  K::park(acc, out + i * SLOT);
}

template <class C>
int lazy_acc_op_launch(int kind, const void* acc, const void* other, void* out, size_t n, hipStream_t s) {
  if (kind < 0 || kind >= ACC_KINDS) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL((lazy_acc_op_kernel<C>), dim3((unsigned)((n * LazyK<C>::LANES + 127) / 128)), dim3(128), 0, s, kind,
                     (const char*)acc, (const char*)other, (char*)out, n);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
#endif  // ARK_LAZYTEST_HOST

}  // namespace lazytest
}  // namespace arkhip
