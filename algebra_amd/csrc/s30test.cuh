// TEST HOOKS ONLY (libark_hip_test.so through testops_curve.hip; tests/lazy30_raw_host.hip): the raw-digit interface to the signed
// 30-bit arithmetic of fp30s.cuh and to the mixed addition of ec30s.cuh, beside lazytest.cuh's for the 28-bit forms.
//
// One call = one op on n lanes.  Lane t reads IN_WORDS(op) int32 words at in[t * IN_WORDS] and writes OUT_WORDS(op) words at
// out[t * OUT_WORDS].  A field element is a slot of 13 signed digits AS THE TEST CHOSE THEM (not canonical words); a canonical
// element takes the first 12 words of a slot.  s30_raw_apply is __host__ __device__: compiled for the device, mul / sqr / sop2 / mul_sub /
// sqr_sub2 are the v_mad_i64_i32 column chains the accumulate kernel runs; compiled for the host they are the portable _c forms, and
// the same vector files go through both.  The kernel indexes memory by lane only.
#pragma once
#include "curves.cuh"
#include "lazyk.cuh"
#include "s30test_api.hpp"

namespace arkhip {
namespace s30test {

template <class C>
ARK_HD void s30_raw_apply(int op, const i32* in, i32* out) {
  typedef LazySK<C> K;
  typedef typename K::FL F;
  typedef typename K::FM FM;
  static_assert(F::L == SLOT, "slot = 13 digits");
  auto ld = [&](int j) {
    F x;
#pragma unroll
    for (int i = 0; i < SLOT; i++) x.l[i] = in[j * SLOT + i];
    return x;
  };
  auto canon = [&](int at) {
    FM x;
#pragma unroll
    for (int i = 0; i < FM::N; i++) x.l[i] = (u32)in[at + i];
    return x;
  };
  F r = F::zero();
  switch (op) {
    case MUL: r = F::mul(ld(0), ld(1)); break;
    case SQR: r = F::sqr(ld(0)); break;
    case SOP2: r = F::sop2(ld(0), ld(1), ld(2), ld(3)); break;
    case SUB: r = F::sub(ld(0), ld(1)); break;
    case ADD_2B: r = F::add_2b(ld(0), ld(1)); break;
    case FROM_CANONICAL_SHL: r = F::from_canonical_shl(canon(0).l); break;
    case TO_CANONICAL: {
      const FM c = ld(0).to_canonical();
#pragma unroll
      for (int i = 0; i < FM::N; i++) r.l[i] = (i32)c.l[i];
      break;
    }
    case MADD: {
      typename K::Acc acc = K::unpark(in);
      F x2, y2;
      s30_from_affine<typename K::P>(canon(4 * SLOT + 1), canon(5 * SLOT + 1), x2, y2);
      const bool eq = xyzz_madd_s<typename K::P>(acc, x2, y2);
      K::park(acc, out);
      out[4 * SLOT + 1] = eq ? 1 : 0;
      return;
    }
    case FROM_CANONICAL_U: r = F::from_canonical_u(canon(0).l); break;
    case MADD_ENTRY: {
      typename K::Acc acc = K::unpark(in);
      Affine<FM> p;
      p.x = canon(4 * SLOT + 1);
      p.y = canon(5 * SLOT + 1);
      const bool eq = K::madd(acc, p, in[6 * SLOT + 1] != 0);
      K::park(acc, out);
      out[4 * SLOT + 1] = eq ? 1 : 0;
      return;
    }
    case ADD_FULL:
    case ADD_FULL_ACC: {
      auto pt = [&](int j) {
        XYZZ<FM> b;
        b.x = canon(j * SLOT);
        b.y = canon((j + 1) * SLOT);
        b.zz = canon((j + 2) * SLOT);
        b.zzz = canon((j + 3) * SLOT);
        return b;
      };
      typename K::Acc acc = K::inf();
      K::add(acc, pt(0));
      if (op == ADD_FULL) {
        K::add(acc, pt(4));
      } else {
        typename K::Acc other = K::inf();
        K::add(other, pt(4));
        K::add_acc(acc, other);
      }
      const XYZZ<FM> o = K::to_bucket(acc);
#pragma unroll
      for (int i = 0; i < SLOT; i++) {
        out[i] = i < FM::N ? (i32)o.x.l[i] : 0;
        out[SLOT + i] = i < FM::N ? (i32)o.y.l[i] : 0;
        out[2 * SLOT + i] = i < FM::N ? (i32)o.zz.l[i] : 0;
        out[3 * SLOT + i] = i < FM::N ? (i32)o.zzz.l[i] : 0;
      }
      return;
    }
    case MUL_SUB: r = F::mul_sub(ld(0), ld(1), ld(2)); break;
    case SQR_SUB2: r = F::sqr_sub2(ld(0), ld(1), ld(2)); break;
    default: break;
  }
#pragma unroll
  for (int i = 0; i < SLOT; i++) out[i] = r.l[i];
}

// is C a curve whose plain accumulate kernel has the signed form?
template <class C, int LN = C::FA::LANES> struct Served : std::false_type {};
template <class C> struct Served<C, 1> : HasS30<typename C::F::P> {};

#if defined(__HIPCC__)
template <class C>
__global__ void __launch_bounds__(128) s30_raw_op_kernel(int op, const i32* __restrict__ in, i32* __restrict__ out, size_t n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  s30_raw_apply<C>(op, in + t * (size_t)in_words(op), out + t * (size_t)out_words(op));
}
// -1: not an op, or a curve without the signed form
template <class C>
int s30_raw_op_launch(int op, const void* in, void* out, size_t n, hipStream_t s) {
  if constexpr (Served<C>::value) {
    if (op < 0 || op >= OPS) return -1;
    hipLaunchKernelGGL((s30_raw_op_kernel<C>), dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, op, (const i32*)in, (i32*)out, n);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
  } else {
    return -1;
  }
}
#endif

}  // namespace s30test
}  // namespace arkhip
