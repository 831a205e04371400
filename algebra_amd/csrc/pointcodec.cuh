// Compressed affine points: decompress (+ validate) and compress, where the points live.
//
// What the reference does when it reads a point with Compress::Yes (ec/src/models/short_weierstrass/mod.rs:149-193 with
// Affine::get_ys_from_x_unchecked, affine.rs:129-143; BLS12-381: curves/bls12_381/src/curves/util.rs, g1.rs:97-113, g2.rs:124-140)
// and when it writes one (mod.rs:125-146, g1.rs:115-147).  sw_decompress_point / sw_compress_point are ONE host/device function
// each: the kernels below, the host twins behind ark_hip_test_host_sw_{de,}compress and a stand-alone host program run the same code.
//
// Encodings (E bytes per point; "larger" = y > -y on canonical residues, Fp2: c1 decides, c0 if c1 = 0):
//   arkworks (BN254 G1 32, BLS12-377 G1 48, G2 96): x little-endian (Fp2: c0 | c1), bit 7 of the last byte = larger, bit 6 =
//     infinity.  Both set: refused.  Every component < p after the two bits are cleared -- also with the infinity bit, and then
//     the result is the identity whatever x is.
//   zcash (BLS12-381 G1 48, G2 96): x big-endian (Fp2: c1 | c0), byte 0: bit 7 = compressed (must be set), bit 6 = infinity,
//     bit 5 = larger.  Infinity with larger: refused; infinity with any other bit of the E bytes set: refused.
//   In both forms the flags sit in the top bits of the top limb of the c1 (or only) component.
// status = the first stage that fails:
//   0 ok   1 flags refused / malformed   2 a component is not a field element   3 x^3 + b has no square root
//   4 [r]P != O (only with validate)
// A point with a non-zero status is written as the identity (0, 0).
//
// Square roots.  Fp, p = 3 mod 4 (BN254, BLS12-381): w = a^((p-3)/4), root = w a, accepted iff root^2 = a; then 1/root = w, and for a
// non-residue root^2 = -a and w root = -1 (both used by the Fp2 root).  BLS12-377 Fq (p - 1 = 2^46 q): Tonelli-Shanks with fixed
// trip counts (RFC 9380 appendix I.4): z = a^((q-1)/2), t = z^2 a, r = z a, then for i = 46 .. 2: b = t^(2^(i-2)); if b != 1:
// r *= c, t *= c^2; c = c^2.  The inner trip count depends on i alone, the conditional step is a select: every lane of a wave
// runs the same 1590 products, whatever the input; no table, no per-lane array.  A non-residue ends in r^2 != a.
// Products per root: codec_consts.hpp SQRT_<field>::PRODUCTS (361 / 607 / 1590).
// Fp2: the reference's complex method (quadratic_extension.rs:368-426): alpha = sqrt(c0^2 - beta c1^2), delta = (c0 + alpha) / 2,
// or delta - alpha if that is no square; root = (sqrt(delta), c1 / (2 sqrt(delta))).  Over BLS12-381 (beta = -1, p = 3 mod 4) the
// failed attempt on delta already gives the answer: with x^2 = -delta and w x = -1, root = (-c1 w / 2, x) -- two exponentiations
// per root, always.  Over BLS12-377: up to three roots and one inversion.  c1 = 0: (sqrt(c0), 0), or (0, sqrt(c0 / beta)).
// Every Fp2 root is accepted only if its square is the argument.
#pragma once
#include "pointcheck.cuh"
#include "codec_consts.hpp"

namespace arkhip {

enum { SW_DEC_OK = 0, SW_DEC_FLAGS = 1, SW_DEC_NOT_REDUCED = 2, SW_DEC_NO_ROOT = 3, SW_DEC_OFF_SUBGROUP = 4 };

template <class P> struct SqrtK;
template <> struct SqrtK<BN254_FQ> : SQRT_BN254_FQ {};
template <> struct SqrtK<BLS12_381_FQ> : SQRT_BLS12_381_FQ {};
template <> struct SqrtK<BLS12_377_FQ> : SQRT_BLS12_377_FQ {};
template <class C> struct CodecK;
template <> struct CodecK<BN254_G1> : CODEC_BN254_G1 {};
template <> struct CodecK<BLS12_381_G1> : CODEC_BLS12_381_G1 {};
template <> struct CodecK<BLS12_377_G1> : CODEC_BLS12_377_G1 {};
template <> struct CodecK<BLS12_377_G2> : CODEC_BLS12_377_G2 {};
template <> struct CodecK<BLS12_381_G2> : CODEC_BLS12_381_G2 {};

// CALL: the out-of-line product (Fp2 kernels: the chains below would otherwise inline a dozen copies of it)
template <class P, bool CALL>
ARK_HD Fp<P> cd_mul(const Fp<P>& a, const Fp<P>& b) {
  if constexpr (CALL) return Fp<P>::mul_call(a, b);
  else return Fp<P>::mul(a, b);
}
template <class P>
ARK_HD Fp<P> cd_sel(bool c, const Fp<P>& a, const Fp<P>& b) {
  Fp<P> r;
#pragma unroll
  for (int i = 0; i < P::N; i++) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}
template <class P>
ARK_HD Fp<P> cd_const(const u32* k) {
  Fp<P> r;
#pragma unroll
  for (int i = 0; i < P::N; i++) r.l[i] = k[i];
  return r;
}
// a^e for a per-field constant e of `bits` bits (top bit set): the square / multiply branch is the same for every lane, the loop
// stays rolled
template <class P, bool CALL>
ARK_HD Fp<P> cd_pow(const Fp<P>& a, const u32* e, int bits) {
  Fp<P> r = a;
#pragma unroll 1
  for (int i = bits - 2; i >= 0; i--) {
    r = cd_mul<P, CALL>(r, r);
    if ((e[i >> 5] >> (i & 31)) & 1u) r = cd_mul<P, CALL>(r, a);
  }
  return r;
}
template <class P, bool CALL>
ARK_HD Fp<P> cd_inv(const Fp<P>& a) {   // a^(p-2)
  return cd_pow<P, CALL>(a, SqrtK<P>::PM2, P::BITS);
}

// root^2 == a?  root is written either way.  P3MOD4: w = a^((p-3)/4) is written too (1 / root for a residue; for a non-residue
// root^2 = -a and w root = -1).
template <class P, bool CALL>
ARK_HD bool fp_sqrt(const Fp<P>& a, Fp<P>& root, Fp<P>& w) {
  typedef SqrtK<P> K;
  typedef Fp<P> B;
  if constexpr (K::P3MOD4) {
    w = cd_pow<P, CALL>(a, K::E, K::E_BITS);
    root = cd_mul<P, CALL>(w, a);
  } else {
    const B z = cd_pow<P, CALL>(a, K::E, K::E_BITS);   // a^((q-1)/2)
    B t = cd_mul<P, CALL>(cd_mul<P, CALL>(z, z), a);   // a^q: its order divides 2^(S-1) iff a is a square
    B r = cd_mul<P, CALL>(z, a);                       // a^((q+1)/2): r^2 = t a
    B c = cd_const<P>(K::ROOT);
    const B one = B::one();
#pragma unroll 1
    for (int i = K::S; i >= 2; i--) {
      B b = t;
#pragma unroll 1
      for (int j = 0; j < i - 2; j++) b = cd_mul<P, CALL>(b, b);
      const bool e = B::eq(b, one);
      const B rc = cd_mul<P, CALL>(r, c);
      c = cd_mul<P, CALL>(c, c);
      const B tc = cd_mul<P, CALL>(t, c);
      r = cd_sel(e, r, rc);
      t = cd_sel(e, t, tc);
    }
    root = r;
    w = r;
  }
  return B::eq(cd_mul<P, CALL>(root, root), a);
}

// the square root in the curve's coordinate field; false: none (root is then unspecified)
template <class P>
ARK_HD bool coord_sqrt(const Fp<P>& a, Fp<P>& root) {
  Fp<P> w;
  return fp_sqrt<P, false>(a, root, w);
}
template <class P, int NB>
ARK_HD bool coord_sqrt(const Fp2<P, NB>& a, Fp2<P, NB>& root) {
  typedef Fp<P> B;
  typedef SqrtK<P> K;
  constexpr bool SHORT = K::P3MOD4 && NB == 1;   // beta = -1, p = 3 mod 4: a failed attempt is the root of the negated argument
  const B two_inv = cd_const<P>(K::TWO_INV);
  B r, w;
  if (a.c1.is_zero()) {
    if (fp_sqrt<P, true>(a.c0, r, w)) {
      root = Fp2<P, NB>{r, B::zero()};
      return true;
    }
    // c0 is no square in Fp: c0 / beta is one (beta is none either), and (s u)^2 = beta s^2
    if constexpr (!SHORT) {
      static_assert(NB == 5, "1 / beta is generated for BLS12-377 Fq2 only");
      if (!fp_sqrt<P, true>(B::mul_call(a.c0, cd_const<P>(CODEC_BLS12_377_G2::INV_BETA)), r, w)) return false;
    }
    root = Fp2<P, NB>{B::zero(), r};
    return true;
  }
  const B norm = B::add(B::mul_call(a.c0, a.c0), Fp2<P, NB>::mul_neg_beta(B::mul_call(a.c1, a.c1)));   // c0^2 - beta c1^2
  B alpha;
  if (!fp_sqrt<P, true>(norm, alpha, w)) return false;
  B delta = B::mul_call(B::add(alpha, a.c0), two_inv);
  B x0, x1;
  if (fp_sqrt<P, true>(delta, x0, w)) {
    if constexpr (!K::P3MOD4) w = cd_inv<P, true>(x0);
    x1 = B::mul_call(B::mul_call(a.c1, w), two_inv);   // c1 / (2 x0); x0 != 0 because c1 != 0
  } else if constexpr (SHORT) {
    x1 = x0;                                           // x0^2 = -delta, w x0 = -1
    x0 = B::neg(B::mul_call(B::mul_call(a.c1, w), two_inv));
  } else {
    delta = B::sub(delta, alpha);
    if (!fp_sqrt<P, true>(delta, x0, w)) return false;
    if constexpr (!K::P3MOD4) w = cd_inv<P, true>(x0);
    x1 = B::mul_call(B::mul_call(a.c1, w), two_inv);
  }
  root = Fp2<P, NB>{x0, x1};
  return Fp2<P, NB>::eq(Fp2<P, NB>::sqr(root), a);
}

// y > -y for a Montgomery-form y: the deciding component, as an integer, is above (p - 1) / 2
template <class P>
ARK_HD bool fp_above_half(const Fp<P>& mont) {
  const Fp<P> v = Fp<P>::from_mont(mont);
  u32 borrow = 0;
#pragma unroll
  for (int i = 0; i < P::N; i++) {
    u32 bo;
    (void)__builtin_subc((u32)SqrtK<P>::HALF_P[i], v.l[i], borrow, &bo);
    borrow = bo;
  }
  return borrow != 0;
}
template <class P>
ARK_HD bool fe_is_larger(const Fp<P>& y) { return fp_above_half(y); }
template <class P, int NB>
ARK_HD bool fe_is_larger(const Fp2<P, NB>& y) {   // quadratic_extension.rs:443-453: c1 first, then c0
  return fp_above_half(cd_sel(y.c1.is_zero(), y.c0, y.c1));
}
template <class P>
ARK_HD Fp<P> fe_to_mont(const Fp<P>& a) { return Fp<P>::to_mont(a); }
template <class P, int NB>
ARK_HD Fp2<P, NB> fe_to_mont(const Fp2<P, NB>& a) { return Fp2<P, NB>{Fp<P>::to_mont(a.c0), Fp<P>::to_mont(a.c1)}; }
template <class P>
ARK_HD Fp<P> fe_from_mont(const Fp<P>& a) { return Fp<P>::from_mont(a); }
template <class P, int NB>
ARK_HD Fp2<P, NB> fe_from_mont(const Fp2<P, NB>& a) { return Fp2<P, NB>{Fp<P>::from_mont(a.c0), Fp<P>::from_mont(a.c1)}; }

// ---- bytes <-> integer limbs.  Device pointers are 4-byte aligned (checked at the entry); host pointers are not assumed to be.
ARK_HD u32 cd_ld32(const unsigned char* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const u32*)p;
#else
  u32 v;
  __builtin_memcpy(&v, p, 4);
  return v;
#endif
}
ARK_HD void cd_st32(unsigned char* p, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  *(u32*)p = v;
#else
  __builtin_memcpy(p, &v, 4);
#endif
}
// one Fp component of 4 N bytes: little-endian (arkworks) or big-endian (zcash)
template <class P, bool BE>
ARK_HD Fp<P> cd_load_fp(const unsigned char* p) {
  Fp<P> r;
#pragma unroll
  for (int i = 0; i < P::N; i++) r.l[i] = BE ? __builtin_bswap32(cd_ld32(p + 4 * (P::N - 1 - i))) : cd_ld32(p + 4 * i);
  return r;
}
template <class P, bool BE>
ARK_HD void cd_store_fp(unsigned char* p, const Fp<P>& a) {
#pragma unroll
  for (int i = 0; i < P::N; i++) {
    if constexpr (BE) cd_st32(p + 4 * (P::N - 1 - i), __builtin_bswap32(a.l[i]));
    else cd_st32(p + 4 * i, a.l[i]);
  }
}
// the whole x: Fp2 is c0 | c1 (arkworks) or c1 | c0 (zcash).  top(): the limb that carries the flags.
template <bool BE, class P>
ARK_HD void cd_load_x(const unsigned char* p, Fp<P>& x) { x = cd_load_fp<P, BE>(p); }
template <bool BE, class P, int NB>
ARK_HD void cd_load_x(const unsigned char* p, Fp2<P, NB>& x) {
  x.c0 = cd_load_fp<P, BE>(p + (BE ? 4 * P::N : 0));
  x.c1 = cd_load_fp<P, BE>(p + (BE ? 0 : 4 * P::N));
}
template <bool BE, class P>
ARK_HD void cd_store_x(unsigned char* p, const Fp<P>& x) { cd_store_fp<P, BE>(p, x); }
template <bool BE, class P, int NB>
ARK_HD void cd_store_x(unsigned char* p, const Fp2<P, NB>& x) {
  cd_store_fp<P, BE>(p + (BE ? 4 * P::N : 0), x.c0);
  cd_store_fp<P, BE>(p + (BE ? 0 : 4 * P::N), x.c1);
}
template <class P>
ARK_HD u32& cd_top(Fp<P>& x) { return x.l[P::N - 1]; }
template <class P, int NB>
ARK_HD u32& cd_top(Fp2<P, NB>& x) { return x.c1.l[P::N - 1]; }

template <class C>
ARK_HD u32 sw_decompress_point(const unsigned char* bytes, int validate, int method, Affine<typename C::F>& out) {
  typedef typename C::F F;
  typedef CodecK<C> K;
  out.x = F::zero();
  out.y = F::zero();
  F x;
  cd_load_x<K::ZCASH>(bytes, x);
  u32& top = cd_top(x);
  const u32 flags = top;
  bool larger, infinity;
  if constexpr (K::ZCASH) {
    top &= 0x1fffffffu;
    larger = (flags >> 29) & 1u;
    infinity = (flags >> 30) & 1u;
    if (!(flags >> 31)) return SW_DEC_FLAGS;                       // util.rs:103-137: the compressed form only
    if (infinity && (larger || !x.is_zero())) return SW_DEC_FLAGS;
  } else {
    top &= 0x3fffffffu;
    larger = (flags >> 31) & 1u;
    infinity = (flags >> 30) & 1u;
    if (larger && infinity) return SW_DEC_FLAGS;                   // serialization_flags.rs:55-80
  }
  if (!fe_is_reduced(x)) return SW_DEC_NOT_REDUCED;
  if (infinity) return SW_DEC_OK;
  const F xm = fe_to_mont(x);
  F b;
  load_coeff_b<CheckK<C>>(b);
  const F rhs = F::add(F::mul(F::sqr(xm), xm), b);
  F y;
  if (!coord_sqrt(rhs, y)) return SW_DEC_NO_ROOT;
  if (fe_is_larger(y) != larger) y = F::neg(y);
  Affine<F> p;
  p.x = xm;
  p.y = y;
  if (validate) {
    const bool endo = CheckK<C>::HAS_ENDO && (method == 2 || (method == 0 && ARK_SW_CHECK_AUTO_ENDO));
    if (!sw_in_subgroup<C>(p, endo)) return SW_DEC_OFF_SUBGROUP;
  }
  out = p;
  return SW_DEC_OK;
}

// the canonical encoding of a point whose coordinates are reduced field elements (what check_bases establishes)
template <class C>
ARK_HD void sw_compress_point(const Affine<typename C::F>& p, unsigned char* bytes) {
  typedef typename C::F F;
  typedef CodecK<C> K;
  F x = F::zero();
  u32 flags = K::ZCASH ? 0x80000000u : 0u;
  if (p.is_zero()) {
    flags |= 0x40000000u;
  } else {
    x = fe_from_mont(p.x);
    if (fe_is_larger(p.y)) flags |= K::ZCASH ? 0x20000000u : 0x80000000u;
  }
  cd_top(x) |= flags;
  cd_store_x<K::ZCASH>(bytes, x);
}

// One lane per point.  points: n Affine (x | y, Montgomery form).  status (may be null): one byte per point.  out: five 64-bit
// words the caller initialises to {all ones, 0, 0, 0, 0}: out[0] = smallest index (base + i) with a non-zero status,
// out[1..4] = points with status 1..4.  Counts and the first bad lane are reduced in LDS; a workgroup that found something
// issues one atomic per non-zero word.
template <class C>
__global__ void __launch_bounds__(128) sw_decompress_kernel(const unsigned char* __restrict__ in, size_t n, size_t base, int validate,
                                                            int method, char* __restrict__ points,
                                                            unsigned char* __restrict__ status, unsigned long long* out) {
  typedef typename C::F F;
  __shared__ u32 s_cnt[4];
  __shared__ u32 s_first;
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 4) s_first = 0xffffffffu;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  u32 st = SW_DEC_OK;
  if (i < n) {
    Affine<F> p;
    st = sw_decompress_point<C>(in + i * CodecK<C>::E, validate, method, p);
    p.x.store(points + i * Affine<F>::BYTES);
    p.y.store(points + i * Affine<F>::BYTES + F::FULL_BYTES);
    if (status) status[i] = (unsigned char)st;
  }
  if (st != SW_DEC_OK) {
    atomicAdd(&s_cnt[st - 1], 1u);
    atomicMin(&s_first, threadIdx.x);
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const u32 c = s_cnt[threadIdx.x];
    if (c) atomicAdd(&out[1 + threadIdx.x], (unsigned long long)c);
  }
  if (threadIdx.x == 4 && s_first != 0xffffffffu)
    atomicMin(&out[0], (unsigned long long)(base + (size_t)blockIdx.x * blockDim.x + s_first));
}

template <class C>
__global__ void __launch_bounds__(128) sw_compress_kernel(const char* __restrict__ points, size_t n, unsigned char* __restrict__ bytes) {
  typedef typename C::F F;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) sw_compress_point<C>(Affine<F>::load(points + i * Affine<F>::BYTES), bytes + i * CodecK<C>::E);
}

template <class C>
int sw_decompress_launch(const void* d_bytes, size_t n, size_t base, int validate, int method, void* d_points, void* d_status,
                         void* d_out, hipStream_t s) {
  if (n == 0) return 0;
  const size_t blocks = (n + 127) / 128;
  if (blocks > 0x7fffffffull) return -2;   // ARK_HIP_ERR_SIZE
  hipLaunchKernelGGL((sw_decompress_kernel<C>), dim3((unsigned)blocks), dim3(128), 0, s, (const unsigned char*)d_bytes, n, base, validate,
                     method, (char*)d_points, (unsigned char*)d_status, (unsigned long long*)d_out);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
template <class C>
int sw_compress_launch(const void* d_points, size_t n, void* d_bytes, hipStream_t s) {
  if (n == 0) return 0;
  const size_t blocks = (n + 127) / 128;
  if (blocks > 0x7fffffffull) return -2;
  hipLaunchKernelGGL((sw_compress_kernel<C>), dim3((unsigned)blocks), dim3(128), 0, s, (const char*)d_points, n, (unsigned char*)d_bytes);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// the host twins: the per-point functions on the calling thread, no device involved
template <class C>
void sw_decompress_host(const unsigned char* bytes, size_t n, int validate, int method, uint64_t* xy, unsigned char* status) {
  typedef typename C::F F;
  for (size_t i = 0; i < n; i++) {
    Affine<F> p;
    const u32 st = sw_decompress_point<C>(bytes + i * CodecK<C>::E, validate, method, p);
    p.x.store((char*)xy + i * Affine<F>::BYTES);
    p.y.store((char*)xy + i * Affine<F>::BYTES + F::FULL_BYTES);
    if (status) status[i] = (unsigned char)st;
  }
}
template <class C>
void sw_compress_host(const uint64_t* xy, size_t n, unsigned char* bytes) {
  typedef typename C::F F;
  for (size_t i = 0; i < n; i++) sw_compress_point<C>(Affine<F>::load((const char*)xy + i * Affine<F>::BYTES), bytes + i * CodecK<C>::E);
}

// ---- test hook: the square root in the coordinate field, out = the root with r <= -r, or zero with ok = 0 ----
template <class F>
ARK_HD u32 coord_sqrt_smaller(const F& a, F& out) {
  F r;
  if (!coord_sqrt(a, r)) {
    out = F::zero();
    return 0;
  }
  out = fe_is_larger(r) ? F::neg(r) : r;
  return 1;
}
template <class C>
__global__ void __launch_bounds__(128) coord_sqrt_kernel(const char* __restrict__ in, char* __restrict__ out, unsigned char* __restrict__ ok,
                                                         size_t n) {
  typedef typename C::F F;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    F r;
    ok[i] = (unsigned char)coord_sqrt_smaller(F::load(in + i * F::FULL_BYTES), r);
    r.store(out + i * F::FULL_BYTES);
  }
}
template <class C>
int coord_sqrt_launch(const void* d_in, void* d_out, void* d_ok, size_t n, hipStream_t s) {
  if (n == 0) return 0;
  const size_t blocks = (n + 127) / 128;
  if (blocks > 0x7fffffffull) return -2;
  hipLaunchKernelGGL((coord_sqrt_kernel<C>), dim3((unsigned)blocks), dim3(128), 0, s, (const char*)d_in, (char*)d_out, (unsigned char*)d_ok, n);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}
template <class C>
void coord_sqrt_host(const uint64_t* in, uint64_t* out, unsigned char* ok, size_t n) {
  typedef typename C::F F;
  for (size_t i = 0; i < n; i++) {
    F r;
    ok[i] = (unsigned char)coord_sqrt_smaller(F::load((const char*)in + i * F::FULL_BYTES), r);
    r.store((char*)out + i * F::FULL_BYTES);
  }
}

}  // namespace arkhip
