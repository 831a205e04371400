// One-word prime fields in Montgomery form: Goldilocks (u64, R = 2^64), BabyBear and KoalaBear (u32, R = 2^32) -- the
// reference's SmallFp<P> instances of test-curves/src/smallfp.rs.  An element in memory is the canonical residue x*R mod p in
// the field's own word; every function here takes and returns canonical words (< p), on the host and on the device alike, so the
// host entries of capi_sfp.hip and the kernels of sfp_fft.cuh run the same code.  DESIGN.md section 27.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace arkhip {

// ---- constants by the backend's rules (ff-macros/src/small_fp/montgomery_backend.rs), computed at compile time --------------
constexpr uint64_t sfp_mulmod(uint64_t a, uint64_t b, uint64_t p) { return (uint64_t)(((unsigned __int128)a * b) % p); }
constexpr uint64_t sfp_powmod(uint64_t a, uint64_t e, uint64_t p) {
  uint64_t r = 1 % p;
  for (; e; e >>= 1, a = sfp_mulmod(a, a, p))
    if (e & 1) r = sfp_mulmod(r, a, p);
  return r;
}
constexpr uint64_t sfp_r_mod_p(int k_bits, uint64_t p) { return (uint64_t)((((unsigned __int128)1) << k_bits) % p); }
constexpr uint32_t sfp_neg_inv32(uint32_t p) {   // -p^-1 mod 2^32 (p odd): Newton's iteration doubles the correct bits
  uint32_t x = p;                                // 3 bits: p * p = 1 mod 8
  for (int i = 0; i < 5; i++) x *= 2u - p * x;
  return 0u - x;
}
constexpr int sfp_two_adicity(uint64_t p) {
  int s = 0;
  for (uint64_t m = p - 1; !(m & 1); m >>= 1) s++;
  return s;
}

template <class T_, uint64_t P_, uint64_t GEN_>
struct SfpCfg {
  using T = T_;
  static constexpr uint64_t P = P_;
  static constexpr uint64_t GEN = GEN_;                                    // plain
  static constexpr int K_BITS = 8 * (int)sizeof(T_);                       // R = 2^K_BITS: 64, and 32 for BOTH 31-bit fields
  static constexpr uint64_t R1 = sfp_r_mod_p(K_BITS, P_);                  // one, as stored
  static constexpr uint64_t R2 = sfp_mulmod(R1, R1, P_);
  static constexpr int TWO_ADICITY = sfp_two_adicity(P_);
  static constexpr uint64_t ROOT_PLAIN = sfp_powmod(GEN_, (P_ - 1) >> TWO_ADICITY, P_);
  static constexpr uint64_t ROOT = sfp_mulmod(ROOT_PLAIN, R1, P_);         // TWO_ADIC_ROOT_OF_UNITY as stored
  static constexpr uint64_t GEN_MONT = sfp_mulmod(GEN_, R1, P_);
  static constexpr uint32_t NPRIME32 = sfp_neg_inv32((uint32_t)P_);        // the 32-bit fields' t * N'
};
using GOLDILOCKS = SfpCfg<uint64_t, 0xFFFFFFFF00000001ull, 7>;
using BABYBEAR = SfpCfg<uint32_t, 2013265921ull, 31>;
using KOALABEAR = SfpCfg<uint32_t, 2130706433ull, 3>;

template <class Cfg>
struct SFp {
  using T = typename Cfg::T;
  static constexpr T P = (T)Cfg::P;
  static constexpr T ONE = (T)Cfg::R1;
  static constexpr bool WIDE = sizeof(T) == 8;

  __host__ __device__ static inline T add(T a, T b) {
    T s = a + b;
    if constexpr (WIDE) {
      // no spare bit: the sum may leave 64 bits.  a, b < p, so a + b - p < p fits again
      if (s < a || s >= P) s -= P;
    } else {
      if (s >= P) s -= P;   // p < 2^31: no carry out of the word
    }
    return s;
  }
  __host__ __device__ static inline T sub(T a, T b) {
    T d = a - b;
    if (a < b) d += P;
    return d;
  }
  __host__ __device__ static inline T neg(T a) { return a ? (T)(P - a) : (T)0; }

  // a * b * R^-1 mod p, canonical
  __host__ __device__ static inline T mul(T a, T b) {
    if constexpr (WIDE) {
      // Goldilocks: p = 2^64 - 2^32 + 1, so p^-1 = 2^32 + 1 mod 2^64.  The reduction of eprint 2022/274 section 5.1 as the
      // reference has it: k = lo * p^-1 mod 2^64, l = the high word of k * p (t - k * p has a zero low word), result th - l mod p
#if defined(__HIP_DEVICE_COMPILE__)
      const uint64_t tl = a * b, th = __umul64hi(a, b);
#else
      const unsigned __int128 t = (unsigned __int128)a * b;
      const uint64_t tl = (uint64_t)t, th = (uint64_t)(t >> 64);
#endif
      const uint64_t k = tl + (tl << 32);
      const uint64_t of = k < tl ? 1u : 0u;
      const uint64_t l = k - (k >> 32) - of;
      uint64_t r = th - l;
      if (th < l) r -= 0xFFFFFFFFull;      // borrowed 2^64 = 2^32 - 1 mod p
      if (r >= P) r -= P;
      return r;
    } else {
      const uint64_t t = (uint64_t)a * b;                      // < p^2 < 2^62
      const uint32_t m = (uint32_t)t * Cfg::NPRIME32;          // t * N' mod R
      uint64_t r = (t + (uint64_t)m * P) >> 32;                // < 2p, no overflow: m * p < 2^63
      if (r >= P) r -= P;
      return (T)r;
    }
  }
  __host__ __device__ static inline T sqr(T a) { return mul(a, a); }
  __host__ __device__ static inline T pow(T a, uint64_t e) {
    T r = ONE;
    for (; e; e >>= 1, a = sqr(a))
      if (e & 1) r = mul(r, a);
    return r;
  }
  __host__ __device__ static inline T inv(T a) { return pow(a, Cfg::P - 2); }   // 0 -> 0
  // an integer of the word's range -> Montgomery form; values >= p are reduced first (SmallFpConfig::new)
  __host__ __device__ static inline T from_canonical(T x) {
    if constexpr (WIDE) {
      if (x >= P) x -= P;       // 2^64 < 2p
    } else {
      x %= P;
    }
    return mul(x, (T)Cfg::R2);
  }
  __host__ __device__ static inline T into_canonical(T a) { return mul(a, (T)1); }
};

// pointwise operations of the vector kernels (sfp_fft.cuh: sfp_vec_launch) and of SmallFieldOps::vec_op
enum { SFP_OP_ADD = 0, SFP_OP_SUB = 1, SFP_OP_MUL = 2, SFP_OP_NEG = 3, SFP_OP_SCALE = 4, SFP_OP_INVERSE = 5, SFP_OP_FROM_CANONICAL = 6,
       SFP_OP_INTO_CANONICAL = 7 };

}  // namespace arkhip
