// The Fiat-Shamir transcript of the device sumcheck, written once for host and device: plain C++, no
// inline assembly of its own.  The state is 32 bytes.  One operation, challenge(e_0 .. e_{k-1}), k >= 0:
//   msg   = state | u32_le(k) | le32(e_0) | .. | le32(e_{k-1})     (le32: the canonical value, out of Montgomery form)
//   out   = SHAKE256(msg, 96 bytes)
//   state = out[0:32]
//   c     = int_le(out[32:96]) mod r                               (returned in Montgomery form)
// Every piece of msg is a whole number of 32-bit words, so the sponge absorbs a WORD array: TRANSCRIPT_HEAD_WORDS + 8 k words
// that the caller lays out (transcript_put_element writes one element's eight).  The sponge addresses its 25 lanes with
// compile-time indices only -- the permutation is unrolled per round, the round loop is rolled -- so on the device the state
// can live in registers; the message is read from wherever the caller keeps it (LDS in the kernels of sumcheck.cuh).
#pragma once
#include "fp.cuh"

namespace arkhip {

constexpr int TRANSCRIPT_STATE_WORDS = 8;
constexpr int TRANSCRIPT_HEAD_WORDS = TRANSCRIPT_STATE_WORDS + 1;   // state | count
constexpr int TRANSCRIPT_RATE_WORDS = 34;                           // SHAKE256: 136 bytes
constexpr u32 transcript_words(u32 count) { return (u32)TRANSCRIPT_HEAD_WORDS + 8u * count; }

ARK_HD u64 keccak_rotl(u64 x, int n) { return (x << n) | (x >> (64 - n)); }

// Keccak-f[1600] on 25 64-bit lanes, a[x + 5 y] (FIPS 202 section 3.2)
ARK_HD void keccak_f1600(u64 (&a)[25]) {
  static constexpr u64 RC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
      0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
      0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
      0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  constexpr int ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
  constexpr int PIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
#pragma unroll 1
  for (int round = 0; round < 24; round++) {
    u64 c[5];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) {
      const u64 d = c[(x + 4) % 5] ^ keccak_rotl(c[(x + 1) % 5], 1);
#pragma unroll
      for (int y = 0; y < 25; y += 5) a[x + y] ^= d;
    }
    u64 t = a[1];
#pragma unroll
    for (int i = 0; i < 24; i++) {
      const u64 next = a[PIL[i]];
      a[PIL[i]] = keccak_rotl(t, ROT[i]);
      t = next;
    }
#pragma unroll
    for (int y = 0; y < 25; y += 5) {
      u64 row[5];
#pragma unroll
      for (int x = 0; x < 5; x++) row[x] = a[y + x];
#pragma unroll
      for (int x = 0; x < 5; x++) a[y + x] = row[x] ^ (~row[(x + 1) % 5] & row[(x + 2) % 5]);
    }
    a[0] ^= RC[round];
  }
}

// word i of the padded message: the message, then SHAKE's suffix 1111 and the first padding bit (0x1f); the last padding bit
// (0x80 in the block's last byte) is added by the caller
ARK_HD u32 shake_word(const u32* msg, u32 nwords, u32 i) { return i < nwords ? msg[i] : (i == nwords ? 0x1fu : 0u); }

// out[0 .. 23] = the first 96 bytes of SHAKE256(msg[0 .. nwords)) as little-endian words
ARK_HD void shake256_96(const u32* msg, u32 nwords, u32* out) {
  u64 a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
  const u32 blocks = nwords / (u32)TRANSCRIPT_RATE_WORDS + 1;   // a message that fills its last block gets one of padding alone
#pragma unroll 1
  for (u32 b = 0; b < blocks; b++) {
    const u32 base = b * (u32)TRANSCRIPT_RATE_WORDS;
#pragma unroll
    for (int j = 0; j < TRANSCRIPT_RATE_WORDS / 2; j++)
      a[j] ^= (u64)shake_word(msg, nwords, base + 2 * j) | ((u64)shake_word(msg, nwords, base + 2 * j + 1) << 32);
    if (b + 1 == blocks) a[TRANSCRIPT_RATE_WORDS / 2 - 1] ^= 0x8000000000000000ull;
    keccak_f1600(a);
  }
#pragma unroll
  for (int j = 0; j < 12; j++) {   // 96 bytes < the rate: one squeeze
    out[2 * j] = (u32)a[j];
    out[2 * j + 1] = (u32)(a[j] >> 32);
  }
}

// int_le(w[0 .. 15]) mod r in Montgomery form: with the 512 bits split as lo + 2^256 hi and R = 2^256,
//   (lo + R hi) R = mont(lo, R^2) + mont(hi, R^3),   R^3 = mont(R^2, R^2).
// A Montgomery product takes ANY 256-bit first operand when the second is canonical: (a b + m p) / R < 2p for a < R, b < p.
template <class F>
ARK_HD F transcript_reduce512(const u32* w) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  F lo, hi, r2;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    lo.l[i] = w[i];
    hi.l[i] = w[8 + i];
    r2.l[i] = F::P::R2[i];
  }
  return F::add(F::mul(lo, r2), F::mul(hi, F::mul(r2, r2)));
}

// the eight words of element number `at` of a message
template <class F>
ARK_HD void transcript_put_element(u32* msg, u32 at, const F& mont) {
  const F x = F::from_mont(mont);
#pragma unroll
  for (int i = 0; i < 8; i++) msg[TRANSCRIPT_HEAD_WORDS + 8 * at + i] = x.l[i];
}

// msg: transcript_words(count) words, elements in place, msg[0 .. 7] the state; sets msg[8], overwrites msg[0 .. 7] with the new
// state and returns the challenge
template <class F>
ARK_HD F transcript_challenge_words(u32* msg, u32 count) {
  msg[TRANSCRIPT_STATE_WORDS] = count;
  u32 out[24];
  shake256_96(msg, transcript_words(count), out);
#pragma unroll
  for (int i = 0; i < TRANSCRIPT_STATE_WORDS; i++) msg[i] = out[i];
  return transcript_reduce512<F>(out + TRANSCRIPT_STATE_WORDS);
}

}  // namespace arkhip
