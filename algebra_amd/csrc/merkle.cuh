// Merkle commitments over column batches: SHA3-256 leaves and nodes, written once for host and device
// like transcript.cuh, whose Keccak-f[1600] this file uses at throughput: one hash per lane, the 25-lane state in registers.
//   leaf(i) = H( u32_le(count) | u32_le(elem_bytes) | ser(col_0[i]) | .. | ser(col_{count-1}[i]) )
//   node    = H( u32_le(0xFFFFFFFF) | u32_le(0) | left | right )                               (72 bytes: one permutation)
// H = SHA3-256: rate 136 bytes = 17 lanes of 64 bits, suffix 0x06, last padding bit 0x80 in the block's last byte.  Every message
// is a whole number of 32-bit words, so the sponge absorbs LANES that a function of the lane index generates (header, element
// words, suffix, zero) -- the manner of shake_word.  The state is addressed with compile-time indices only.
// The tree: 2n - 1 digests, node t at byte 32 t, root t = 0, children 2t + 1 and 2t + 2, leaf i at t = n - 1 + i.  Level l holds
// the 2^l nodes 2^l - 1 .. 2^(l+1) - 2; the leaves are level log n.
#pragma once
#include "transcript.cuh"

namespace arkhip {

constexpr int MERKLE_RATE_LANES = 17;        // 136 bytes
constexpr int MERKLE_BLOCK = 256;            // threads of every kernel here
constexpr int MERKLE_BLOCK_LOG = 8;
// The node levels of a tree of 2^k leaves are k - 1 .. 0.  One workgroup computes levels min(TAIL_LOG, k - 1) .. 0 in one launch
// (the tail); the levels above go NODE_LEVELS at a time, from the top, one workgroup per 256 nodes of a launch's first level.
constexpr int MERKLE_TAIL_LOG = 8;           // <= MERKLE_BLOCK_LOG: one node per lane
constexpr int MERKLE_NODE_LEVELS = 4;        // <= MERKLE_BLOCK_LOG + 1
constexpr int MERKLE_PERM = 1;               // the permutation of the kernels: 0 keccak_f1600, 1 merkle_f1600 (below)
constexpr u64 MERKLE_NODE_HEADER = 0x00000000FFFFFFFFull;
constexpr u64 MERKLE_SUFFIX = 0x06;
constexpr u64 MERKLE_LAST_BIT = 0x8000000000000000ull;

// ---- a second permutation: the same function, shaped for a lane-per-hash kernel ---------------------------------------------
// keccak_f1600 walks rho and pi as one chain through a temporary and rotates on 64 bits; hipcc turns that into pairs of 64-bit
// shifts and a move per step.  Here a round is out of place (B = pi(rho(theta(A))), A = chi(B)), a rotation works on the two
// 32-bit halves (one v_alignbit_b32 each; by 32: a swap of names), and two rounds make one loop body.
ARK_HD u64 merkle_rotl(u64 x, int n) {   // 0 <= n < 64, a constant once unrolled
#if defined(__HIP_DEVICE_COMPILE__)
  if (n == 0) return x;
  u32 lo = (u32)x, hi = (u32)(x >> 32);
  if (n >= 32) {
    const u32 t = lo;
    lo = hi;
    hi = t;
    n -= 32;
  }
  if (n == 0) return ((u64)hi << 32) | lo;
  const u32 nh = __builtin_amdgcn_alignbit(hi, lo, 32 - n), nl = __builtin_amdgcn_alignbit(lo, hi, 32 - n);
  return ((u64)nh << 32) | nl;
#else
  return n ? (x << n) | (x >> (64 - n)) : x;
#endif
}
ARK_HD void merkle_round(u64 (&a)[25], u64 rc) {
  constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};   // [x + 5 y]
  u64 c[5], d[5], b[25];
#pragma unroll
  for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
  for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ merkle_rotl(c[(x + 1) % 5], 1);
#pragma unroll
  for (int y = 0; y < 5; y++)
#pragma unroll
    for (int x = 0; x < 5; x++) b[y + 5 * ((2 * x + 3 * y) % 5)] = merkle_rotl(a[x + 5 * y] ^ d[x], RHO[x + 5 * y]);
#pragma unroll
  for (int y = 0; y < 25; y += 5)
#pragma unroll
    for (int x = 0; x < 5; x++) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
  a[0] ^= rc;
}
ARK_HD void merkle_f1600(u64 (&a)[25]) {
  static constexpr u64 RC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
      0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
      0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
      0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
#pragma unroll 1
  for (int round = 0; round < 24; round += 2) {
    merkle_round(a, RC[round]);
    merkle_round(a, RC[round + 1]);
  }
}
// PERM 0: keccak_f1600 as the transcript has it; PERM 1: merkle_f1600
template <int PERM>
ARK_HD void merkle_permute(u64 (&a)[25]) {
  if constexpr (PERM == 0) keccak_f1600(a);
  else merkle_f1600(a);
}

// ---- the sponge over generated lanes -------------------------------------------------------------------------------------
// permutations of a message of `words` 32-bit words: the suffix needs room, so a message that fills its last block gets one more
ARK_HD u64 merkle_blocks(u64 words) { return words / (2 * MERKLE_RATE_LANES) + 1; }
ARK_HD u64 merkle_leaf_words(u64 count, unsigned elem_bytes) { return 2 + count * (elem_bytes / 4); }

// d = SHA3-256 of the message whose padded lane g (suffix included, last bit not) is src.lane(g).  The lanes of block b + 1 are
// generated -- on the device: their loads issued -- before block b is permuted.
template <int PERM, class Src>
ARK_HD void merkle_sponge(Src& src, u64 blocks, u64 (&d)[4]) {
  u64 a[25], nxt[MERKLE_RATE_LANES];
#pragma unroll
  for (int j = 0; j < 25; j++) a[j] = 0;
#pragma unroll
  for (int j = 0; j < MERKLE_RATE_LANES; j++) nxt[j] = src.lane((u64)j);
#pragma unroll 1
  for (u64 b = 0; b < blocks; b++) {
#pragma unroll
    for (int j = 0; j < MERKLE_RATE_LANES; j++) a[j] ^= nxt[j];
    if (b + 1 == blocks) {
      a[MERKLE_RATE_LANES - 1] ^= MERKLE_LAST_BIT;
    } else {
#pragma unroll
      for (int j = 0; j < MERKLE_RATE_LANES; j++) nxt[j] = src.lane((b + 1) * MERKLE_RATE_LANES + (u64)j);
    }
    merkle_permute<PERM>(a);
  }
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = a[j];
}

// a row of one-word elements (T = uint32_t or uint64_t) hashed as it lies: element e at p[e * stride]
template <class T>
struct MerkleWordRow {
  const T* p;
  size_t stride;
  u64 count;
  ARK_HD u64 word(u64 e) const { return e < count ? (u64)p[e * stride] : (e == count ? MERKLE_SUFFIX : 0); }
  ARK_HD u64 lane(u64 g) const {
    if (g == 0) return count | ((u64)sizeof(T) << 32);
    if constexpr (sizeof(T) == 8) return word(g - 1);
    else return word(2 * g - 2) | (word(2 * g - 1) << 32);
  }
};
// a row of 32-byte Montgomery elements (F = Fp<..>, eight 32-bit limbs): element e at p + e * stride * 32, hashed as its canonical
// value.  Lane g is the same in every lane of a wave, so the conversion of an element runs once for its four lanes.
template <class F>
struct MerkleFrRow {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  const char* p;
  size_t stride;
  u64 count;
  u64 cur;
  F x;
  ARK_HD MerkleFrRow(const void* p_, size_t stride_, u64 count_) : p((const char*)p_), stride(stride_), count(count_), cur(~(u64)0) {}
  ARK_HD u64 lane(u64 g) {
    if (g == 0) return count | ((u64)32 << 32);
    const u64 e = (g - 1) >> 2;
    const unsigned part = (unsigned)((g - 1) & 3);
    if (e >= count) return (e == count && part == 0) ? MERKLE_SUFFIX : 0;
    if (e != cur) {
      x = F::from_mont(F::load(p + e * stride * 32));
      cur = e;
    }
    const u32 lo = part == 0 ? x.l[0] : part == 1 ? x.l[2] : part == 2 ? x.l[4] : x.l[6];
    const u32 hi = part == 0 ? x.l[1] : part == 1 ? x.l[3] : part == 2 ? x.l[5] : x.l[7];
    return ((u64)hi << 32) | lo;
  }
};
struct MerkleNodeMsg {
  const u64* l;
  const u64* r;
  ARK_HD u64 lane(u64 g) const { return g == 0 ? MERKLE_NODE_HEADER : g < 5 ? l[g - 1] : g < 9 ? r[g - 5] : g == 9 ? MERKLE_SUFFIX : 0; }
};
// one permutation, every lane index a constant
template <int PERM>
ARK_HD void merkle_node_digest(const u64 (&l)[4], const u64 (&r)[4], u64 (&d)[4]) {
  u64 a[25];
#pragma unroll
  for (int j = 0; j < 25; j++) a[j] = 0;
  a[0] = MERKLE_NODE_HEADER;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    a[1 + j] = l[j];
    a[5 + j] = r[j];
  }
  a[9] = MERKLE_SUFFIX;
  a[MERKLE_RATE_LANES - 1] = MERKLE_LAST_BIT;
  merkle_permute<PERM>(a);
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = a[j];
}

// ---- the plan: pure host arithmetic ---------------------------------------------------------------------------------------
// The two seams and the permutation, for A/B measurements (tools/bench_merkle.py): ARK_HIP_MERKLE_TAIL_LOG (0 .. 8),
// ARK_HIP_MERKLE_LEVELS (1 .. 9), ARK_HIP_MERKLE_PERM (0, 1); read on every call, anything out of range is the default.
struct MerkleKnobs { int tail_log, node_levels, perm; };
inline MerkleKnobs merkle_knobs() {
  auto env = [](const char* name, int lo, int hi, int dflt) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    const int v = atoi(e);
    return v < lo || v > hi ? dflt : v;
  };
  return MerkleKnobs{env("ARK_HIP_MERKLE_TAIL_LOG", 0, MERKLE_BLOCK_LOG, MERKLE_TAIL_LOG),
                     env("ARK_HIP_MERKLE_LEVELS", 1, MERKLE_BLOCK_LOG + 1, MERKLE_NODE_LEVELS), env("ARK_HIP_MERKLE_PERM", 0, 1, MERKLE_PERM)};
}
struct MerklePlan {
  int k;             // log n
  int tail_top;      // the tail's first level, -1 without node levels (n = 1)
  int multi;         // multi-level launches above the tail
  int node_levels;   // levels of one of them (the last may be shorter)
  u64 leaf_blocks, node_blocks;   // workgroups of the leaf launch and of the first multi-level launch (0 without one)
  u64 leaf_perms;    // permutations of one leaf
};
inline MerklePlan merkle_plan(int k, u64 count, unsigned elem_bytes, const MerkleKnobs& kn = merkle_knobs()) {
  MerklePlan pl{};
  pl.k = k;
  pl.node_levels = kn.node_levels;
  pl.tail_top = k == 0 ? -1 : (k - 1 < kn.tail_log ? k - 1 : kn.tail_log);
  const int above = k - 1 - pl.tail_top;   // levels k - 1 .. tail_top + 1
  pl.multi = k == 0 ? 0 : (above + kn.node_levels - 1) / kn.node_levels;
  pl.leaf_blocks = k <= MERKLE_BLOCK_LOG ? 1 : (u64)1 << (k - MERKLE_BLOCK_LOG);
  pl.node_blocks = pl.multi ? (k - 1 > MERKLE_BLOCK_LOG ? (u64)1 << (k - 1 - MERKLE_BLOCK_LOG) : 1) : 0;
  pl.leaf_perms = merkle_blocks(merkle_leaf_words(count, elem_bytes));
  return pl;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
ARK_DEV void merkle_store_digest(char* tree, size_t t, const u64 (&d)[4]) {
  ulonglong2* q = (ulonglong2*)(tree + 32 * t);
  q[0] = make_ulonglong2(d[0], d[1]);
  q[1] = make_ulonglong2(d[2], d[3]);
}
ARK_DEV void merkle_load_digest(const char* tree, size_t t, u64 (&d)[4]) {
  const ulonglong2* q = (const ulonglong2*)(tree + 32 * t);
  const ulonglong2 a = q[0], b = q[1];
  d[0] = a.x; d[1] = a.y; d[2] = b.x; d[3] = b.y;
}

// one leaf per lane: lane i reads element i of every column, so a wave's loads are consecutive
template <class T, int PERM>
__global__ void __launch_bounds__(MERKLE_BLOCK) merkle_leaves_word_kernel(const T* data, u64 count, size_t stride, size_t n, u64 blocks,
                                                                          char* tree) {
  const size_t i = (size_t)blockIdx.x * MERKLE_BLOCK + threadIdx.x;
  if (i >= n) return;
  MerkleWordRow<T> row{data + i, stride, count};
  u64 d[4];
  merkle_sponge<PERM>(row, blocks, d);
  merkle_store_digest(tree, n - 1 + i, d);
}
template <class F, int PERM>
__global__ void __launch_bounds__(MERKLE_BLOCK) merkle_leaves_fr_kernel(const char* data, u64 count, size_t stride, size_t n, u64 blocks,
                                                                        char* tree) {
  const size_t i = (size_t)blockIdx.x * MERKLE_BLOCK + threadIdx.x;
  if (i >= n) return;
  MerkleFrRow<F> row(data + i * 32, stride, count);
  u64 d[4];
  merkle_sponge<PERM>(row, blocks, d);
  merkle_store_digest(tree, n - 1 + i, d);
}

// `levels` node levels from `top` downwards, one node per lane.  A workgroup owns min(256, 2^top) nodes of level `top` and every
// node below them that the launch reaches: the first level reads its children from the tree, the others from LDS (two buffers
// in turn, one digest word per array so that a wave's accesses are consecutive).  levels <= log2(nodes per workgroup) + 1.
template <int PERM>
__global__ void __launch_bounds__(MERKLE_BLOCK) merkle_nodes_kernel(char* tree, int top, int levels) {
  __shared__ u64 sh[2][4][MERKLE_BLOCK];
  const unsigned t = threadIdx.x;
  const unsigned wtop = top < MERKLE_BLOCK_LOG ? 1u << top : (unsigned)MERKLE_BLOCK;
  for (int j = 0; j < levels; j++) {
    const unsigned width = wtop >> j;
    if (t < width) {
      const size_t id = (((size_t)1 << (top - j)) - 1) + (size_t)blockIdx.x * width + t;
      u64 l[4], r[4], d[4];
      if (j == 0) {
        merkle_load_digest(tree, 2 * id + 1, l);
        merkle_load_digest(tree, 2 * id + 2, r);
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          l[q] = sh[(j - 1) & 1][q][2 * t];
          r[q] = sh[(j - 1) & 1][q][2 * t + 1];
        }
      }
      merkle_node_digest<PERM>(l, r, d);
      merkle_store_digest(tree, id, d);
#pragma unroll
      for (int q = 0; q < 4; q++) sh[j & 1][q][t] = d[q];
    }
    __syncthreads();
  }
}

// the openings: lanes [0, q k) copy the sibling of query / level, lanes [q k, q (k + count)) the element of query / column
static __global__ void __launch_bounds__(MERKLE_BLOCK) merkle_open_kernel(const char* tree, size_t n, int k, const char* data, unsigned elem_bytes,
                                                                   u64 count, size_t stride, const u64* indices, size_t q, char* paths,
                                                                   char* rows) {
  const size_t g = (size_t)blockIdx.x * MERKLE_BLOCK + threadIdx.x;
  const size_t npath = q * (size_t)k;
  if (g < npath) {
    const size_t qi = g / (size_t)k;
    const int lev = (int)(g % (size_t)k);
    const size_t h = ((n + (size_t)indices[qi]) >> lev) ^ 1;   // the sibling, numbered from 1
    u64 d[4];
    merkle_load_digest(tree, h - 1, d);
    merkle_store_digest(paths, g, d);
    return;
  }
  const size_t e = g - npath;
  if (!data || e >= q * count) return;
  const size_t qi = e / count, col = e % count;
  const size_t at = col * stride + (size_t)indices[qi];
  if (elem_bytes == 4) ((u32*)rows)[e] = ((const u32*)data)[at];
  else if (elem_bytes == 8) ((u64*)rows)[e] = ((const u64*)data)[at];
  else {
    const ulonglong2* s = (const ulonglong2*)(data + at * 32);
    ulonglong2* o = (ulonglong2*)(rows + e * 32);
    o[0] = s[0];
    o[1] = s[1];
  }
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
inline int merkle_launch_ok() { return hipGetLastError() == hipSuccess ? 0 : -1000; }

template <class T>
int merkle_leaves_word_launch(const void* data, u64 count, size_t stride, size_t n, void* tree, int perm, hipStream_t s) {
  const u64 perms = merkle_blocks(merkle_leaf_words(count, sizeof(T)));
  const dim3 grid((unsigned)((n + MERKLE_BLOCK - 1) / MERKLE_BLOCK)), block(MERKLE_BLOCK);
  if (perm)
    hipLaunchKernelGGL((merkle_leaves_word_kernel<T, 1>), grid, block, 0, s, (const T*)data, count, stride, n, perms, (char*)tree);
  else
    hipLaunchKernelGGL((merkle_leaves_word_kernel<T, 0>), grid, block, 0, s, (const T*)data, count, stride, n, perms, (char*)tree);
  return merkle_launch_ok();
}
template <class F>
int merkle_leaves_fr_launch(const void* data, u64 count, size_t stride, size_t n, void* tree, int perm, hipStream_t s) {
  const u64 perms = merkle_blocks(merkle_leaf_words(count, 32));
  const dim3 grid((unsigned)((n + MERKLE_BLOCK - 1) / MERKLE_BLOCK)), block(MERKLE_BLOCK);
  if (perm)
    hipLaunchKernelGGL((merkle_leaves_fr_kernel<F, 1>), grid, block, 0, s, (const char*)data, count, stride, n, perms, (char*)tree);
  else
    hipLaunchKernelGGL((merkle_leaves_fr_kernel<F, 0>), grid, block, 0, s, (const char*)data, count, stride, n, perms, (char*)tree);
  return merkle_launch_ok();
}
// every node level of a tree whose leaves are written: pl.multi launches from the top, then the tail
inline int merkle_nodes_launch(void* tree, const MerklePlan& pl, int perm, hipStream_t s) {
  if (pl.k == 0) return 0;
  for (int top = pl.k - 1; top > pl.tail_top; top -= pl.node_levels) {
    const int levels = top - pl.tail_top < pl.node_levels ? top - pl.tail_top : pl.node_levels;
    const dim3 grid(top > MERKLE_BLOCK_LOG ? 1u << (top - MERKLE_BLOCK_LOG) : 1u), block(MERKLE_BLOCK);
    if (perm) hipLaunchKernelGGL((merkle_nodes_kernel<1>), grid, block, 0, s, (char*)tree, top, levels);
    else hipLaunchKernelGGL((merkle_nodes_kernel<0>), grid, block, 0, s, (char*)tree, top, levels);
    if (int rc = merkle_launch_ok()) return rc;
  }
  if (perm) hipLaunchKernelGGL((merkle_nodes_kernel<1>), dim3(1), dim3(MERKLE_BLOCK), 0, s, (char*)tree, pl.tail_top, pl.tail_top + 1);
  else hipLaunchKernelGGL((merkle_nodes_kernel<0>), dim3(1), dim3(MERKLE_BLOCK), 0, s, (char*)tree, pl.tail_top, pl.tail_top + 1);
  return merkle_launch_ok();
}
inline int merkle_open_launch(const void* tree, size_t n, int k, const void* data, unsigned elem_bytes, u64 count, size_t stride,
                              const void* d_indices, size_t q, void* d_paths, void* d_rows, hipStream_t s) {
  const size_t lanes = q * ((size_t)k + (data ? (size_t)count : 0));
  if (lanes == 0) return 0;
  hipLaunchKernelGGL(merkle_open_kernel, dim3((unsigned)((lanes + MERKLE_BLOCK - 1) / MERKLE_BLOCK)), dim3(MERKLE_BLOCK), 0, s,
                     (const char*)tree, n, k, (const char*)data, elem_bytes, count, stride, (const u64*)d_indices, q, (char*)d_paths,
                     (char*)d_rows);
  return merkle_launch_ok();
}

}  // namespace arkhip
