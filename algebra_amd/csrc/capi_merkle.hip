// C ABI of the Merkle commitments (ark_hip_merkle_*): SHA3-256 trees over column batches of the one-word fields and of the
// four-limb scalar fields.  The leaf kernel of 4- and 8-byte elements, the node kernels and the open kernel need no field and are
// instantiated here; the leaf kernel of 32-byte elements converts out of Montgomery form and comes through FieldOps.  The host
// entries (leaf, node, verify, plan) run the same hashing source and need no GPU.  DESIGN.md section 28.
#include "capi_core.hpp"
#include "merkle.cuh"
#include "sfp.cuh"

using namespace arkhip;
using namespace arkhip::capi;

namespace {

// element bytes of a one-word field, 0 for an unknown id
unsigned sfp_elem_bytes(int sfield) {
  switch (sfield) {
    case ARK_HIP_SFP_GOLDILOCKS: return sizeof(GOLDILOCKS::T);
    case ARK_HIP_SFP_BABYBEAR: return sizeof(BABYBEAR::T);
    case ARK_HIP_SFP_KOALABEAR: return sizeof(KOALABEAR::T);
  }
  return 0;
}
int log2_exact(size_t n) {   // -1 unless n = 2^k
  if (n == 0 || (n & (n - 1))) return -1;
  int k = 0;
  while (((size_t)1 << k) != n) k++;
  return k;
}
bool count_ok(size_t count) { return count >= 1 && (uint64_t)count <= 0xFFFFFFFEull; }

// the host hashing always runs merkle_f1600: both permutations are the same function
void digest_out(const u64 (&d)[4], uint8_t* out) { memcpy(out, d, 32); }   // little-endian host
void leaf_words_host(unsigned elem_bytes, const void* row, size_t count, uint8_t* out) {
  u64 d[4];
  const u64 blocks = merkle_blocks(merkle_leaf_words(count, elem_bytes));
  if (elem_bytes == 8) {
    MerkleWordRow<uint64_t> r{(const uint64_t*)row, 1, count};
    merkle_sponge<1>(r, blocks, d);
  } else {
    MerkleWordRow<uint32_t> r{(const uint32_t*)row, 1, count};
    merkle_sponge<1>(r, blocks, d);
  }
  digest_out(d, out);
}
template <class FP>
int leaf_fr_host(const uint64_t* row, size_t count, uint8_t* out) {
  u64 d[4];
  MerkleFrRow<Fp<FP>> r(row, 1, count);
  merkle_sponge<1>(r, merkle_blocks(merkle_leaf_words(count, 32)), d);
  digest_out(d, out);
  return 0;
}
int leaf_fr_any(int field, const uint64_t* row, size_t count, uint8_t* out) {
#define X(NAME) leaf_fr_host<NAME>(row, count, out)
  ARK_FIELD_SWITCH(field, X);
#undef X
}
void node_host(const uint8_t* left, const uint8_t* right, uint8_t* out) {
  u64 l[4], r[4], d[4];
  memcpy(l, left, 32);
  memcpy(r, right, 32);
  merkle_node_digest<1>(l, r, d);
  digest_out(d, out);
}
// leaf -> root along the path; index < n = 2^k checked by the caller
int verify_from_leaf(const uint8_t* leaf, const uint8_t* root, int k, uint64_t index, const uint8_t* path) {
  uint8_t cur[32], nxt[32];
  memcpy(cur, leaf, 32);
  for (int lev = 0; lev < k; lev++, index >>= 1) {
    const uint8_t* sib = path + 32 * (size_t)lev;
    if (index & 1) node_host(sib, cur, nxt);
    else node_host(cur, sib, nxt);
    memcpy(cur, nxt, 32);
  }
  return memcmp(cur, root, 32) == 0 ? 1 : 0;
}

// [a, a + na) and [b, b + nb) share a byte
bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}
// the checks every device entry shares; *extent = bytes from d_data to the end of the last column
int matrix_check(unsigned elem_bytes, const void* d_data, size_t count, size_t stride, size_t n, size_t* extent, int* k) {
  *k = log2_exact(n);
  if (*k < 0 || !count_ok(count) || stride < n || !d_data) return ARK_HIP_ERR_ARG;
  if ((uintptr_t)d_data % (elem_bytes < 16 ? elem_bytes : 16)) return ARK_HIP_ERR_ARG;
  const size_t lim = ~(size_t)0 / elem_bytes;
  if (n > lim || count - 1 > (lim - n) / stride) return ARK_HIP_ERR_SIZE;
  *extent = ((count - 1) * stride + n) * elem_bytes;
  return 0;
}
int tree_check(const void* d_tree, int k, size_t* bytes) {
  if (!d_tree || (uintptr_t)d_tree % 16) return ARK_HIP_ERR_ARG;
  if (k > 40) return ARK_HIP_ERR_SIZE;   // the leaf launch's grid and every byte count stay far inside their types
  *bytes = ((((size_t)1 << k) << 1) - 1) * ARK_HIP_MERKLE_DIGEST_BYTES;
  return 0;
}

// leaves by `leaves`, then the node levels; the root read back with one wait when asked for
template <class LeafFn>
int commit_entry(unsigned elem_bytes, const void* d_data, size_t count, size_t stride, size_t n, void* d_tree, uint8_t* out_root,
                 LeafFn&& leaves) {
  size_t extent, tree_bytes;
  int k;
  if (int rc = matrix_check(elem_bytes, d_data, count, stride, n, &extent, &k)) return rc;
  if (int rc = tree_check(d_tree, k, &tree_bytes)) return rc;
  if (overlaps(d_data, extent, d_tree, tree_bytes)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  const MerkleKnobs kn = merkle_knobs();
  const MerklePlan pl = merkle_plan(k, count, elem_bytes, kn);
  if (int rc = leaves(kn.perm, c->stream)) return rc;
  if (int rc = merkle_nodes_launch(d_tree, pl, kn.perm, c->stream)) return rc;
  if (!out_root) return mark_producer(c);
  ARK_HIP_TRY(hipMemcpyAsync(out_root, d_tree, ARK_HIP_MERKLE_DIGEST_BYTES, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace

extern "C" {

int ark_hip_merkle_plan(size_t n, size_t count, unsigned elem_bytes, uint64_t out[8]) {
  const int k = log2_exact(n);
  if (!out || k < 0 || !count_ok(count) || (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 32)) return ARK_HIP_ERR_ARG;
  if (k > 40) return ARK_HIP_ERR_SIZE;
  const MerkleKnobs kn = merkle_knobs();
  const MerklePlan pl = merkle_plan(k, count, elem_bytes, kn);
  out[0] = (2 * (uint64_t)n - 1) * ARK_HIP_MERKLE_DIGEST_BYTES;
  out[1] = pl.leaf_perms;
  out[2] = 1 + (uint64_t)pl.multi + (k > 0 ? 1 : 0);
  out[3] = (uint64_t)kn.tail_log;
  out[4] = pl.leaf_blocks;
  out[5] = pl.node_blocks;
  out[6] = (uint64_t)kn.node_levels;
  out[7] = (uint64_t)kn.perm;
  return 0;
}

int ark_hip_merkle_leaf_sfp(int sfield, const void* row, size_t count, uint8_t out[32]) {
  const unsigned eb = sfp_elem_bytes(sfield);
  if (!eb || !row || !out || !count_ok(count)) return ARK_HIP_ERR_ARG;
  leaf_words_host(eb, row, count, out);
  return 0;
}

int ark_hip_merkle_leaf_fr(int field, const uint64_t* row, size_t count, uint8_t out[32]) {
  if (!row || !out || !count_ok(count)) return ARK_HIP_ERR_ARG;
  return leaf_fr_any(field, row, count, out);
}

int ark_hip_merkle_node(const uint8_t left[32], const uint8_t right[32], uint8_t out[32]) {
  if (!left || !right || !out) return ARK_HIP_ERR_ARG;
  node_host(left, right, out);
  return 0;
}

int ark_hip_merkle_verify_sfp(int sfield, const uint8_t root[32], size_t n, uint64_t index, const void* row, size_t count,
                              const uint8_t* path, int* ok) {
  const unsigned eb = sfp_elem_bytes(sfield);
  const int k = log2_exact(n);
  if (!eb || !root || !row || !ok || k < 0 || !count_ok(count) || index >= (uint64_t)n || (k > 0 && !path)) return ARK_HIP_ERR_ARG;
  uint8_t leaf[32];
  leaf_words_host(eb, row, count, leaf);
  *ok = verify_from_leaf(leaf, root, k, index, path);
  return 0;
}

int ark_hip_merkle_verify_fr(int field, const uint8_t root[32], size_t n, uint64_t index, const uint64_t* row, size_t count,
                             const uint8_t* path, int* ok) {
  const int k = log2_exact(n);
  if (!root || !row || !ok || k < 0 || !count_ok(count) || index >= (uint64_t)n || (k > 0 && !path)) return ARK_HIP_ERR_ARG;
  uint8_t leaf[32];
  if (int rc = leaf_fr_any(field, row, count, leaf)) return rc;
  *ok = verify_from_leaf(leaf, root, k, index, path);
  return 0;
}

int ark_hip_merkle_commit_sfp_device(int sfield, const void* d_data, size_t count, size_t stride, size_t n, void* d_tree,
                                     uint8_t* out_root) {
  const unsigned eb = sfp_elem_bytes(sfield);
  if (!eb) return ARK_HIP_ERR_ARG;
  return commit_entry(eb, d_data, count, stride, n, d_tree, out_root, [&](int perm, hipStream_t s) {
    return eb == 8 ? merkle_leaves_word_launch<uint64_t>(d_data, count, stride, n, d_tree, perm, s)
                   : merkle_leaves_word_launch<uint32_t>(d_data, count, stride, n, d_tree, perm, s);
  });
}

int ark_hip_merkle_commit_fr_device(int field, const void* d_data, size_t count, size_t stride, size_t n, void* d_tree,
                                    uint8_t* out_root) {
  const FieldOps* ops = field_ops(field);
  if (!ops) return ARK_HIP_ERR_ARG;
  return commit_entry(32, d_data, count, stride, n, d_tree, out_root,
                      [&](int perm, hipStream_t s) { return ops->merkle_leaves(d_data, count, stride, n, d_tree, perm, s); });
}

int ark_hip_merkle_open_device(const void* d_tree, size_t n, const void* d_data, unsigned elem_bytes, size_t count, size_t stride,
                               const uint64_t* indices, size_t q, void* out_rows, uint8_t* out_paths) {
  const int k = log2_exact(n);
  if (k < 0 || (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 32)) return ARK_HIP_ERR_ARG;
  size_t tree_bytes, extent = 0;
  if (int rc = tree_check(d_tree, k, &tree_bytes)) return rc;
  if (out_rows && !d_data) return ARK_HIP_ERR_ARG;
  if (d_data) {
    int k2;
    if (!out_rows) return ARK_HIP_ERR_ARG;
    if (int rc = matrix_check(elem_bytes, d_data, count, stride, n, &extent, &k2)) return rc;
  }
  if (q && (!indices || (k > 0 && !out_paths))) return ARK_HIP_ERR_ARG;
  for (size_t i = 0; i < q; i++)
    if (indices[i] >= (uint64_t)n) return ARK_HIP_ERR_ARG;
  const size_t per_query = (size_t)k * ARK_HIP_MERKLE_DIGEST_BYTES + (d_data ? count * elem_bytes : 0);
  if (q > (~(size_t)0 >> 8) / (per_query + 8)) return ARK_HIP_ERR_SIZE;
  ARK_SCOPE(sc);
  if (q == 0) return 0;
  Context* c = sc.c;
  // staged: [paths | rows | indices], every part a multiple of 8 bytes behind a multiple of 32
  const size_t path_bytes = q * (size_t)k * ARK_HIP_MERKLE_DIGEST_BYTES, row_bytes = d_data ? q * count * elem_bytes : 0;
  const size_t idx_at = (path_bytes + row_bytes + 15) & ~(size_t)15, total = idx_at + q * 8;
  if (c->merkle_stage.cap < total)
    if (int rc = sync_compute(c)) return rc;   // the buffer is about to be replaced: nothing may still use the old one
  if (c->merkle_stage.ensure(total)) return ARK_HIP_ERR_NOMEM;
  char* st = (char*)c->merkle_stage.p;
  ARK_HIP_TRY(hipMemcpyAsync(st + idx_at, indices, q * 8, hipMemcpyHostToDevice, c->stream));
  if (int rc = merkle_open_launch(d_tree, n, k, d_data, elem_bytes, count, stride, st + idx_at, q, st, st + path_bytes, c->stream)) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  if (path_bytes + row_bytes == 0) {
    ARK_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  }
  // one copy and one wait; two destinations share it through a host buffer
  std::vector<char> host;
  char* dst = (char*)out_paths;
  if (row_bytes && path_bytes) {
    host.resize(path_bytes + row_bytes);
    dst = host.data();
  } else if (row_bytes) {
    dst = (char*)out_rows;
  }
  ARK_HIP_TRY(hipMemcpyAsync(dst, st, path_bytes + row_bytes, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  if (row_bytes && path_bytes) {
    memcpy(out_paths, host.data(), path_bytes);
    memcpy(out_rows, host.data() + path_bytes, row_bytes);
  }
  return 0;
}

}  // extern "C"
