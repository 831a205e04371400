// ark_hip::MerkleTree of include/ark_hip.hpp driven from a compiled C++ program on the GPU, against roots the Python model wrote
// (tests/test_gpu_cpp_merkle.py).  The file is a stream of decimal numbers, one block per case:
//   kind (0: BabyBear, 1: BLS12-381 Fr)  count  log_n  q
//   the matrix, column by column (count * n elements; an Fr element as four 64-bit words)
//   the root (32 bytes)   the q indices
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "ark_hip.hpp"
using namespace ark_hip;

static int fails = 0;
#define EXPECT(c, msg) do { if (!(c)) { std::printf("FAIL (case %d): %s\n", kind, msg); fails++; } } while (0)

template <class W>
static std::vector<W> take(std::ifstream& in, size_t n) {
  std::vector<W> v(n);
  for (auto& x : v) { uint64_t t; in >> t; x = (W)t; }
  return v;
}

// what both cases share once the tree stands: the root, the plan, the openings, the host verification and its refusals
template <class Verify>
static void check_tree(int kind, MerkleTree& tree, const Digest& want_root, const std::vector<uint64_t>& idx, const uint8_t* matrix,
                       size_t count, size_t n, unsigned elem_bytes, Verify&& verify) {
  EXPECT(tree.root() == want_root, "the root");
  const MerklePlan pl = merkle_plan(n, count, elem_bytes);
  EXPECT(pl.tree_bytes == (2 * n - 1) * 32 && pl.leaf_permutations == (8 + count * elem_bytes) / 136 + 1, "the plan");
  const size_t k = tree.log_size();
  const MerkleTree::Opening o = tree.open(idx);
  EXPECT(o.paths.size() == idx.size() * k * 32 && o.rows.size() == idx.size() * count * elem_bytes, "the opening's sizes");
  for (size_t i = 0; i < idx.size(); i++) {
    const uint8_t* row = o.rows.data() + i * count * elem_bytes;
    bool same = true;
    for (size_t c = 0; c < count; c++)
      same = same && std::memcmp(row + c * elem_bytes, matrix + (c * n + idx[i]) * elem_bytes, elem_bytes) == 0;
    EXPECT(same, "an opened row");
    const uint8_t* path = o.paths.data() + i * k * 32;
    EXPECT(verify(want_root, idx[i], row, path), "verify accepts the opening");
    if (k == 0) continue;
    EXPECT(!verify(want_root, idx[i] ^ 1, row, path), "verify refuses another index");
    std::vector<uint8_t> bad(path, path + k * 32);
    bad[k * 32 - 1] ^= 1;
    EXPECT(!verify(want_root, idx[i], row, bad.data()), "verify refuses an edited path");
  }
  const MerkleTree::Opening p = tree.open(idx, false);
  EXPECT(p.rows.empty() && p.paths == o.paths, "paths only");
}

int main(int argc, char** argv) {
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 2) { std::printf("usage: merkle_check vectors.txt\n"); return 3; }
  std::ifstream in(argv[1]);
  int cases = 0;
  try {
    int kind;
    uint64_t count, log, q;
    while (in >> kind >> count >> log >> q) {
      const size_t n = (size_t)1 << log;
      if (kind == 0) {
        constexpr int SF = ARK_HIP_SFP_BABYBEAR;
        const auto m = take<uint32_t>(in, count * n);
        Digest root;
        const auto rb = take<uint8_t>(in, 32);
        std::memcpy(root.data(), rb.data(), 32);
        const auto idx = take<uint64_t>(in, q);
        const auto dev = SmallDeviceVec<SF>::from_vec(m);
        MerkleTree tree = MerkleTree::commit_small<SF>(dev, count, n, n);
        check_tree(kind, tree, root, idx, (const uint8_t*)m.data(), count, n, 4, [&](const Digest& r, uint64_t i, const uint8_t* row, const uint8_t* path) {
          return MerkleTree::verify_small<SF>(r, n, i, row, count, path);
        });
        MerkleTree later = MerkleTree::commit_small<SF>(dev, count, n, n, false);   // asynchronous: the root comes from the tree
        EXPECT(later.root() == root, "the asynchronous commit");
        std::vector<uint32_t> row0(count);
        for (size_t c = 0; c < count; c++) row0[c] = m[c * n];
        EXPECT(merkle_node(merkle_leaf_small<SF>(row0), root) != root, "leaf and node on the host");
      } else {
        constexpr int F = ARK_HIP_BLS12_381_FR;
        const auto w = take<uint64_t>(in, count * n * 4);
        Digest root;
        const auto rb = take<uint8_t>(in, 32);
        std::memcpy(root.data(), rb.data(), 32);
        const auto idx = take<uint64_t>(in, q);
        std::vector<Fr> m(count * n);
        std::memcpy((void*)m.data(), w.data(), w.size() * 8);
        const auto dev = DeviceVec<F>::from_vec(m);
        MerkleTree tree = MerkleTree::commit_fr<F>(dev, count);
        check_tree(kind, tree, root, idx, (const uint8_t*)w.data(), count, n, 32, [&](const Digest& r, uint64_t i, const uint8_t* row, const uint8_t* path) {
          return MerkleTree::verify_fr<F>(r, n, i, row, count, path);
        });
        if (n == 1) EXPECT(merkle_leaf_fr<F>(m) == root, "a tree of one leaf is the leaf");
      }
      cases++;
    }
  } catch (const Error& e) {
    std::printf("FAIL: %s threw %d\n", e.what(), e.code);
    return 1;
  }
  if (fails || cases != 3 || !in.eof()) { std::printf("%d failures, %d cases\n", fails, cases); return 1; }
  std::printf("all ok\n");
  return 0;
}
