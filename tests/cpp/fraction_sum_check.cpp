// fraction_tree, count_indices and FractionalSum::prove of the C++ mirror (include/ark_hip.hpp) driven from a compiled C++
// program on the GPU at 9 variables over BLS12-381 Fr, against values the caller computed with big integers and against the
// oracle's field arithmetic:
//   argv: P  Q  n0  n1  d0  d1  claim_num  claim_den     (each 64 hex digits: 4 limbs, most significant first)
//   (P, Q) = the root; n0 .. d1 = the last layer's values; the claims = the verifier's last claims num(point), den(point).
// The tables are the oracle's seeded scalars (seeds 71 numerators, 72 denominators) and the challenges are the oracle's seeded
// scalars (seed 73) in the order they are asked for, which the caller generates the same way.
// Built and run by tests/test_gpu_cpp_fraction_sum.py (g++, links libark_hip.so and the oracle).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "ark_hip.hpp"
extern "C" {
#include "ark_oracle.h"
}
using namespace ark_hip;

static int fails = 0;
#define EXPECT(c, msg) do { if (!(c)) { std::printf("FAIL: %s\n", msg); fails++; } } while (0)

static Fr parse(const char* hex) {
  Fr r;
  const std::string s(hex);
  if (s.size() != 64) { std::printf("bad argument %s\n", hex); std::exit(3); }
  for (int i = 0; i < 4; i++) r.limbs[3 - i] = std::strtoull(s.substr(16 * i, 16).c_str(), nullptr, 16);
  return r;
}

static void run(char** argv) {
  constexpr int FIELD = ARK_HIP_BLS12_381_FR;
  constexpr size_t NV = 9;
  using M = DenseMultilinearExtension<FIELD>;
  using Vec = DeviceVec<FIELD>;
  auto op = [](int o, const Fr& a, const Fr& b) {   // the oracle's field arithmetic: 0 add, 1 sub, 2 mul
    Fr r;
    ark_oracle_field_op(FIELD, o, a.limbs.data(), b.limbs.data(), r.limbs.data(), 1);
    return r;
  };
  Fr arg[8];
  for (int i = 0; i < 8; i++) arg[i] = parse(argv[1 + i]);
  const Fr P = arg[0], Q = arg[1], claim_num = arg[6], claim_den = arg[7];
  const size_t n = (size_t)1 << NV;
  std::vector<Fr> tn(n), td(n), ch(64);
  ark_oracle_gen_scalars(FIELD, 71, n, 1, reinterpret_cast<uint64_t*>(tn.data()));
  ark_oracle_gen_scalars(FIELD, 72, n, 1, reinterpret_cast<uint64_t*>(td.data()));
  ark_oracle_gen_scalars(FIELD, 73, ch.size(), 1, reinterpret_cast<uint64_t*>(ch.data()));
  M num = M::from_evaluations_vec(NV, tn), den = M::from_evaluations_vec(NV, td);
  const Fr one = M::eq({}).to_evaluations()[0];

  // the trees: every element with the oracle's arithmetic, the root against the caller's; then with ones for numerators
  for (int has_num = 1; has_num >= 0; has_num--) {
    typename M::FractionTree tree = den.fraction_tree(has_num ? &num : nullptr);
    if (has_num) EXPECT(tree.root_num == P && tree.root_den == Q, "tree: the root against the caller's values");
    std::vector<Fr> un = has_num ? tn : std::vector<Fr>(n, one), ud = td;
    size_t at = 0;
    bool same = true;
    for (size_t j = 1; j <= NV; j++) {
      EXPECT(tree.level_offset(j) == at && tree.level_len(j) == ud.size() / 2, "tree: the levels tile the vectors");
      const std::vector<Fr> ln = tree.num_level(j).to_vec(), ld = tree.den_level(j).to_vec();
      const size_t h = ud.size() / 2;
      std::vector<Fr> nn(h), nd(h);
      for (size_t i = 0; i < h; i++) {
        nn[i] = op(0, op(2, un[i], ud[i + h]), op(2, un[i + h], ud[i]));
        nd[i] = op(2, ud[i], ud[i + h]);
        same = same && ln[i] == nn[i] && ld[i] == nd[i];
      }
      at += h;
      un = nn;
      ud = nd;
    }
    EXPECT(same, "tree: every element of both trees against the oracle's arithmetic");
    EXPECT(at == n - 1 && tree.num.len() == n - 1 && tree.den.len() == n - 1, "tree: 2^nv - 1 elements each");
    EXPECT(un[0] == tree.root_num && ud[0] == tree.root_den, "tree: the root is the last element of each tree");
    size_t levels = 0;
    for (auto& launches : M::fraction_tree_plan(NV, has_num != 0)) levels += (size_t)launches.first;
    EXPECT(levels == NV, "tree: the plan's levels");
  }
  EXPECT(num.to_evaluations() == tn && den.to_evaluations() == td, "tree: inputs untouched");
  {
    typename M::FractionTree c = M::from_evaluations_vec(0, {td[5]}).fraction_tree(nullptr);
    EXPECT(c.root_num == one && c.root_den == td[5], "tree: of a constant with a one for numerator");
  }

  // the counts: indices from the low bits of the oracle's scalars, some past the table
  {
    const size_t table_len = 100;
    std::vector<uint32_t> idx(n);
    std::vector<uint64_t> want(table_len, 0);
    for (size_t i = 0; i < n; i++) {
      idx[i] = (uint32_t)(tn[i].limbs[0] % 128);
      if (idx[i] < table_len) want[idx[i]]++;
    }
    void* d_idx = nullptr;
    EXPECT(ark_hip_malloc(n * 4, &d_idx) == 0 && ark_hip_memcpy_h2d(d_idx, idx.data(), n * 4) == 0, "counts: upload");
    Vec m = M::count_indices(static_cast<const uint32_t*>(d_idx), n, table_len);
    const std::vector<Fr> got = m.to_vec();
    bool same = got.size() == table_len;
    size_t total = 0;
    for (size_t j = 0; same && j < table_len; j++) {
      Fr c = Fr{};                                   // want[j] as an element: want[j] times one, by doubling and adding
      Fr acc = one;
      for (uint64_t b = want[j]; b; b >>= 1, acc = op(0, acc, acc))
        if (b & 1) c = op(0, c, acc);
      same = got[j] == c;
      total += want[j];
    }
    EXPECT(same, "counts: every cell against the host's count");
    EXPECT(total < n && total > 0, "counts: some indices lie past the table and are skipped");
    ark_hip_free(d_idx);
  }

  // the layered proof: the challenges are ch[0], ch[1], .. in the order they are asked for
  {
    size_t asked = 0;
    bool order = true;
    int last_round = 0;
    FractionalSum<FIELD> fs(&num, den);
    FractionalSumProof<FIELD> proof = fs.prove([&](size_t layer, int round, const std::vector<Fr>& values) {
      if (round == FractionalSum<FIELD>::LAMBDA_ROUND) order = order && values.empty() && layer > 0 && last_round == FractionalSum<FIELD>::TAU_ROUND;
      if (round == FractionalSum<FIELD>::TAU_ROUND) order = order && values.size() == 4;
      last_round = round;
      return ch[asked++];
    });
    EXPECT(order, "prove: lambda is asked for before a layer's sumcheck, with no values; tau with the layer's four");
    EXPECT(proof.root_num == P && proof.root_den == Q, "prove: the root");
    EXPECT(proof.values.size() == NV && proof.sumchecks.size() == NV && proof.point.size() == NV, "prove: one layer per variable");
    EXPECT(asked == 1 + (NV - 1) * 2 + (NV - 1) * NV / 2, "prove: one challenge per round and two per layer");
    const std::vector<Fr>& v0 = proof.values[0];
    EXPECT(!proof.sumchecks[0].has_value() && op(0, op(2, v0[0], v0[3]), op(2, v0[1], v0[2])) == P && op(2, v0[2], v0[3]) == Q, "prove: layer 0");
    // the verifier's chain of claims with the oracle's arithmetic
    size_t at = 0;
    Fr tau = ch[at++];
    Fr cn = op(0, v0[0], op(2, tau, op(1, v0[1], v0[0]))), cd = op(0, v0[2], op(2, tau, op(1, v0[3], v0[2])));
    bool chain = true;
    for (size_t k = 1; k < NV; k++) {
      const SumcheckProof<FIELD>& sc = *proof.sumchecks[k];
      const std::vector<Fr>& v = proof.values[k];
      const Fr lambda = ch[at++];
      chain = chain && sc.rounds.size() == k && v.size() == 4 && op(0, sc.rounds[0][0], sc.rounds[0][1]) == op(0, cn, op(2, lambda, cd));
      for (size_t i = 0; i < k; i++) chain = chain && sc.point[i] == ch[at + i];
      at += k;
      const Fr inner = op(0, op(0, op(2, v[0], v[3]), op(2, v[1], v[2])), op(2, lambda, op(2, v[2], v[3])));
      chain = chain && op(2, sc.final_evaluations[0], inner) == sc.final_value;
      tau = ch[at++];
      cn = op(0, v[0], op(2, tau, op(1, v[1], v[0])));
      cd = op(0, v[2], op(2, tau, op(1, v[3], v[2])));
    }
    EXPECT(chain, "prove: every layer's sumcheck starts from the batched claim the layer before left");
    const std::vector<Fr>& vl = proof.values.back();
    EXPECT(vl[0] == arg[2] && vl[1] == arg[3] && vl[2] == arg[4] && vl[3] == arg[5], "prove: the last values against the caller's");
    EXPECT(cn == claim_num && cd == claim_den, "prove: the last claims against the caller's");
    EXPECT(num.evaluate(proof.point) == claim_num && den.evaluate(proof.point) == claim_den, "prove: num(point), den(point) on the device are the last claims");
    EXPECT(num.to_evaluations() == tn && den.to_evaluations() == td, "prove: inputs untouched");
    // ones for numerators: the last layer's values are the pair (d0, d1)
    FractionalSumProof<FIELD> ones = FractionalSum<FIELD>(nullptr, den).prove([&](size_t, int, const std::vector<Fr>&) { return ch[7]; });
    EXPECT(ones.values.size() == NV && ones.values.back().size() == 2 && ones.values[0].size() == 4, "prove: ones for numerators");
  }
}

int main(int argc, char** argv) {
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 9) { std::printf("usage: fraction_sum_check P Q n0 n1 d0 d1 claim_num claim_den\n"); return 3; }
  run(argv);
  ark_hip_shutdown();
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
