// product_tree, linear_combination and GrandProduct::prove of the C++ mirror (include/ark_hip.hpp) driven from a compiled C++
// program on the GPU at 9 variables over BLS12-381 Fr, against values the caller computed with big integers and against the
// oracle's field arithmetic:
//   argv: product  left  right  claim     (each 64 hex digits: 4 limbs, most significant first)
//   product = the product of the table; left, right = the last layer's pair; claim = the verifier's last claim f(point).
// The table is the oracle's seeded scalars (seed 61) and the challenges are the oracle's seeded scalars (seed 62) in the order
// they are asked for, which the caller generates the same way.
// Built and run by tests/test_gpu_cpp_grand_product.py (g++, links libark_hip.so and the oracle).
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
  const Fr product = parse(argv[1]), left = parse(argv[2]), right = parse(argv[3]), claim = parse(argv[4]);
  const size_t n = (size_t)1 << NV;
  std::vector<Fr> t(n), ch(64);
  ark_oracle_gen_scalars(FIELD, 61, n, 1, reinterpret_cast<uint64_t*>(t.data()));
  ark_oracle_gen_scalars(FIELD, 62, ch.size(), 1, reinterpret_cast<uint64_t*>(ch.data()));
  M f = M::from_evaluations_vec(NV, t);

  // the tree: every element with the oracle's arithmetic, the product against the caller's
  {
    typename M::ProductTree tree = f.product_tree();
    EXPECT(tree.product == product, "tree: the product against the caller's value");
    std::vector<Fr> up = t;
    size_t at = 0;
    bool same = true;
    for (size_t j = 1; j <= NV; j++) {
      EXPECT(tree.level_offset(j) == at && tree.level_len(j) == up.size() / 2, "tree: the levels tile the vector");
      const std::vector<Fr> lv = tree.level_to_vec(j);
      std::vector<Fr> next(up.size() / 2);
      for (size_t i = 0; i < next.size(); i++) {
        next[i] = op(2, up[i], up[i + next.size()]);
        same = same && lv[i] == next[i];
      }
      at += lv.size();
      up = next;
    }
    EXPECT(same, "tree: every element against the oracle's arithmetic");
    EXPECT(at == n - 1 && tree.all.len() == n - 1 && up[0] == product, "tree: 2^nv - 1 elements, the product last");
    EXPECT(f.to_evaluations() == t, "tree: input untouched");
    size_t levels = 0;
    for (auto& launches : M::product_tree_plan(NV)) levels += (size_t)launches.first;
    EXPECT(levels == NV, "tree: the plan's levels");
    // a view frees nothing and cannot leave its owner
    {
      Vec v = tree.level(NV);
      EXPECT(v.is_view() && v.len() == 1 && v.to_vec()[0] == product, "view: the last level is the product");
    }
    EXPECT(tree.level_to_vec(NV)[0] == product, "view: the owner outlives its view");
    bool threw = false;
    try { Vec::view(tree.all, n - 2, 2); } catch (const Error&) { threw = true; }
    EXPECT(threw, "view: leaving the owner is refused");
    EXPECT(M::from_evaluations_vec(0, {t[5]}).product_tree().product == t[5], "tree: of a constant");
  }

  // the linear combination: every element with the oracle's arithmetic
  {
    std::vector<Fr> t2(n), t3(n);
    ark_oracle_gen_scalars(FIELD, 63, n, 1, reinterpret_cast<uint64_t*>(t2.data()));
    ark_oracle_gen_scalars(FIELD, 64, n, 1, reinterpret_cast<uint64_t*>(t3.data()));
    M f2 = M::from_evaluations_vec(NV, t2), f3 = M::from_evaluations_vec(NV, t3);
    const std::vector<Fr> c = {ch[60], ch[61], ch[62]};
    const Fr gamma = ch[63];
    M with = M::linear_combination({&f, &f2, &f3}, c, &gamma), without = M::linear_combination({&f, &f2, &f3}, c);
    const std::vector<Fr> a = with.to_evaluations(), b = without.to_evaluations();
    bool same = a.size() == n && b.size() == n;
    for (size_t i = 0; same && i < n; i++) {
      const Fr s = op(0, op(0, op(2, c[0], t[i]), op(2, c[1], t2[i])), op(2, c[2], t3[i]));
      same = b[i] == s && a[i] == op(0, gamma, s);
    }
    EXPECT(same, "linear_combination: every element against the oracle's arithmetic");
    bool threw = false;
    try { M::linear_combination({&f, &f2}, c); } catch (const Error&) { threw = true; }
    EXPECT(threw, "linear_combination: one coefficient per table");
  }

  // the layered proof: the challenges are ch[0], ch[1], .. in the order they are asked for
  {
    size_t asked = 0;
    GrandProduct<FIELD> gp(f);
    GrandProductProof<FIELD> proof = gp.prove([&](size_t, int, const std::vector<Fr>&) { return ch[asked++]; });
    EXPECT(proof.product == product, "prove: the product");
    EXPECT(proof.pairs.size() == NV && proof.sumchecks.size() == NV && proof.point.size() == NV, "prove: one layer per variable");
    EXPECT(asked == 1 + (NV - 1) * (NV + 2) / 2, "prove: one challenge per round and one per layer");
    EXPECT(!proof.sumchecks[0].has_value() && op(2, proof.pairs[0].first, proof.pairs[0].second) == product, "prove: layer 0");
    // the verifier's chain of claims with the oracle's arithmetic: every layer's first round sums to the claim before it
    size_t at = 0;
    Fr cl = op(0, proof.pairs[0].first, op(2, ch[at++], op(1, proof.pairs[0].second, proof.pairs[0].first)));
    bool chain = true;
    for (size_t k = 1; k < NV; k++) {
      const SumcheckProof<FIELD>& sc = *proof.sumchecks[k];
      chain = chain && sc.rounds.size() == k && op(0, sc.rounds[0][0], sc.rounds[0][1]) == cl;
      for (size_t i = 0; i < k; i++) chain = chain && sc.point[i] == ch[at + i];
      at += k;
      chain = chain && op(2, sc.final_evaluations[0], op(2, proof.pairs[k].first, proof.pairs[k].second)) == sc.final_value;
      cl = op(0, proof.pairs[k].first, op(2, ch[at++], op(1, proof.pairs[k].second, proof.pairs[k].first)));
    }
    EXPECT(chain, "prove: every layer's sumcheck starts from the claim the layer before left");
    EXPECT(proof.pairs.back().first == left && proof.pairs.back().second == right, "prove: the last pair against the caller's");
    EXPECT(cl == claim, "prove: the last claim against the caller's");
    EXPECT(f.evaluate(proof.point) == claim, "prove: f(point) on the device is the last claim");
    EXPECT(f.to_evaluations() == t, "prove: input untouched");
  }
}

int main(int argc, char** argv) {
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 5) { std::printf("usage: grand_product_check product left right claim\n"); return 3; }
  run(argv);
  ark_hip_shutdown();
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
