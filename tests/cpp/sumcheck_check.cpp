// ListOfProducts of include/ark_hip.hpp driven from a compiled C++ program on the GPU: one whole sumcheck prover at 9
// variables for  a b c + k c a  over three tables, on the field named by argv[1].
//   argv: field id, k, r_0 .. r_8   (elements: 64 hex digits, 4 limbs, most significant first, Montgomery)
// The tables are the oracle's seeded scalars (seeds 51, 52, 53), which the caller generates the same way; the challenges are
// the caller's r_i whatever the evaluations.  The program prints its transcript -- "round i t value", "final k value",
// "value v" -- for the caller to compare with its big-integer model, and checks by itself what needs no model.
// Built and run by tests/test_gpu_cpp_sumcheck.py (g++, links libark_hip.so and the oracle).
#include <cstdio>
#include <cstdlib>
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
static void print(const char* what, size_t i, size_t t, const Fr& v) {
  std::printf("%s %zu %zu %016llx%016llx%016llx%016llx\n", what, i, t, (unsigned long long)v.limbs[3], (unsigned long long)v.limbs[2],
              (unsigned long long)v.limbs[1], (unsigned long long)v.limbs[0]);
}

template <int FIELD>
static void run(char** argv) {
  using M = DenseMultilinearExtension<FIELD>;
  constexpr size_t NV = 9;
  const Fr k = parse(argv[2]);
  std::vector<Fr> r;
  for (size_t i = 0; i < NV; i++) r.push_back(parse(argv[3 + i]));
  const size_t n = (size_t)1 << NV;
  std::vector<std::vector<Fr>> t(3, std::vector<Fr>(n));
  for (int q = 0; q < 3; q++) ark_oracle_gen_scalars(FIELD, 51 + q, n, 1, reinterpret_cast<uint64_t*>(t[q].data()));
  M a = M::from_evaluations_vec(NV, t[0]), b = M::from_evaluations_vec(NV, t[1]), c = M::from_evaluations_vec(NV, t[2]);
  Fr one{};
  ark_oracle_field_const(FIELD, 1, one.limbs.data());

  ListOfProducts<FIELD> lp(NV);
  lp.add_product({&a, &b, &c}, one);
  lp.add_product({&c, &a}, k);
  EXPECT(lp.num_vars() == NV && lp.max_multiplicands() == 3, "num_vars, max_multiplicands");
  size_t asked = 0;
  SumcheckProof<FIELD> proof = lp.prove([&](size_t i, const std::vector<Fr>& evals) {
    EXPECT(i == asked && evals.size() == 4, "challenge(i, evals): rounds in order, D + 1 evaluations");
    asked++;
    return r[i];
  });
  EXPECT(asked == NV && proof.rounds.size() == NV && proof.point == r, "nu rounds, the point is the challenges");
  for (size_t i = 0; i < proof.rounds.size(); i++)
    for (size_t e = 0; e < proof.rounds[i].size(); e++) print("round", i, e, proof.rounds[i][e]);
  EXPECT(proof.final_evaluations.size() == 3, "one final value per table");
  for (size_t q = 0; q < proof.final_evaluations.size(); q++) print("final", q, 0, proof.final_evaluations[q]);
  print("value", 0, 0, proof.final_value);

  // what needs no model: the final values are the tables at the point, and the caller's tables are as they were
  EXPECT(proof.final_evaluations.size() == 3 && a.evaluate(r) == proof.final_evaluations[0] && b.evaluate(r) == proof.final_evaluations[1] &&
             c.evaluate(r) == proof.final_evaluations[2], "final values == evaluate(point)");
  EXPECT(a.to_evaluations() == t[0] && b.to_evaluations() == t[1] && c.to_evaluations() == t[2], "inputs untouched");
  // single rounds through the same entry: a plain round of a fresh list is round 0, a round with r_0 is round 1
  ListOfProducts<FIELD> again(NV);
  again.add_product({&a, &b, &c}, one);
  again.add_product({&c, &a}, k);
  EXPECT(again.round() == proof.rounds[0] && again.round(&r[0]) == proof.rounds[1], "round(), round(r_0)");
  bool threw = false;
  try { (void)lp.round(); } catch (const Error&) { threw = true; }
  EXPECT(threw, "a round after the last is refused");
  threw = false;
  try { M small = M::from_evaluations_vec(2, std::vector<Fr>(4)); again.add_product({&small}, one); } catch (const Error&) { threw = true; }
  EXPECT(threw, "a product with another num_vars is refused");
}

int main(int argc, char** argv) {
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 3 + 9) { std::printf("usage: sumcheck_check field k r_0 .. r_8\n"); return 3; }
  switch (std::atoi(argv[1])) {
    case ARK_HIP_BN254_FR: run<ARK_HIP_BN254_FR>(argv); break;
    case ARK_HIP_BLS12_381_FR: run<ARK_HIP_BLS12_381_FR>(argv); break;
    case ARK_HIP_BLS12_377_FR: run<ARK_HIP_BLS12_377_FR>(argv); break;
    default: std::printf("unknown field\n"); return 3;
  }
  ark_hip_shutdown();
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
