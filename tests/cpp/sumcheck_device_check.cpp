// ListOfProducts::prove_device and Transcript of include/ark_hip.hpp driven from a compiled C++ program on the GPU: the whole
// sumcheck proof in one wait at 9 variables for  a b c + k c a  over three tables, on the field named by argv[1].
//   argv: field id, k (64 hex digits, 4 limbs, most significant first, Montgomery), the transcript's seed (64 hex digits: 32 bytes)
// The tables are the oracle's seeded scalars (seeds 51, 52, 53), which the caller generates the same way.  The program prints
// "round i t value", "point i 0 value", "final k 0 value", "value 0 0 v" and "state <hex>" for the caller to compare with
// its model, and checks by itself that the host-driven prove() with the Transcript as its source of challenges gives the
// same proof.  Built and run by tests/test_gpu_cpp_sumcheck_device.py (g++, links libark_hip.so and the oracle).
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
  const std::string seed_hex(argv[3]);
  if (seed_hex.size() != 64) { std::printf("bad seed\n"); std::exit(3); }
  std::array<uint8_t, 32> seed;
  for (int i = 0; i < 32; i++) seed[i] = (uint8_t)std::strtoul(seed_hex.substr(2 * i, 2).c_str(), nullptr, 16);
  const size_t n = (size_t)1 << NV;
  std::vector<std::vector<Fr>> t(3, std::vector<Fr>(n));
  for (int q = 0; q < 3; q++) ark_oracle_gen_scalars(FIELD, 51 + q, n, 1, reinterpret_cast<uint64_t*>(t[q].data()));
  M a = M::from_evaluations_vec(NV, t[0]), b = M::from_evaluations_vec(NV, t[1]), c = M::from_evaluations_vec(NV, t[2]);
  Fr one{};
  ark_oracle_field_const(FIELD, 1, one.limbs.data());

  ListOfProducts<FIELD> lp(NV);
  lp.add_product({&a, &b, &c}, one);
  lp.add_product({&c, &a}, k);
  Transcript<FIELD> tr(seed);
  EXPECT(tr.state() == seed, "the state starts as the seed");
  SumcheckProof<FIELD> proof = lp.prove_device(tr);
  EXPECT(proof.rounds.size() == NV && proof.point.size() == NV && proof.final_evaluations.size() == 3, "nu rounds, nu challenges, one final value per table");
  for (size_t i = 0; i < proof.rounds.size(); i++) {
    EXPECT(proof.rounds[i].size() == 4, "D + 1 evaluations");
    for (size_t e = 0; e < proof.rounds[i].size(); e++) print("round", i, e, proof.rounds[i][e]);
  }
  for (size_t i = 0; i < proof.point.size(); i++) print("point", i, 0, proof.point[i]);
  for (size_t q = 0; q < proof.final_evaluations.size(); q++) print("final", q, 0, proof.final_evaluations[q]);
  print("value", 0, 0, proof.final_value);
  std::printf("state ");
  for (uint8_t v : tr.state()) std::printf("%02x", v);
  std::printf("\n");

  // the host-driven prover with the same transcript as its source of challenges: the same proof, the same end state
  ListOfProducts<FIELD> host(NV);
  host.add_product({&a, &b, &c}, one);
  host.add_product({&c, &a}, k);
  Transcript<FIELD> th(seed);
  SumcheckProof<FIELD> want = host.prove([&](size_t, const std::vector<Fr>& evals) { return th.challenge(evals); });
  EXPECT(want.rounds == proof.rounds && want.point == proof.point && want.final_evaluations == proof.final_evaluations &&
             want.final_value == proof.final_value && th.state() == tr.state(), "prove_device == prove with the Transcript");
  // with the tail elsewhere and without it: the same proof
  for (int tail : {0, 3, 14}) {
    ListOfProducts<FIELD> again(NV);
    again.add_product({&a, &b, &c}, one);
    again.add_product({&c, &a}, k);
    Transcript<FIELD> ta(seed);
    SumcheckProof<FIELD> got = again.prove_device(ta, tail);
    EXPECT(got.rounds == proof.rounds && got.point == proof.point && got.final_evaluations == proof.final_evaluations &&
               got.final_value == proof.final_value && ta.state() == tr.state(), "the proof does not depend on tail_vars");
  }
  EXPECT(a.evaluate(proof.point) == proof.final_evaluations[0] && b.evaluate(proof.point) == proof.final_evaluations[1] &&
             c.evaluate(proof.point) == proof.final_evaluations[2], "final values == evaluate(point)");
  EXPECT(a.to_evaluations() == t[0] && b.to_evaluations() == t[1] && c.to_evaluations() == t[2], "inputs untouched");
  bool threw = false;
  try { Transcript<FIELD> t2(seed); (void)host.prove_device(t2); } catch (const Error&) { threw = true; }
  EXPECT(threw, "prove_device after rounds have been run is refused");
}

int main(int argc, char** argv) {
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 4) { std::printf("usage: sumcheck_device_check field k seed\n"); return 3; }
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
