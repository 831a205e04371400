// The extension-field and FRI classes of include/ark_hip.hpp from a plain C++ program on the GPU (tests/test_gpu_cpp_fri.py):
// one commit phase per line of the vectors file, its roots and final polynomial printed for the test to compare with the model,
// a few queries verified here.  The challenge of a layer is word k of its root modulo p: the test's model uses the same rule.
//   line: sfield log_n log_arity num_folds offset   then d * n stored words of layer 0, component by component
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>
#include "ark_hip.hpp"

using namespace ark_hip;

template <int S>
struct RootChallenger : FriProver<S>::Challenger {
  uint64_t p = small_field_info<S>().p;
  ExtElement next_beta(const Digest& root) override {
    ExtElement b{};
    for (unsigned k = 0; k < small_ext_degree<S>(); k++) {
      uint64_t w = 0;
      for (int i = 7; i >= 0; i--) w = (w << 8) | root[8 * k + i];
      b[k] = w % p;
    }
    return b;
  }
};

template <int S>
int run(std::istream& in, unsigned log_n, unsigned a, unsigned folds, uint64_t offset) {
  using Word = typename SmallWord<S>::type;
  constexpr unsigned D = small_ext_degree<S>();
  const size_t n = (size_t)1 << log_n;
  std::vector<std::vector<Word>> comps(D, std::vector<Word>(n));
  for (auto& c : comps)
    for (auto& w : c) {
      uint64_t v;
      in >> v;
      w = (Word)v;
    }
  auto dom = SmallRadix2EvaluationDomain<S>::create(n)->get_coset(offset);
  auto layer0 = SmallExtVec<S>::from_components(comps);
  // the pointwise mirror: (f * f) * f^-1 = f wherever f != 0, through mul_const by one
  {
    auto t = SmallExtVec<S>::from_components(comps);
    auto inv = SmallExtVec<S>::from_components(comps);
    inv.batch_inverse();
    t *= layer0;
    t *= inv;
    t.mul_const(ExtElement{small_field_info<S>().r, 0, 0, 0});
    if (t.data().to_vec() != layer0.data().to_vec()) {
      std::printf("pointwise mismatch\n");
      return 1;
    }
  }
  FriProver<S> prover(layer0, *dom, a, folds);
  RootChallenger<S> ch;
  prover.commit_phase(ch);
  std::printf("roots");
  for (const Digest& r : prover.roots()) {
    std::printf(" ");
    for (uint8_t b : r) std::printf("%02x", b);
  }
  std::printf("\nfinal");
  for (Word w : prover.final_poly()) std::printf(" %llu", (unsigned long long)w);
  std::printf("\n");
  // queries
  const std::vector<uint64_t> indices = {0, n - 1, n / 2 + 1, 12345 % n};
  const auto openings = prover.query(indices);
  for (size_t q = 0; q < indices.size(); q++) {
    std::vector<std::vector<Word>> rows;
    std::vector<std::vector<uint8_t>> paths;
    for (unsigned l = 0; l < folds; l++) {
      const FriLayer& lay = prover.plan().layers[l];
      const size_t count = (size_t)D << lay.log_arity, plen = (size_t)(lay.log_size - lay.log_arity) * 32;
      const Word* r = (const Word*)openings[l].rows.data() + q * count;
      rows.emplace_back(r, r + count);
      paths.emplace_back(openings[l].paths.begin() + q * plen, openings[l].paths.begin() + (q + 1) * plen);
    }
    if (!fri_verify_query<S>(dom->raw(), a, prover.roots(), prover.betas(), prover.final_poly(), indices[q], rows, paths)) {
      std::printf("query %zu rejected\n", q);
      return 1;
    }
    rows[0][1] ^= 1;
    if (fri_verify_query<S>(dom->raw(), a, prover.roots(), prover.betas(), prover.final_poly(), indices[q], rows, paths)) {
      std::printf("tampered query %zu accepted\n", q);
      return 1;
    }
  }
  std::printf("verify ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (ark_hip_device_count() <= 0) return 2;
  std::ifstream in(argv[1]);
  int sfield;
  unsigned log_n, a, folds;
  uint64_t offset;
  try {
    while (in >> sfield >> log_n >> a >> folds >> offset) {
      int rc = sfield == ARK_HIP_SFP_GOLDILOCKS ? run<ARK_HIP_SFP_GOLDILOCKS>(in, log_n, a, folds, offset)
               : sfield == ARK_HIP_SFP_BABYBEAR ? run<ARK_HIP_SFP_BABYBEAR>(in, log_n, a, folds, offset)
                                                : run<ARK_HIP_SFP_KOALABEAR>(in, log_n, a, folds, offset);
      if (rc) return rc;
    }
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  std::printf("all ok\n");
  return 0;
}
