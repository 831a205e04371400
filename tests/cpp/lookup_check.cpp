// lookup and lookup_plan of the C++ mirror (include/ark_hip.hpp) driven from a compiled C++ program on the GPU: a single-column
// lookup of 2^9 witness cells in a table of 2^6 values over BLS12-381 Fr, end to end without an index array.
//   argv: FILE  P_t  Q_t     (the roots: 64 hex digits each, 4 limbs, most significant first)
//   FILE: one token per line -- gamma, a value outside the table, the 64 table values (Montgomery elements as 64 hex digits),
//         then the 512 indices (decimal) that say which table value each witness cell holds.
// m comes from lookup(t, w); the denominators gamma + t_j and gamma + w_i from linear_combination; the roots of the two fraction
// trees satisfy P_w Q_t = P_t Q_w; with one witness cell moved outside the table, missing == 1 and the identity fails.  Indices
// and counts are compared with a join on the host, the root of the table side with the caller's big-integer values, products
// with the oracle's field arithmetic.
// Built and run by tests/test_gpu_cpp_lookup.py (g++, links libark_hip.so and the oracle).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>
#include "ark_hip.hpp"
extern "C" {
#include "ark_oracle.h"
}
using namespace ark_hip;

static int fails = 0;
#define EXPECT(c, msg) do { if (!(c)) { std::printf("FAIL: %s\n", msg); fails++; } } while (0)

static Fr parse(const std::string& s) {
  Fr r;
  if (s.size() != 64) { std::printf("bad element %s\n", s.c_str()); std::exit(3); }
  for (int i = 0; i < 4; i++) r.limbs[3 - i] = std::strtoull(s.substr(16 * i, 16).c_str(), nullptr, 16);
  return r;
}

static void run(char** argv) {
  constexpr int FIELD = ARK_HIP_BLS12_381_FR;
  using M = DenseMultilinearExtension<FIELD>;
  using Vec = DeviceVec<FIELD>;
  auto op = [](int o, const Fr& a, const Fr& b) {   // the oracle's field arithmetic: 0 add, 1 sub, 2 mul
    Fr r;
    ark_oracle_field_op(FIELD, o, a.limbs.data(), b.limbs.data(), r.limbs.data(), 1);
    return r;
  };
  std::ifstream in(argv[1]);
  std::string tok;
  in >> tok;
  const Fr gamma = parse(tok);
  in >> tok;
  const Fr outside = parse(tok);
  std::vector<Fr> t(64), w(512);
  std::vector<uint32_t> idx(512);
  for (auto& x : t) { in >> tok; x = parse(tok); }
  for (size_t i = 0; i < 512; i++) { in >> idx[i]; w[i] = t[idx[i] % 64]; }
  if (!in) { std::printf("short input file\n"); std::exit(3); }
  const Fr Pt = parse(argv[2]), Qt = parse(argv[3]);
  const Fr one = M::eq({}).to_evaluations()[0];

  const std::pair<unsigned, size_t> plan = M::lookup_plan(64);
  EXPECT(plan.first == 7 && plan.second >= (size_t)4 << 7, "plan: 2^7 slots for 64 values");
  M tm = M::from_evaluations_vec(6, t);
  M tden = M::linear_combination({&tm}, {one}, &gamma);
  for (int altered = 0; altered < 2; altered++) {
    if (altered) w[77] = outside;
    M wm = M::from_evaluations_vec(9, w);
    typename M::Lookup lk = M::lookup(tm.evaluations(), wm.evaluations(), true);
    // the join on the host: first occurrences (the table's values are distinct here) and counts
    std::map<std::array<uint64_t, 4>, uint32_t> first;
    for (uint32_t j = 0; j < 64; j++) first.emplace(t[j].limbs, j);
    std::vector<uint64_t> want(64, 0);
    uint64_t missing = 0;
    bool same = lk.indices.size() == 512;
    for (size_t i = 0; same && i < 512; i++) {
      auto it = first.find(w[i].limbs);
      const uint32_t k = it == first.end() ? ARK_HIP_LOOKUP_MISSING : it->second;
      same = lk.indices[i] == k;
      if (k == ARK_HIP_LOOKUP_MISSING) missing++; else want[k]++;
    }
    EXPECT(same, "lookup: every index against the host's join");
    EXPECT(lk.missing == missing && missing == (uint64_t)altered, "lookup: the number of cells that are not in the table");
    if (altered) EXPECT(lk.indices[77] == ARK_HIP_LOOKUP_MISSING, "lookup: the moved cell is reported missing");
    const std::vector<Fr> got = lk.mult.to_vec();
    same = got.size() == 64;
    for (size_t j = 0; same && j < 64; j++) {
      Fr c = Fr{}, acc = one;                          // want[j] times one, by doubling and adding
      for (uint64_t b = want[j]; b; b >>= 1, acc = op(0, acc, acc))
        if (b & 1) c = op(0, c, acc);
      same = got[j] == c;
    }
    EXPECT(same, "lookup: every count against the host's join");
    M m = M::from_evaluations_vec(6, got);
    typename M::FractionTree tt = tden.fraction_tree(&m);
    M wden = M::linear_combination({&wm}, {one}, &gamma);
    typename M::FractionTree wt = wden.fraction_tree(nullptr);
    if (!altered) EXPECT(tt.root_num == Pt && tt.root_den == Qt, "table side: the root against the caller's values");
    const bool balanced = op(2, wt.root_num, tt.root_den) == op(2, tt.root_num, wt.root_den);
    EXPECT(balanced == !altered, "P_w Q_t = P_t Q_w exactly when every witness cell is in the table");
    EXPECT(tm.to_evaluations() == t && wm.to_evaluations() == w, "lookup: inputs untouched");
  }
}

int main(int argc, char** argv) {
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 4) { std::printf("usage: lookup_check FILE P_t Q_t\n"); return 3; }
  run(argv);
  ark_hip_shutdown();
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
