// DenseMultilinearExtension of include/ark_hip.hpp driven from a compiled C++ program on the GPU at 13 variables over
// BLS12-381 Fr, against values the caller computed with big integers:
//   argv: value  fixed[0]  fixed[last]  relabelled_value  axpy_value  f  r_0 .. r_12      (each 64 hex digits: 4 limbs, most
//   significant first).  value = P(r); fixed = fix_variables(r_0 .. r_4); relabelled_value = P.relabel(2, 8, 3) at r with the
//   same coordinates exchanged (= value); axpy_value = (P + f Q)(r) for Q = the table reversed.
// The table is the oracle's seeded scalars (seed 43), which the caller generates the same way.
// Built and run by tests/test_gpu_cpp_mle.py (g++, links libark_hip.so and the oracle).
#include <algorithm>
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

constexpr int FIELD = ARK_HIP_BLS12_381_FR;
using M = DenseMultilinearExtension<FIELD>;

static Fr parse(const char* hex) {
  Fr r;
  const std::string s(hex);
  if (s.size() != 64) { std::printf("bad argument %s\n", hex); std::exit(3); }
  for (int i = 0; i < 4; i++) r.limbs[3 - i] = std::strtoull(s.substr(16 * i, 16).c_str(), nullptr, 16);
  return r;
}
static Fr op(int o, const Fr& a, const Fr& b) {   // the oracle's field arithmetic: 0 add, 1 sub, 2 mul
  Fr r;
  ark_oracle_field_op(FIELD, o, a.limbs.data(), b.limbs.data(), r.limbs.data(), 1);
  return r;
}

int main(int argc, char** argv) {
  constexpr size_t NV = 13, DIM = 5;
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 7 + (int)NV) { std::printf("usage: mle_check value fixed0 fixedlast relabelled axpy f r_0 .. r_12\n"); return 3; }
  const Fr value = parse(argv[1]), fixed0 = parse(argv[2]), fixedlast = parse(argv[3]), relabelled = parse(argv[4]),
           axpy = parse(argv[5]), f = parse(argv[6]);
  std::vector<Fr> r;
  for (size_t i = 0; i < NV; i++) r.push_back(parse(argv[7 + i]));
  const size_t n = (size_t)1 << NV;
  std::vector<Fr> t(n);
  ark_oracle_gen_scalars(FIELD, 43, n, 1, reinterpret_cast<uint64_t*>(t.data()));
  M p = M::from_evaluations_vec(NV, t);
  EXPECT(p.num_vars() == NV && !p.is_zero(), "num_vars, is_zero");

  // evaluate and fix_variables
  EXPECT(p.evaluate(r) == value, "evaluate against the caller's value");
  M part = p.fix_variables(std::vector<Fr>(r.begin(), r.begin() + DIM));
  EXPECT(part.num_vars() == NV - DIM, "fix_variables: num_vars");
  {
    const std::vector<Fr> e = part.to_evaluations();
    EXPECT(e.size() == n >> DIM && e.front() == fixed0 && e.back() == fixedlast, "fix_variables: both ends against the caller's values");
    // one variable with the oracle's arithmetic: out[b] = t[2b] + r (t[2b+1] - t[2b])
    const std::vector<Fr> one = p.fix_variables({r[0]}).to_evaluations();
    bool same = one.size() == n / 2;
    for (size_t b = 0; same && b < n / 2; b++) same = one[b] == op(0, t[2 * b], op(2, r[0], op(1, t[2 * b + 1], t[2 * b])));
    EXPECT(same, "fix_variables(r_0) against the oracle's arithmetic");
  }
  EXPECT(part.evaluate(std::vector<Fr>(r.begin() + DIM, r.end())) == value, "evaluate after fix_variables");
  EXPECT(p.fix_variables(r).to_evaluations()[0] == value, "fix_variables(point)[0] == evaluate(point)");
  EXPECT(p.fix_variables({}).to_evaluations() == t, "binding no variable copies");
  EXPECT(p.to_evaluations() == t, "input untouched");

  // relabel, out of place and in place
  {
    std::vector<Fr> rs = r;
    for (int i = 0; i < 3; i++) std::swap(rs[2 + i], rs[8 + i]);
    M q = p.relabel(2, 8, 3);
    EXPECT(q.evaluate(rs) == relabelled && relabelled == value, "relabel(2, 8, 3) at the point swapped the same way");
    M w = p.clone();
    w.relabel_in_place(8, 2, 3);
    EXPECT(w.to_evaluations() == q.to_evaluations(), "relabel_in_place gives the same table");
    w.relabel_in_place(2, 8, 3);
    EXPECT(w.to_evaluations() == t, "relabel twice is the identity");
    bool threw = false;
    try { p.relabel(2, 12, 3); } catch (const Error&) { threw = true; }
    EXPECT(threw, "b + k > num_vars is refused");
  }

  // the vector space
  {
    std::vector<Fr> rev(t.rbegin(), t.rend());
    M q = M::from_evaluations_vec(NV, rev);
    M acc = p.clone();
    acc.add_assign_scaled(f, q);
    EXPECT(acc.evaluate(r) == axpy, "P += (f, Q) against the caller's value");
    EXPECT((p + q * f).to_evaluations() == acc.to_evaluations(), "P + Q * f gives the same table");
    EXPECT(((p + q) - q).to_evaluations() == t, "(P + Q) - Q == P");
    EXPECT((-(-p)).to_evaluations() == t, "-(-P) == P");
    M z = M::zero();
    EXPECT(z.is_zero() && (p * Fr{}).is_zero(), "zero(), P * 0");
    EXPECT((p + z).to_evaluations() == t && (z + p).to_evaluations() == t, "adding the zero polynomial copies the other operand");
    bool threw = false;
    try { (void)(p + part); } catch (const Error&) { threw = true; }
    EXPECT(threw, "unequal num_vars is refused");
    M c = M::concat({&p, &q});
    EXPECT(c.num_vars() == NV + 1, "concat: num_vars");
    std::vector<Fr> r2 = r;
    Fr one{};
    ark_oracle_field_const(FIELD, 1, one.limbs.data());
    r2.push_back(f);   // (1 - f) P(r) + f Q(r)
    EXPECT(c.evaluate(r2) == op(0, op(2, op(1, one, f), value), op(2, f, q.evaluate(r))), "concat: (1 - x) P + x Q");
  }
  ark_hip_shutdown();
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
