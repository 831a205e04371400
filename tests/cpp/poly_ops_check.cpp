// The polynomial operations of include/ark_hip.hpp's DeviceVec / Radix2EvaluationDomain (evaluate, divide_by_linear,
// divide_by_vanishing_poly, evaluate_all_lagrange_coefficients, inner_product) driven from a compiled C++ program on the GPU
// at 2^16 over BLS12-381 Fr.  Checked by the identity p = q (x - z) + r at a random point s, by the oracle's field
// arithmetic, and against values the caller computed with big integers:
//   argv: z s tau p(z) p(s) p(tau) L_0(tau) L_{n-1}(tau)        (each 64 hex digits: 4 limbs, most significant first)
// The coefficients are the oracle's seeded scalars (seed 41), which the caller generates the same way.
// Built and run by tests/test_gpu_cpp_poly_ops.py (g++, links libark_hip.so and the oracle).
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

constexpr int FIELD = ARK_HIP_BLS12_381_FR;
using V = DeviceVec<FIELD>;
using D = Radix2EvaluationDomain<FIELD>;

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
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 9) { std::printf("usage: poly_ops_check z s tau p(z) p(s) p(tau) L0 Llast\n"); return 3; }
  const Fr z = parse(argv[1]), s = parse(argv[2]), tau = parse(argv[3]), pz = parse(argv[4]), ps = parse(argv[5]),
           ptau = parse(argv[6]), l0 = parse(argv[7]), llast = parse(argv[8]);
  const size_t n = (size_t)1 << 16;
  std::vector<Fr> p(n);
  ark_oracle_gen_scalars(FIELD, 41, n, 1, reinterpret_cast<uint64_t*>(p.data()));
  V dp = V::from_vec(p);

  // evaluate
  EXPECT(dp.evaluate(z) == pz, "evaluate(z) against the caller's value");
  EXPECT(dp.evaluate(s) == ps, "evaluate(s) against the caller's value");

  // divide_by_linear: remainder = p(z); p(s) = q(s) (s - z) + r; quotient against the recurrence on the host
  auto qr = dp.divide_by_linear(z);
  EXPECT(qr.first.len() == n - 1, "quotient length");
  EXPECT(qr.second == pz, "remainder = p(z)");
  EXPECT(op(0, op(2, qr.first.evaluate(s), op(1, s, z)), qr.second) == ps, "p(s) = q(s) (s - z) + r");
  {
    const std::vector<Fr> q = qr.first.to_vec();
    Fr acc{};   // s[i + 1], from the top
    bool same = true;
    for (size_t i = n - 1; i-- > 0;) {
      acc = op(0, p[i + 1], op(2, z, acc));
      if (!(q[i] == acc)) { same = false; break; }
    }
    EXPECT(same, "quotient coefficients against synthetic division with the oracle's arithmetic");
  }
  EXPECT(dp.to_vec() == p, "input untouched out of place");
  {
    V w = dp.clone();
    const Fr rem = w.divide_by_linear_in_place(z);
    EXPECT(rem == pz && w.len() == n - 1, "in place: remainder and length");
    EXPECT(w.to_vec() == qr.first.to_vec(), "in place: the same quotient");
  }

  // divide_by_vanishing_poly: p = q (x^m - 1) + r at the point s, m = 2^12
  {
    auto dom = D::new_((size_t)1 << 12);
    auto vr = dp.divide_by_vanishing_poly(*dom);
    EXPECT(vr.first.len() == n - dom->size() && vr.second.len() == dom->size(), "vanishing: lengths");
    Fr sm = s;
    for (int i = 0; i < 12; i++) sm = op(2, sm, sm);   // s^m
    Fr one{};
    ark_oracle_field_const(FIELD, 1, one.limbs.data());
    EXPECT(op(0, op(2, vr.first.evaluate(s), op(1, sm, one)), vr.second.evaluate(s)) == ps, "p(s) = q(s) (s^m - 1) + r(s)");
  }

  // Lagrange coefficients over the size-n domain and its coset: the two ends against the caller's values (plain domain),
  // sum_i L_i = 1, and sum_i L_i(tau) P(h g^i) = P(tau) with everything on the device
  {
    auto base = D::new_(n);
    Fr gen{}, one{};   // the field's multiplicative generator as coset offset (poly/benches/fft.rs:107)
    ark_oracle_field_const(FIELD, 3, gen.limbs.data());
    ark_oracle_field_const(FIELD, 1, one.limbs.data());
    for (int coset = 0; coset < 2; coset++) {
      const D dom = coset ? *base->get_coset(gen) : *base;
      V lag = dom.evaluate_all_lagrange_coefficients(tau);
      EXPECT(lag.len() == n, "lagrange: length");
      if (!coset) {
        const std::vector<Fr> l = lag.to_vec();
        EXPECT(l[0] == l0 && l[n - 1] == llast, "lagrange: L_0 and L_{n-1} against the caller's values");
      }
      std::vector<Fr> ones(n, one);
      EXPECT(lag.inner_product(V::from_vec(ones)) == one, "lagrange: the coefficients sum to one");
      auto ev = evaluate_over_domain(dp.clone(), dom);
      EXPECT(lag.inner_product(ev.evals) == ptau, "lagrange: <L(tau), evaluations> = p(tau)");
    }
    // tau in the domain: one-hot
    V hot = base->evaluate_all_lagrange_coefficients(base->group_gen());
    const std::vector<Fr> h = hot.to_vec();
    bool ok = h[1] == one;
    for (size_t i = 0; i < n; i++)
      if (i != 1 && !h[i].is_zero()) ok = false;
    EXPECT(ok, "lagrange: tau = g gives the unit vector e_1");
  }
  ark_hip_shutdown();
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
