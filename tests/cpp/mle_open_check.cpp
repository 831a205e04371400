// eq, quotients and open of DenseMultilinearExtension (include/ark_hip.hpp) driven from a compiled C++ program on the GPU at 9
// variables, on each scalar field with its G1, against values the caller computed with big integers and against the oracle:
//   argv: field (bn254 | bls12_381 | bls12_377)  value  eq_first  eq_last  scale  r_0 .. r_8     (each 64 hex digits: 4 limbs,
//   most significant first).  value = P(r); eq_first, eq_last = the two ends of scale * eq(r, .).
// The table is the oracle's seeded scalars (seed 47), which the caller generates the same way; the bases are the oracle's
// synthetic ones, and every commitment is compared with the oracle's own MSM over the same quotient.
// Built and run by tests/test_gpu_cpp_mle_open.py (g++, links libark_hip.so and the oracle).
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

template <class Curve>
static void run(char** argv) {
  constexpr int FIELD = Curve::SCALAR_FIELD;
  constexpr size_t NV = 9;
  using M = DenseMultilinearExtension<FIELD>;
  using A = Affine<Curve::WORDS>;
  auto op = [](int o, const Fr& a, const Fr& b) {   // the oracle's field arithmetic: 0 add, 1 sub, 2 mul
    Fr r;
    ark_oracle_field_op(FIELD, o, a.limbs.data(), b.limbs.data(), r.limbs.data(), 1);
    return r;
  };
  const Fr value = parse(argv[2]), eq_first = parse(argv[3]), eq_last = parse(argv[4]), scale = parse(argv[5]);
  std::vector<Fr> r;
  for (size_t i = 0; i < NV; i++) r.push_back(parse(argv[6 + i]));
  const size_t n = (size_t)1 << NV;
  std::vector<Fr> t(n);
  ark_oracle_gen_scalars(FIELD, 47, n, 1, reinterpret_cast<uint64_t*>(t.data()));
  M p = M::from_evaluations_vec(NV, t);

  // eq: both ends against the caller, the sum and the inner product with the oracle's arithmetic
  {
    M e = M::eq(r, &scale);
    EXPECT(e.num_vars() == NV, "eq: num_vars");
    const std::vector<Fr> ev = e.to_evaluations();
    EXPECT(ev.size() == n && ev.front() == eq_first && ev.back() == eq_last, "eq: both ends against the caller's values");
    Fr sum{}, dot{};
    for (size_t b = 0; b < n; b++) { sum = op(0, sum, ev[b]); dot = op(0, dot, op(2, ev[b], t[b])); }
    EXPECT(sum == scale, "eq: the table sums to the scale");
    EXPECT(dot == op(2, scale, value), "eq: <eq(r), P> = scale P(r)");
    Fr one{};
    ark_oracle_field_const(FIELD, 1, one.limbs.data());
    M u = M::eq(r);
    const std::vector<Fr> uv = u.to_evaluations();
    bool same = true;
    for (size_t b = 0; same && b < n; b++) same = op(2, uv[b], scale) == ev[b];
    EXPECT(same, "eq without a scale, times the scale");
    EXPECT(M::eq({}, &scale).to_evaluations() == std::vector<Fr>{scale} && M::eq({}).to_evaluations() == std::vector<Fr>{one},
           "eq of no variables");
  }

  // quotients: every element with the oracle's arithmetic, the value against the caller's and against evaluate
  typename M::Quotients q = p.quotients(r);
  EXPECT(q.value == value && q.value == p.evaluate(r), "quotients: the value");
  {
    std::vector<Fr> f = t;
    size_t at = 0;
    bool same = true;
    for (size_t i = 0; i < NV; i++) {
      EXPECT(q.segment_offset(i) == at && q.segment_len(i) == f.size() / 2, "quotients: the segments tile the vector");
      const std::vector<Fr> seg = q.segment_to_vec(i);
      std::vector<Fr> next(f.size() / 2);
      for (size_t b = 0; b < next.size(); b++) {
        const Fr d = op(1, f[2 * b + 1], f[2 * b]);
        same = same && seg[b] == d;
        next[b] = op(0, f[2 * b], op(2, r[i], d));
      }
      at += seg.size();
      f = next;
    }
    EXPECT(same, "quotients: every element against the oracle's arithmetic");
    EXPECT(at == n - 1 && q.all.len() == n - 1 && f[0] == value, "quotients: 2^nv - 1 elements");
    EXPECT(p.to_evaluations() == t, "input untouched");
    bool threw = false;
    try { p.quotients(std::vector<Fr>(r.begin(), r.begin() + 3)); } catch (const Error&) { threw = true; }
    EXPECT(threw, "a point of another length is refused");
  }

  // open: level i's bases are the slice of one base array that q_i is of the quotient vector
  {
    const uint64_t a4[4] = {0xA11CE, 1, 2, 0}, b4[4] = {0xB0B, 3, 0, 0};
    std::vector<A> bases(n);
    ark_oracle_gen_bases(Curve::ID, a4, b4, n, reinterpret_cast<uint64_t*>(bases.data()));
    void* d_bases = nullptr;
    check(ark_hip_malloc(n * sizeof(A), &d_bases), "ark_hip_malloc");
    check(ark_hip_memcpy_h2d(d_bases, bases.data(), n * sizeof(A)), "ark_hip_memcpy_h2d");
    std::vector<const void*> levels;
    for (size_t i = 0; i < NV; i++) levels.push_back((const char*)d_bases + q.segment_offset(i) * sizeof(A));
    auto opened = p.template open<Curve>(r, levels);
    EXPECT(opened.first == value && opened.second.size() == NV, "open: the value");
    bool same = opened.second.size() == NV;
    for (size_t i = 0; same && i < NV; i++) {
      const std::vector<Fr> seg = q.segment_to_vec(i);
      Projective<Curve::WORDS> ref;
      ark_oracle_msm_fr(Curve::ID, reinterpret_cast<const uint64_t*>(bases.data() + q.segment_offset(i)),
                        reinterpret_cast<const uint64_t*>(seg.data()), seg.size(), 0, 1, reinterpret_cast<uint64_t*>(&ref));
      A ref_aff, got_aff;
      ark_oracle_to_affine(Curve::ID, reinterpret_cast<const uint64_t*>(&ref), reinterpret_cast<uint64_t*>(&ref_aff), 1);
      ark_oracle_to_affine(Curve::ID, reinterpret_cast<const uint64_t*>(&opened.second[i]), reinterpret_cast<uint64_t*>(&got_aff), 1);
      same = std::memcmp(&ref_aff, &got_aff, sizeof(A)) == 0;
    }
    EXPECT(same, "open: every level's point against the oracle's MSM");
    bool threw = false;
    try { levels.pop_back(); p.template open<Curve>(r, levels); } catch (const Error&) { threw = true; }
    EXPECT(threw, "one base array per variable");
    check(ark_hip_free(d_bases), "ark_hip_free");
  }
}

int main(int argc, char** argv) {
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 6 + 9) { std::printf("usage: mle_open_check field value eq_first eq_last scale r_0 .. r_8\n"); return 3; }
  const std::string f(argv[1]);
  if (f == "bn254") run<Bn254G1>(argv);
  else if (f == "bls12_381") run<Bls12_381G1>(argv);
  else if (f == "bls12_377") run<Bls12_377G1>(argv);
  else { std::printf("unknown field %s\n", argv[1]); return 3; }
  ark_hip_shutdown();
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
