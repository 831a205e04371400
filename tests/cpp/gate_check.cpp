// SumOfProducts and DeviceVec::rotate of include/ark_hip.hpp driven from a compiled C++ program on the GPU over BLS12-381 Fr,
// against vectors the caller computed with big integers, for the one mixed expression
//   c0 + k a[i] b[i+4] a[i] + c[i-1] + k b[i+R] c[i]        (R = INT64_MIN)
//   argv: dir   which holds dims.bin (n as u64), a.bin, b.bin, c.bin (n elements each), k.bin and c0.bin (one element), want.bin
//               (the expression with c0), plain.bin (without it) and rot.bin (a rotated by -3); elements are 4 little-endian
//               u64 limbs
// Built and run by tests/test_gpu_cpp_gate.py (g++, links libark_hip.so).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ark_hip.hpp"
using namespace ark_hip;

static int fails = 0;
#define EXPECT(c, msg) do { if (!(c)) { std::printf("FAIL: %s\n", msg); fails++; } } while (0)

constexpr int FIELD = ARK_HIP_BLS12_381_FR;
using V = DeviceVec<FIELD>;
using S = SumOfProducts<FIELD>;

template <class T>
static std::vector<T> read(const std::string& path, size_t count) {
  std::vector<T> v(count);
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f || std::fread(v.data(), sizeof(T), count, f) != count) { std::printf("cannot read %s\n", path.c_str()); std::exit(3); }
  std::fclose(f);
  return v;
}

int main(int argc, char** argv) {
  static_assert(sizeof(Fr) == 32, "an element is four u64 limbs");
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc < 2) { std::printf("usage: gate_check dir\n"); return 3; }
  const std::string at = std::string(argv[1]) + "/";
  const size_t n = read<uint64_t>(at + "dims.bin", 1)[0];
  const std::vector<Fr> a = read<Fr>(at + "a.bin", n), b = read<Fr>(at + "b.bin", n), c = read<Fr>(at + "c.bin", n);
  const Fr k = read<Fr>(at + "k.bin", 1)[0], c0 = read<Fr>(at + "c0.bin", 1)[0];
  const std::vector<Fr> want = read<Fr>(at + "want.bin", n), plain = read<Fr>(at + "plain.bin", n), rot = read<Fr>(at + "rot.bin", n);

  const SumOfProductsPlan p = sum_of_products_plan(n);
  EXPECT(p.blocks > 0 && p.rows_per_lane == 1 && (size_t)p.blocks * 256 >= n, "the plan");
  V da = V::from_vec(a), db = V::from_vec(b), dc = V::from_vec(c);
  S s(n);
  s.add_product({{da}, {db, 4}, {da}}, &k);
  s.add_product({{dc, -1}});
  s.add_product({{db, INT64_MIN}, {&dc}}, &k);
  EXPECT(s.num_columns() == 3 && s.num_products() == 3 && s.len() == n, "columns are shared by pointer");
  EXPECT(s.evaluate().to_vec() == plain, "without a constant");
  s.set_constant(c0);
  EXPECT(s.evaluate().to_vec() == want, "with a constant");
  V out = V::from_vec(b);   // garbage of the right length: overwritten in full
  s.evaluate(out);
  EXPECT(out.to_vec() == want, "into a given vector");
  EXPECT(da.to_vec() == a && db.to_vec() == b && dc.to_vec() == c, "inputs untouched");
  s.clear_constant();
  s.evaluate(da);           // a is read at rotation 0 only: in place
  EXPECT(da.to_vec() == plain, "in place");
  da = V::from_vec(a);
  EXPECT(da.rotate(-3).to_vec() == rot, "rotate");
  EXPECT(da.rotate((int64_t)n).to_vec() == a && da.rotate(0).to_vec() == a, "rotate by a multiple of the length");
  {
    bool threw = false;
    try { da.rotate(1, da); } catch (const Error&) { threw = true; }
    EXPECT(threw, "a rotated copy has no in-place form");
    threw = false;
    try { S t(n); t.add_product({{da, 2}, {db}}); t.evaluate(da); } catch (const Error&) { threw = true; }
    EXPECT(threw, "evaluate refuses an output that a factor reads at a rotation");
    threw = false;
    try { S t(n); t.add_product({{V(n + 1)}}); } catch (const Error&) { threw = true; }
    EXPECT(threw, "add_product refuses a column of the wrong length");
    threw = false;
    try { S t(n); t.add_product(std::vector<S::Factor>(9, S::Factor(da))); } catch (const Error&) { threw = true; }
    EXPECT(threw, "add_product refuses nine factors");
    threw = false;
    try { S t(n); t.evaluate(); } catch (const Error&) { threw = true; }
    EXPECT(threw, "evaluate refuses an empty expression");
  }
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
