// The prefix scans of include/ark_hip.hpp's DeviceVec (prefix_product, prefix_sum, prefix_ratio) driven from a compiled C++
// program on the GPU over BLS12-381 Fr, against vectors the caller computed with big integers:
//   argv: n dir      dir holds a.bin, b.bin (n elements each) and product.bin, sum_exclusive.bin, ratio.bin (n + 1 elements
//                    each: the expected vector, then the expected total / last); elements are 4 little-endian u64 limbs
// Built and run by tests/test_gpu_cpp_prefix_scan.py (g++, links libark_hip.so).
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

static std::vector<Fr> read(const std::string& path, size_t count) {
  std::vector<Fr> v(count);
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f || std::fread(v.data(), 32, count, f) != count) { std::printf("cannot read %s\n", path.c_str()); std::exit(3); }
  std::fclose(f);
  return v;
}

int main(int argc, char** argv) {
  static_assert(sizeof(Fr) == 32, "an element is four u64 limbs");
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 3) { std::printf("usage: prefix_scan_check n dir\n"); return 3; }
  const size_t n = std::strtoull(argv[1], nullptr, 10);
  const std::string dir = std::string(argv[2]) + "/";
  const std::vector<Fr> a = read(dir + "a.bin", n), b = read(dir + "b.bin", n);
  std::vector<Fr> product = read(dir + "product.bin", n + 1), sum = read(dir + "sum_exclusive.bin", n + 1),
                  ratio = read(dir + "ratio.bin", n + 1);
  const Fr product_total = product.back(), sum_total = sum.back(), ratio_last = ratio.back();
  product.pop_back();
  sum.pop_back();
  ratio.pop_back();
  int tile = 0, levels = 0;
  EXPECT(ark_hip_prefix_scan_plan(0, n, &tile, &levels) == 0 && n == (size_t)tile + 1 && levels == 2, "the caller chose tile + 1 elements");

  V da = V::from_vec(a), db = V::from_vec(b);
  {
    auto r = da.prefix_product();
    EXPECT(r.first.len() == n && r.first.to_vec() == product, "prefix_product: the vector");
    EXPECT(r.second == product_total, "prefix_product: the total");
  }
  {
    auto r = da.prefix_sum(true);
    EXPECT(r.first.len() == n && r.first.to_vec() == sum, "prefix_sum (exclusive): the vector");
    EXPECT(r.second == sum_total, "prefix_sum: the total");
  }
  {
    auto r = da.prefix_ratio(db);
    EXPECT(r.first.len() == n && r.first.to_vec() == ratio, "prefix_ratio: the vector");
    EXPECT(r.second == ratio_last, "prefix_ratio: the last value");
  }
  EXPECT(da.to_vec() == a && db.to_vec() == b, "inputs untouched");
  {
    bool threw = false;
    try { da.prefix_ratio(V(n + 1)); } catch (const Error&) { threw = true; }
    EXPECT(threw, "prefix_ratio refuses vectors of different lengths");
  }
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
