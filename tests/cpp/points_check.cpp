// DevicePoints<Curve> and sw_mul of include/ark_hip.hpp on BLS12-381 G1 (run on the GPU by tests/test_gpu_cpp_points.py).
// argv[1]: a file of  u64 n | Fr a | Fr b | n Affine P | n Affine Q | n Fr k (Montgomery) | n Affine [k_i] P_i |
//                     n Affine [a][k_i] P_i + [b] Q_i | n Affine [a] P_i   -- the expected values are the oracle's.
#include <cstdio>
#include <cstring>
#include <vector>
#include "ark_hip.hpp"

using namespace ark_hip;
using Curve = Bls12_381G1;
using Aff = Curve::AffineT;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(T), n, f) == n;
}
static std::vector<Aff> affine_of(const std::vector<Curve::ProjectiveT>& jac) {
  std::vector<Aff> out(jac.size());
  check(ark_hip_sw_into_affine(Curve::ID, reinterpret_cast<const uint64_t*>(jac.data()), jac.size(), reinterpret_cast<uint64_t*>(out.data())),
        "ark_hip_sw_into_affine");
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t n64;
  Fr a, b;
  if (std::fread(&n64, 8, 1, f) != 1 || std::fread(&a, sizeof(Fr), 1, f) != 1 || std::fread(&b, sizeof(Fr), 1, f) != 1) return 2;
  const size_t n = n64;
  std::vector<Aff> P, Q, want_mul, want_fold, want_shared;
  std::vector<Fr> k;
  if (!read_n(f, P, n) || !read_n(f, Q, n) || !read_n(f, k, n) || !read_n(f, want_mul, n) || !read_n(f, want_fold, n) ||
      !read_n(f, want_shared, n))
    return 2;
  std::fclose(f);
  try {
    auto scalars = DeviceVec<Curve::SCALAR_FIELD>::from_vec(k);
    DevicePoints<Curve> v = DevicePoints<Curve>::from_affine(P);
    EXPECT(v.len() == n);
    EXPECT(affine_of(v.to_vec()) == P);                         // from_affine converts, the group elements stay
    v.mul_assign(scalars);
    EXPECT(v.normalize_to_vec() == want_mul);
    EXPECT(affine_of(v.to_vec()) == want_mul);
    DevicePoints<Curve> w = v.clone();
    DevicePoints<Curve> hi = DevicePoints<Curve>::from_affine(Q);
    DevicePoints<Curve> folded = v.fold(hi, a, b);
    EXPECT(folded.normalize_to_vec() == want_fold);
    EXPECT(v.normalize_to_vec() == want_mul);                   // fold leaves its inputs alone
    w += hi;
    w -= hi;
    EXPECT(w.normalize_to_vec() == want_mul);
    w -= v;                                                     // X - X: the identity everywhere
    for (const Aff& p : w.normalize_to_vec()) EXPECT(p.is_zero());
    DevicePoints<Curve> s = DevicePoints<Curve>::from_affine(P);
    s.mul_assign(a);
    EXPECT(s.normalize_to_vec() == want_shared);
    // host slices through the staged entry: one scalar per point, and one for all
    EXPECT(affine_of(sw_mul<Curve>(P, k)) == want_mul);
    EXPECT(affine_of(sw_mul<Curve>(P, std::vector<Fr>{a})) == want_shared);
    DevicePoints<Curve> moved = std::move(folded);
    EXPECT(moved.len() == n && folded.len() == 0);
    DevicePoints<Curve> empty = DevicePoints<Curve>::from_affine({});
    empty.mul_assign(a);
    EXPECT(empty.to_vec().empty() && empty.normalize_to_vec().empty());
    bool threw = false;
    try {
      v += empty;
    } catch (const Error& e) {
      threw = e.code == ARK_HIP_ERR_ARG;
    }
    EXPECT(threw);
  } catch (const Error& e) {
    std::printf("ark_hip error %d in %s\n", e.code, e.what());
    return 1;
  }
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
