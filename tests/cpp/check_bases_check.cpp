// check_bases / check_bases_device of include/ark_hip.hpp on BLS12-381 G1 (run on the GPU by tests/test_gpu_check_bases.py).
// argv[1]: a file of  u64 n | u64 first_bad, not_reduced, off_curve, off_subgroup | n Affine points | n expected status bytes.
#include <cstdio>
#include <cstring>
#include <vector>
#include "ark_hip.hpp"

using namespace ark_hip;
using Curve = Bls12_381G1;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static bool same(const BaseCheck& r, const uint64_t* want) {
  return r.first_bad == want[0] && r.not_reduced == want[1] && r.off_curve == want[2] && r.off_subgroup == want[3] &&
         r.ok == (want[1] + want[2] + want[3] == 0);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t head[5];
  if (std::fread(head, 8, 5, f) != 5) return 2;
  const size_t n = head[0];
  std::vector<Curve::AffineT> pts(n);
  std::vector<uint8_t> want(n);
  if (std::fread(pts.data(), sizeof(Curve::AffineT), n, f) != n || std::fread(want.data(), 1, n, f) != n) return 2;
  std::fclose(f);
  try {
    const std::vector<Curve::AffineT> before = pts;
    for (CheckMethod m : {CheckMethod::Auto, CheckMethod::Ladder, CheckMethod::Endomorphism}) {
      BaseCheck r = check_bases<Curve>(pts, true, m, true);
      EXPECT(same(r, head + 1));
      EXPECT(r.status == want);
      EXPECT(same(check_bases<Curve>(pts, true, m), head + 1));
    }
    EXPECT(std::memcmp(before.data(), pts.data(), n * sizeof(Curve::AffineT)) == 0);
    // the device form, status bytes in device memory
    void *d_pts = nullptr, *d_st = nullptr;
    check(ark_hip_malloc(n * sizeof(Curve::AffineT), &d_pts), "ark_hip_malloc");
    check(ark_hip_malloc(n, &d_st), "ark_hip_malloc");
    check(ark_hip_memcpy_h2d(d_pts, pts.data(), n * sizeof(Curve::AffineT)), "ark_hip_memcpy_h2d");
    EXPECT(same(check_bases_device<Curve>(d_pts, n, true, CheckMethod::Auto, d_st), head + 1));
    std::vector<uint8_t> got(n);
    check(ark_hip_memcpy_d2h(got.data(), d_st, n), "ark_hip_memcpy_d2h");
    EXPECT(got == want);
    EXPECT(same(check_bases_device<Curve>(d_pts, n), head + 1));
    // without the subgroup test nothing has status 3, and a valid prefix passes
    BaseCheck c1 = check_bases<Curve>(pts, false, CheckMethod::Auto, true);
    EXPECT(c1.off_subgroup == 0 && c1.not_reduced == head[2] && c1.off_curve == head[3]);
    BaseCheck ok = check_bases<Curve>(pts.data() + n - 1 - 20, 10);   // points 279..288: chain points
    EXPECT(ok.ok && ok.first_bad == 10);
    // method 2 belongs to BLS12-381 G1 alone
    bool threw = false;
    try {
      (void)check_bases_device<Bn254G1>(d_pts, 1, true, CheckMethod::Endomorphism);
    } catch (const Error& e) {
      threw = e.code == ARK_HIP_ERR_ARG;
    }
    EXPECT(threw);
    check(ark_hip_free(d_pts), "ark_hip_free");
    check(ark_hip_free(d_st), "ark_hip_free");
  } catch (const Error& e) {
    std::printf("ark_hip error %d in %s\n", e.code, e.what());
    return 1;
  }
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
