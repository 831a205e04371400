// decompress_bases / decompress_bases_device / compress_bases of include/ark_hip.hpp on BLS12-381 G1 (run on the GPU by
// tests/test_gpu_point_codec.py).  argv[1]: a file of  u64 n | u64 first_bad, bad_flags, not_reduced, no_root, off_subgroup |
// n encodings (48 bytes each) | n expected Affine points | n expected status bytes | n canonical encodings of those points.
#include <cstdio>
#include <cstring>
#include <vector>
#include "ark_hip.hpp"

using namespace ark_hip;
using Curve = Bls12_381G1;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static bool same(const BaseDecode& r, const uint64_t* want) {
  return r.first_bad == want[0] && r.bad_flags == want[1] && r.not_reduced == want[2] && r.no_root == want[3] && r.off_subgroup == want[4] &&
         r.ok == (want[1] + want[2] + want[3] + want[4] == 0);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t head[6];
  if (std::fread(head, 8, 6, f) != 6) return 2;
  const size_t n = head[0], E = compressed_size<Curve>();
  if (E != 48) return 2;
  std::vector<uint8_t> enc(n * E), want_st(n), canon(n * E);
  std::vector<Curve::AffineT> want(n);
  if (std::fread(enc.data(), E, n, f) != n || std::fread(want.data(), sizeof(Curve::AffineT), n, f) != n ||
      std::fread(want_st.data(), 1, n, f) != n || std::fread(canon.data(), E, n, f) != n)
    return 2;
  std::fclose(f);
  try {
    for (CheckMethod m : {CheckMethod::Auto, CheckMethod::Ladder, CheckMethod::Endomorphism}) {
      std::vector<Curve::AffineT> pts;
      BaseDecode r = decompress_bases<Curve>(enc.data(), n, pts, true, m, true);
      EXPECT(same(r, head + 1));
      EXPECT(r.status == want_st);
      EXPECT(pts.size() == n && std::memcmp(pts.data(), want.data(), n * sizeof(Curve::AffineT)) == 0);
      EXPECT(same(decompress_bases<Curve>(enc.data(), n, pts, true, m), head + 1));
    }
    EXPECT(compress_bases<Curve>(want) == canon);
    // without validation nothing has status 4
    std::vector<Curve::AffineT> pts;
    BaseDecode nv = decompress_bases<Curve>(enc.data(), n, pts, false);
    EXPECT(nv.off_subgroup == 0 && nv.bad_flags == head[2] && nv.not_reduced == head[3] && nv.no_root == head[4]);
    // the device forms
    void *d_enc = nullptr, *d_pts = nullptr, *d_st = nullptr, *d_back = nullptr;
    check(ark_hip_malloc(n * E, &d_enc), "ark_hip_malloc");
    check(ark_hip_malloc(n * sizeof(Curve::AffineT), &d_pts), "ark_hip_malloc");
    check(ark_hip_malloc(n, &d_st), "ark_hip_malloc");
    check(ark_hip_malloc(n * E, &d_back), "ark_hip_malloc");
    check(ark_hip_memcpy_h2d(d_enc, enc.data(), n * E), "ark_hip_memcpy_h2d");
    EXPECT(same(decompress_bases_device<Curve>(d_enc, n, d_pts, true, CheckMethod::Auto, d_st), head + 1));
    std::vector<uint8_t> got_st(n), back(n * E);
    std::vector<Curve::AffineT> got(n);
    check(ark_hip_memcpy_d2h(got_st.data(), d_st, n), "ark_hip_memcpy_d2h");
    check(ark_hip_memcpy_d2h(got.data(), d_pts, n * sizeof(Curve::AffineT)), "ark_hip_memcpy_d2h");
    EXPECT(got_st == want_st);
    EXPECT(std::memcmp(got.data(), want.data(), n * sizeof(Curve::AffineT)) == 0);
    compress_bases_device<Curve>(d_pts, n, d_back);
    check(ark_hip_synchronize(), "ark_hip_synchronize");
    check(ark_hip_memcpy_d2h(back.data(), d_back, n * E), "ark_hip_memcpy_d2h");
    EXPECT(back == canon);
    bool threw = false;
    try {
      (void)decompress_bases_device<Bn254G1>(d_enc, 1, d_pts, true, CheckMethod::Endomorphism);
    } catch (const Error& e) {
      threw = e.code == ARK_HIP_ERR_ARG;
    }
    EXPECT(threw);
    for (void* p : {d_enc, d_pts, d_st, d_back}) check(ark_hip_free(p), "ark_hip_free");
  } catch (const Error& e) {
    std::printf("ark_hip error %d in %s\n", e.code, e.what());
    return 1;
  }
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
