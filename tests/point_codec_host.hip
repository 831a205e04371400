// sw_decompress_point / sw_compress_point / coord_sqrt (csrc/pointcodec.cuh) as a stand-alone HOST program: the very functions
// the codec kernels run, over vectors written by tests/test_point_codec_host.py.  Built with -fsanitize=address,undefined on the
// host side.  argv[i]: a file of bytes
//   u64 curve | u64 n | u64 combos | u64 m | n encodings (E bytes each)
//   per combo: u64 validate | u64 method | n status bytes | n points (2 fe_words u64 each)      decompress
//   n encodings: compress of the points of combo 0                                             compress
//   m elements in | m elements out | m ok bytes                                                  the square root
#include <cstdio>
#include <cstring>
#include <vector>
#include "pointcodec.cuh"
using namespace arkhip;

template <class C>
static int run(const std::vector<unsigned char>& f) {
  typedef typename C::F F;
  uint64_t hdr[4];
  std::memcpy(hdr, f.data(), 32);
  const size_t n = hdr[1], combos = hdr[2], m = hdr[3], E = CodecK<C>::E, PB = Affine<F>::BYTES, FB = F::FULL_BYTES;
  if (combos < 1 || f.size() != 32 + n * E + combos * (16 + n + n * PB) + n * E + m * (2 * FB + 1)) return 2;
  // exact-size copies on the heap: an access one byte past an encoding or a point is an ASan report
  std::vector<unsigned char> enc(f.begin() + 32, f.begin() + 32 + n * E);
  int bad = 0;
  size_t off = 32 + n * E;
  std::vector<uint64_t> first(n * PB / 8);
  for (size_t k = 0; k < combos; k++) {
    uint64_t vm[2];
    std::memcpy(vm, f.data() + off, 16);
    const unsigned char* st = f.data() + off + 16;
    const unsigned char* pts = st + n;
    for (size_t i = 0; i < n; i++) {
      std::vector<unsigned char> one(enc.begin() + i * E, enc.begin() + (i + 1) * E);
      Affine<F> p;
      const u32 got = sw_decompress_point<C>(one.data(), (int)vm[0], (int)vm[1], p);
      std::vector<unsigned char> out(PB);
      p.x.store(out.data());
      p.y.store(out.data() + FB);
      if (got != st[i] || std::memcmp(out.data(), pts + i * PB, PB)) {
        std::printf("curve %d encoding %zu validate %d method %d: status %u, expected %u\n", C::ID, i, (int)vm[0], (int)vm[1], got, st[i]);
        bad++;
      }
      if (k == 0) std::memcpy((char*)first.data() + i * PB, out.data(), PB);
    }
    off += 16 + n + n * PB;
  }
  for (size_t i = 0; i < n; i++) {
    std::vector<unsigned char> one(E, 0xEE);
    sw_compress_point<C>(Affine<F>::load((const char*)first.data() + i * PB), one.data());
    if (std::memcmp(one.data(), f.data() + off + i * E, E)) {
      std::printf("curve %d compress %zu differs\n", C::ID, i);
      bad++;
    }
  }
  off += n * E;
  const unsigned char *in = f.data() + off, *want = in + m * FB, *ok = want + m * FB;
  for (size_t i = 0; i < m; i++) {
    std::vector<unsigned char> a(in + i * FB, in + (i + 1) * FB), out(FB);
    F r;
    const u32 got = coord_sqrt_smaller(F::load(a.data()), r);
    r.store(out.data());
    if (got != ok[i] || std::memcmp(out.data(), want + i * FB, FB)) {
      std::printf("curve %d sqrt %zu: ok %u, expected %u\n", C::ID, i, got, ok[i]);
      bad++;
    }
  }
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  for (int a = 1; a < argc; a++) {
    FILE* fp = std::fopen(argv[a], "rb");
    if (!fp) return 2;
    std::vector<unsigned char> f;
    unsigned char buf[4096];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, fp)) > 0) f.insert(f.end(), buf, buf + got);
    std::fclose(fp);
    if (f.size() < 32) return 2;
    uint64_t curve;
    std::memcpy(&curve, f.data(), 8);
    int r = 2;
    switch ((int)curve) {
      case 0: r = run<BN254_G1>(f); break;
      case 1: r = run<BLS12_381_G1>(f); break;
      case 2: r = run<BLS12_377_G1>(f); break;
      case 3: r = run<BLS12_377_G2>(f); break;
      case 4: r = run<BLS12_381_G2>(f); break;
    }
    if (r == 0) std::printf("curve %d: ok\n", (int)curve);
    rc |= r;
  }
  return rc;
}
