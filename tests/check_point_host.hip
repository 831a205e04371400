// sw_check_point (csrc/pointcheck.cuh) as a stand-alone HOST program: the very function the check kernel runs, over planted
// vectors written by tests/test_check_bases_host.py.  Built with -fsanitize=address,undefined on the host side.
// argv[i]: a file of u64 words:  curve | n | combos | n points (2 * fe_words words each) | per combo: checks | method | n statuses
#include <cstdio>
#include <vector>
#include "pointcheck.cuh"
using namespace arkhip;

template <class C>
static int run(const std::vector<uint64_t>& w) {
  typedef typename C::F F;
  const size_t n = w[1], combos = w[2], words = Affine<F>::BYTES / 8;
  if (w.size() != 3 + n * words + combos * (2 + n)) return 2;
  const uint64_t* pts = w.data() + 3;
  int bad = 0;
  for (size_t k = 0; k < combos; k++) {
    const uint64_t* c = w.data() + 3 + n * words + k * (2 + n);
    for (size_t i = 0; i < n; i++) {
      const u32 st = sw_check_point<C>(Affine<F>::load(pts + i * words), (int)c[0], (int)c[1]);
      if (st != c[2 + i]) {
        std::printf("curve %d point %zu checks %d method %d: got %u, expected %u\n", C::ID, i, (int)c[0], (int)c[1], st, (unsigned)c[2 + i]);
        bad++;
      }
    }
  }
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  for (int a = 1; a < argc; a++) {
    FILE* f = std::fopen(argv[a], "rb");
    if (!f) return 2;
    std::vector<uint64_t> w;
    uint64_t buf[512];
    size_t got;
    while ((got = std::fread(buf, 8, 512, f)) > 0) w.insert(w.end(), buf, buf + got);
    std::fclose(f);
    if (w.size() < 3) return 2;
    int r = 2;
    switch ((int)w[0]) {
      case 0: r = run<BN254_G1>(w); break;
      case 1: r = run<BLS12_381_G1>(w); break;
      case 2: r = run<BLS12_377_G1>(w); break;
      case 3: r = run<BLS12_377_G2>(w); break;
      case 4: r = run<BLS12_381_G2>(w); break;
    }
    if (r == 0) std::printf("curve %d: ok\n", (int)w[0]);
    rc |= r;
  }
  return rc;
}
