// The one-word fields of include/ark_hip.hpp (SmallRadix2EvaluationDomain, SmallDeviceVec) driven from a compiled C++ program on the
// GPU, against vectors the Python big-integer model wrote (tests/test_gpu_cpp_smallfp.py).  The file is a stream of decimal
// numbers, one block per field:
//   sfield  log  offset  k  n_coeffs
//   a[n]  b[n]                                  n = 2^log
//   algebra[n]       = -(((a + b) * b - a) * k)
//   inverse[n]       = batch_inverse(algebra)
//   evals[n]         = the coset transform of a
//   short_evals[n]   = the coset transform of a[0 .. n_coeffs)
//   canonical[n]     = into_canonical(a)
// followed by the model's domain constants: size_inv group_gen group_gen_inv offset_inv offset_pow_size.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>
#include "ark_hip.hpp"
using namespace ark_hip;

static int fails = 0;
#define EXPECT(c, msg) do { if (!(c)) { std::printf("FAIL (field %d): %s\n", SF, msg); fails++; } } while (0)

template <class W>
static std::vector<W> take(std::ifstream& in, size_t n) {
  std::vector<W> v(n);
  for (auto& x : v) { uint64_t t; in >> t; x = (W)t; }
  return v;
}

template <int SF>
static void block(std::ifstream& in, unsigned log, uint64_t offset, uint64_t k, size_t n_coeffs) {
  using D = SmallRadix2EvaluationDomain<SF>;
  using V = SmallDeviceVec<SF>;
  using W = typename D::Word;
  const size_t n = (size_t)1 << log;
  const auto a = take<W>(in, n), b = take<W>(in, n), algebra = take<W>(in, n), inverse = take<W>(in, n), evals = take<W>(in, n),
             short_evals = take<W>(in, n), canonical = take<W>(in, n);
  const auto consts = take<uint64_t>(in, 5);
  const SmallFieldInfo info = small_field_info<SF>();
  EXPECT(info.bytes == sizeof(W), "the word size");
  EXPECT(small_field_pow<SF>(offset, n) == consts[4], "pow");
  const SmallFftPlan plan = small_fft_plan<SF>(log);
  int stages = 0;
  for (int s : plan.stages) stages += s;
  EXPECT(stages == (int)log, "the plan's stages sum to log n");
  EXPECT(!D::create((size_t)1 << (info.two_adicity + 1)).has_value(), "no domain beyond the two-adicity");
  const D plain = *D::create(n - 1);
  EXPECT(plain.size() == n && plain.log_size_of_group() == log && plain.coset_offset() == info.r, "create");
  EXPECT(!plain.get_coset(0).has_value(), "no coset of zero");
  const D dom = *plain.get_coset(offset);
  EXPECT(dom.size_inv() == consts[0] && dom.group_gen() == consts[1] && dom.group_gen_inv() == consts[2] &&
             dom.coset_offset_inv() == consts[3] && dom.coset_offset_pow_size() == consts[4] && dom.coset_offset() == offset,
         "the domain constants");

  V va = V::from_vec(a), vb = V::from_vec(b);
  V vc = va.clone();
  vc += vb;
  vc *= vb;
  vc -= va;
  vc.scale(k).negate();
  EXPECT(vc.to_vec() == algebra, "+=, *=, -=, scale, negate");
  V vi = vc.clone();
  vi.batch_inverse();
  EXPECT(vi.to_vec() == inverse, "batch_inverse");
  EXPECT(va.to_vec() == a && va.len() == n, "the inputs are untouched");
  V ve = va.evaluate_over_domain(dom);
  EXPECT(ve.to_vec() == evals, "evaluate_over_domain");
  EXPECT(ve.interpolate(dom).to_vec() == a, "interpolate");
  V vs = V::from_vec(std::vector<W>(a.begin(), a.begin() + n_coeffs));
  EXPECT(vs.evaluate_over_domain(dom).to_vec() == short_evals, "evaluate_over_domain of a short polynomial");
  V vcan = va.clone();
  vcan.into_canonical();
  EXPECT(vcan.to_vec() == canonical, "into_canonical");
  vcan.from_canonical();
  EXPECT(vcan.to_vec() == a, "from_canonical");
  // host slices, and two columns with a gap through the batch entry
  std::vector<W> h = a;
  dom.fft_in_place(h);
  EXPECT(h == evals, "fft_in_place on a host vector");
  dom.ifft_in_place(h);
  EXPECT(h == a, "ifft_in_place on a host vector");
  std::vector<W> two(2 * n + 3, (W)~(W)0);
  for (size_t i = 0; i < n; i++) two[i] = a[i], two[n + 3 + i] = a[i];
  V vt = V::from_vec(two);
  dom.fft_batch_in_place(vt.device_ptr(), 2, n + 3);
  const auto out = vt.to_vec();
  bool ok = true;
  for (size_t i = 0; i < n; i++) ok = ok && out[i] == evals[i] && out[n + 3 + i] == evals[i];
  for (size_t i = 0; i < 3; i++) ok = ok && out[n + i] == (W)~(W)0;
  EXPECT(ok, "two columns with a gap");
  V zero(5);
  EXPECT(zero.to_vec() == std::vector<W>(5, 0), "a zeroed vector");
}

int main(int argc, char** argv) {
  if (ark_hip_device_count() <= 0) { std::printf("no GPU\n"); return 2; }
  if (argc != 2) { std::printf("usage: smallfp_check vectors.txt\n"); return 3; }
  std::ifstream in(argv[1]);
  int blocks = 0;
  try {
    uint64_t sf, log, offset, k, nc;
    while (in >> sf >> log >> offset >> k >> nc) {
      constexpr int SF = -1;
      if (sf == ARK_HIP_SFP_GOLDILOCKS) block<ARK_HIP_SFP_GOLDILOCKS>(in, (unsigned)log, offset, k, nc);
      else if (sf == ARK_HIP_SFP_BABYBEAR) block<ARK_HIP_SFP_BABYBEAR>(in, (unsigned)log, offset, k, nc);
      else if (sf == ARK_HIP_SFP_KOALABEAR) block<ARK_HIP_SFP_KOALABEAR>(in, (unsigned)log, offset, k, nc);
      else EXPECT(false, "unknown field in the vectors");
      blocks++;
    }
  } catch (const Error& e) {
    std::printf("FAIL: %s threw %d\n", e.what(), e.code);
    return 1;
  }
  if (fails || blocks != 3 || !in.eof()) { std::printf("%d failures, %d blocks\n", fails, blocks); return 1; }
  std::printf("all ok\n");
  return 0;
}
