// C ABI of libark_hip.so, unit 5 of 5 -- TEST HOOKS, linked into libark_hip_test.so only (the shipped libark_hip.so exports no
// ark_hip_test_* symbol: VERDICT r5 next #8).  Device field / point arithmetic and the host tail, reachable from tests/.
#ifndef ARK_HIP_TEST_HOOKS
#define ARK_HIP_TEST_HOOKS 1
#endif
#include "capi_core.hpp"
#include "capi_hostmath.hpp"
#include "capi_cache.hpp"
#include "capi_csr.hpp"
#include "msm_piece_dump.cuh"
#include "pointcheck.cuh"
#include "pointcodec.cuh"
#include "pointvec.cuh"
#include "lazytest_api.hpp"
#include "relaxtest_api.hpp"
#include "s30test_api.hpp"
#include "testops_api.hpp"
#include "scratch_list.hpp"
#include "transcript.cuh"
#include <map>
#include <string>
using namespace arkhip;
using namespace arkhip::capi;

namespace arkhip {
namespace capi {
int msm_sharded_emulated(int curve, int world, const void* const* d_bases, const void* const* d_scalars, const size_t* n_local,
                         int scalars_are_montgomery, uint64_t* out_xyz, int* path);   // capi_comm.hip
}
}
namespace {
// the test hooks of a curve / scalar field by its id (testops_api.hpp), nullptr for an id this build does not serve
const TestCurveOps* test_curve_ops(int curve) {
  switch (curve) {
#ifndef ARK_HIP_DEV
    case ARK_HIP_BN254_G1: return &test_curve_ops_BN254_G1();
    case ARK_HIP_BLS12_377_G1: return &test_curve_ops_BLS12_377_G1();
    case ARK_HIP_BLS12_377_G2: return &test_curve_ops_BLS12_377_G2();
    case ARK_HIP_BLS12_381_G2: return &test_curve_ops_BLS12_381_G2();
#endif
    case ARK_HIP_BLS12_381_G1: return &test_curve_ops_BLS12_381_G1();
  }
  return nullptr;
}
const TestFieldOps* test_field_ops(int field) {
  switch (field) {
#ifndef ARK_HIP_DEV
    case ARK_HIP_BN254_FR: return &test_field_ops_BN254_FR();
    case ARK_HIP_BLS12_377_FR: return &test_field_ops_BLS12_377_FR();
#endif
    case ARK_HIP_BLS12_381_FR: return &test_field_ops_BLS12_381_FR();
  }
  return nullptr;
}
// a base field is served through the curves over it: its own ops by the G1 unit, the Fp2 ops over it by the G2 unit (-1: none)
int curve_over(int field, bool g2) {
  switch (field) {
    case ARK_HIP_BN254_FQ: return g2 ? -1 : ARK_HIP_BN254_G1;
    case ARK_HIP_BLS12_381_FQ: return g2 ? ARK_HIP_BLS12_381_G2 : ARK_HIP_BLS12_381_G1;
    case ARK_HIP_BLS12_377_FQ: return g2 ? ARK_HIP_BLS12_377_G2 : ARK_HIP_BLS12_377_G1;
  }
  return -1;
}
// raw-limb ops of a field: a scalar field's own unit, a base field's through curve_over; pair: the Fp2L / Fp2 / Fp2Half ops
const TestRawOps* test_raw_ops(int field, bool pair) {
  const int curve = curve_over(field, pair);
  if (curve >= 0) return test_curve_ops(curve);
  return pair ? nullptr : test_field_ops(field);
}
// the elementwise hooks share one signature: member `op` of the hooks of `curve`, empty where this build does not serve it
typedef std::function<int(int, const void*, const void*, void*, size_t, hipStream_t)> elementwise_fn;
typedef int (TestCurveOps::*curve_elementwise)(int, const void*, const void*, void*, size_t, hipStream_t) const;
elementwise_fn curve_fn(int curve, curve_elementwise op) {
  const TestCurveOps* t = test_curve_ops(curve);
  if (!t) return nullptr;
  return [t, op](int k, const void* a, const void* b, void* r, size_t n, hipStream_t s) { return (t->*op)(k, a, b, r, n, s); };
}
// the product's field_op for a scalar field; base fields: through the G1 curve over them
elementwise_fn field_op_fn(int field) {
  if (const FieldOps* f = field_ops(field))
    return [f](int op, const void* a, const void* b, void* r, size_t n, hipStream_t s) { return f->field_op(op, a, b, r, n, s); };
  return curve_fn(curve_over(field, false), &TestCurveOps::basefield_op);
}
// limbs of the carry-free form of a field (params.hpp LZ_L): 14 x 28 bits for the 384-bit fields, 9 x 29 bits otherwise
int lazy_limbs(int field) { return (field == ARK_HIP_BLS12_381_FQ || field == ARK_HIP_BLS12_377_FQ) ? 14 : 9; }

// ---- scratch poisoning (scratch_list.hpp) ---------------------------------------------------------------------------------
// fill [0, bytes) with the bytes of `word`, repeated (plain vector stores; the last word may be cut)
__global__ void __launch_bounds__(256) scratch_fill_kernel(unsigned char* p, size_t bytes, u32 word) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w * 4 < bytes; w += stride) {
    if (w * 4 + 4 <= bytes) {
      ((u32*)p)[w] = word;
    } else {
      for (size_t o = w * 4; o < bytes; o++) p[o] = (unsigned char)(word >> (8 * (o & 3)));
    }
  }
}
// out[0] += the bytes of [lo, hi) that differ from the poison pattern, out[1] = min(out[1], offset of the first one)
__global__ void __launch_bounds__(256) scratch_scan_kernel(const unsigned char* p, size_t lo, size_t hi, u32 word,
                                                            unsigned long long* out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  unsigned long long cnt = 0, first = ~0ull;
  for (size_t w = lo / 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; w * 4 < hi; w += stride) {
    const size_t b0 = w * 4;
    if (b0 >= lo && b0 + 4 <= hi && ((const u32*)p)[w] == word) continue;
    for (size_t o = b0 < lo ? lo : b0; o < b0 + 4 && o < hi; o++)
      if (p[o] != (unsigned char)(word >> (8 * (o & 3)))) {
        cnt++;
        if (o < first) first = o;
      }
  }
  if (cnt) {
    atomicAdd(&out[0], cnt);
    atomicMin(&out[1], first);
  }
}
unsigned scratch_blocks(size_t bytes) {
  const size_t b = (bytes / 4 + 256) / 256;
  return (unsigned)(b < 4096 ? b : 4096);
}
// where every scratch buffer stood when it was last poisoned (per context: the hooks serve the calling thread's device)
std::map<std::string, const void*> g_poisoned[MAX_DEV];
std::mutex g_poisoned_mu;

bool scratch_jobs_busy(Context* c) {
  for (int l = 0; l < 2; l++) {
    std::lock_guard<std::mutex> lock(c->msm[l].mu);
    for (const auto& j : c->msm[l].jobs)
      if (j.busy) return true;
  }
  return false;
}
int scratch_poison(Context* c, u32 word) {
  if (scratch_jobs_busy(c)) return ARK_HIP_ERR_ARG;
  ARK_HIP_TRY(hipDeviceSynchronize());   // every stream of the context (and any other of this device) has drained
  std::lock_guard<std::mutex> lock(g_poisoned_mu);
  auto& seen = g_poisoned[c->logical];
  seen.clear();
  for_each_scratch(*c, [&](const char* name, DevBuf& b) {
    if (b.p && b.cap)
      hipLaunchKernelGGL(scratch_fill_kernel, dim3(scratch_blocks(b.cap)), dim3(256), 0, c->stream, (unsigned char*)b.p, b.cap, word);
    b.asked = 0;
    seen[name] = b.p;
  });
  for_each_pinned_scratch(*c, [&](const char* name, void* p, size_t cap, size_t) {
    for (size_t o = 0; p && o < cap; o++) ((unsigned char*)p)[o] = (unsigned char)(word >> (8 * (o & 3)));
    seen[name] = p;
  });
  for (int l = 0; l < 2; l++)
    for (auto& j : c->msm[l].jobs) j.pinned_asked = 0;
  ARK_HIP_TRY(hipGetLastError());
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
int scratch_report(Context* c, u32 word, ark_hip_scratch_row* rows, size_t cap_rows, size_t* n_rows) {
  ARK_HIP_TRY(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lock(g_poisoned_mu);
  auto& seen = g_poisoned[c->logical];
  size_t n = 0;
  for_each_scratch(*c, [&](const char*, DevBuf&) { n++; });
  const size_t ndev = n;
  for_each_pinned_scratch(*c, [&](const char*, void*, size_t, size_t) { n++; });
  *n_rows = n;
  if (n > cap_rows) return ARK_HIP_ERR_SIZE;
  unsigned long long* d_out = nullptr;
  std::vector<unsigned long long> h_out(2 * ndev);
  for (size_t i = 0; i < ndev; i++) h_out[2 * i] = 0, h_out[2 * i + 1] = ~0ull;
  ARK_HIP_TRY(hipMalloc((void**)&d_out, h_out.size() * 8));
  hipError_t e = hipMemcpy(d_out, h_out.data(), h_out.size() * 8, hipMemcpyHostToDevice);
  auto fill_row = [&](ark_hip_scratch_row& r, const char* name, const void* p, size_t cap, size_t asked) {
    memset(&r, 0, sizeof r);
    snprintf(r.name, sizeof r.name, "%s", name);
    r.cap = cap;
    r.asked = asked;
    auto it = seen.find(name);
    r.regrown = (it == seen.end() || it->second != p) ? 1 : 0;
    r.first_dirty_offset = ~0ull;
  };
  size_t i = 0;
  for_each_scratch(*c, [&](const char* name, DevBuf& b) {
    fill_row(rows[i], name, b.p, b.cap, b.asked);
    if (e == hipSuccess && b.p && b.asked < b.cap)
      hipLaunchKernelGGL(scratch_scan_kernel, dim3(scratch_blocks(b.cap - b.asked)), dim3(256), 0, c->stream, (const unsigned char*)b.p,
                         b.asked, b.cap, word, d_out + 2 * i);
    i++;
  });
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h_out.data(), d_out, h_out.size() * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_out);
  ARK_HIP_TRY(e);
  for (size_t k = 0; k < ndev; k++) {
    rows[k].dirty_beyond = h_out[2 * k];
    rows[k].first_dirty_offset = h_out[2 * k + 1];
  }
  for_each_pinned_scratch(*c, [&](const char* name, void* p, size_t cap, size_t asked) {
    fill_row(rows[i], name, p, cap, asked);
    for (size_t o = asked; p && o < cap; o++)
      if (((const unsigned char*)p)[o] != (unsigned char)(word >> (8 * (o & 3)))) {
        if (!rows[i].dirty_beyond) rows[i].first_dirty_offset = o;
        rows[i].dirty_beyond++;
      }
    i++;
  });
  return 0;
}
}  // namespace

extern "C" {

// ---- test hooks ----
static int run_elementwise(size_t abytes, size_t bbytes, size_t rbytes, const void* a, const void* b, void* r,
                           const elementwise_fn& fn, int op, size_t n) {
  if (!fn) return ARK_HIP_ERR_ARG;  // curve/field not in this (development) build
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) return 0;
  if (c->stage_a.ensure(abytes) || c->stage_b.ensure(bbytes ? bbytes : 16) || c->stage_c.ensure(rbytes)) return ARK_HIP_ERR_NOMEM;
  ARK_HIP_TRY(hipMemcpyAsync(c->stage_a.p, a, abytes, hipMemcpyHostToDevice, c->stream));
  if (b) ARK_HIP_TRY(hipMemcpyAsync(c->stage_b.p, b, bbytes, hipMemcpyHostToDevice, c->stream));
  int rc = fn(op, c->stage_a.p, b ? c->stage_b.p : nullptr, c->stage_c.p, n, c->stream);
  if (rc) return rc;
  ARK_HIP_TRY(hipMemcpyAsync(r, c->stage_c.p, rbytes, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int ark_hip_test_field_op(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* r, size_t n) {
  const bool lazy_op = op >= 20 && op <= 22;   // the 28-bit-limb device forms (testops.cuh)
  if (!a || !r || op < 0 || (op > 8 && !lazy_op) || op == 6) return ARK_HIP_ERR_ARG;
  size_t fb = field_bytes(field);
  if (field < 0 || field > 5) return ARK_HIP_ERR_ARG;
  if ((field == ARK_HIP_BN254_FQ || field == ARK_HIP_BLS12_381_FQ || field == ARK_HIP_BLS12_377_FQ) && op > 5 && !lazy_op)
    return ARK_HIP_ERR_ARG;
  return run_elementwise(n * fb, b ? n * fb : 0, n * fb, a, b, r, field_op_fn(field), op, n);
}

int ark_hip_test_basefield_op(int curve, int op, const uint64_t* a, const uint64_t* b, uint64_t* r, size_t n) {
  if (curve < 0 || curve > 4 || !a || !r || op < 0 || op > 5) return ARK_HIP_ERR_ARG;
  size_t fb = (size_t)CURVES[curve].fe_words * 8;
  return run_elementwise(n * fb, b ? n * fb : 0, n * fb, a, b, r, curve_fn(curve, &TestCurveOps::basefield_op), op, n);
}

int ark_hip_test_host_basefield_op(int curve, int op, const uint64_t* a, const uint64_t* b, uint64_t* r, size_t n) {
  if (curve < 0 || curve > 4 || !a || !r || op < 0 || op > 5 || (op <= 2 && !b)) return ARK_HIP_ERR_ARG;
  switch (curve) {
#ifndef ARK_HIP_DEV
    case ARK_HIP_BN254_G1: host_field_ops<BN254_G1::F>(op, a, b, r, n); return 0;
    case ARK_HIP_BLS12_377_G1: host_field_ops<BLS12_377_G1::F>(op, a, b, r, n); return 0;
    case ARK_HIP_BLS12_377_G2: host_field_ops<BLS12_377_G2::F>(op, a, b, r, n); return 0;
    case ARK_HIP_BLS12_381_G2: host_field_ops<BLS12_381_G2::F>(op, a, b, r, n); return 0;
#endif
    case ARK_HIP_BLS12_381_G1: host_field_ops<BLS12_381_G1::F>(op, a, b, r, n); return 0;
  }
  return ARK_HIP_ERR_ARG;
}

// sw_check_point (pointcheck.cuh) on the calling thread: the HOST build of the function the check kernel runs, no GPU involved
int ark_hip_test_host_sw_check(int curve, const uint64_t* bases_xy, size_t n, int checks, int method, uint8_t* status) {
  if (curve < 0 || curve > 4 || checks < 1 || checks > 3 || method < 0 || method > 2 || (n && (!bases_xy || !status))) return ARK_HIP_ERR_ARG;
  if (method == 2 && curve != ARK_HIP_BLS12_381_G1) return ARK_HIP_ERR_ARG;
  switch (curve) {
#ifndef ARK_HIP_DEV
    case ARK_HIP_BN254_G1: sw_check_host<BN254_G1>(bases_xy, n, checks, method, status); return 0;
    case ARK_HIP_BLS12_377_G1: sw_check_host<BLS12_377_G1>(bases_xy, n, checks, method, status); return 0;
    case ARK_HIP_BLS12_377_G2: sw_check_host<BLS12_377_G2>(bases_xy, n, checks, method, status); return 0;
    case ARK_HIP_BLS12_381_G2: sw_check_host<BLS12_381_G2>(bases_xy, n, checks, method, status); return 0;
#endif
    case ARK_HIP_BLS12_381_G1: sw_check_host<BLS12_381_G1>(bases_xy, n, checks, method, status); return 0;
  }
  return ARK_HIP_ERR_ARG;
}

// sw_decompress_point / sw_compress_point (pointcodec.cuh) on the calling thread: the HOST builds of the functions the codec kernels
// run, no GPU involved
int ark_hip_test_host_sw_decompress(int curve, const uint8_t* bytes, size_t n, int validate, int method, uint64_t* points_xy,
                                    uint8_t* status) {
  if (curve < 0 || curve > 4 || validate < 0 || validate > 1 || method < 0 || method > 2 || (n && (!bytes || !points_xy))) return ARK_HIP_ERR_ARG;
  if (method == 2 && curve != ARK_HIP_BLS12_381_G1) return ARK_HIP_ERR_ARG;
  switch (curve) {
#ifndef ARK_HIP_DEV
    case ARK_HIP_BN254_G1: sw_decompress_host<BN254_G1>(bytes, n, validate, method, points_xy, status); return 0;
    case ARK_HIP_BLS12_377_G1: sw_decompress_host<BLS12_377_G1>(bytes, n, validate, method, points_xy, status); return 0;
    case ARK_HIP_BLS12_377_G2: sw_decompress_host<BLS12_377_G2>(bytes, n, validate, method, points_xy, status); return 0;
    case ARK_HIP_BLS12_381_G2: sw_decompress_host<BLS12_381_G2>(bytes, n, validate, method, points_xy, status); return 0;
#endif
    case ARK_HIP_BLS12_381_G1: sw_decompress_host<BLS12_381_G1>(bytes, n, validate, method, points_xy, status); return 0;
  }
  return ARK_HIP_ERR_ARG;
}
int ark_hip_test_host_sw_compress(int curve, const uint64_t* points_xy, size_t n, uint8_t* bytes) {
  if (curve < 0 || curve > 4 || (n && (!points_xy || !bytes))) return ARK_HIP_ERR_ARG;
  switch (curve) {
#ifndef ARK_HIP_DEV
    case ARK_HIP_BN254_G1: sw_compress_host<BN254_G1>(points_xy, n, bytes); return 0;
    case ARK_HIP_BLS12_377_G1: sw_compress_host<BLS12_377_G1>(points_xy, n, bytes); return 0;
    case ARK_HIP_BLS12_377_G2: sw_compress_host<BLS12_377_G2>(points_xy, n, bytes); return 0;
    case ARK_HIP_BLS12_381_G2: sw_compress_host<BLS12_381_G2>(points_xy, n, bytes); return 0;
#endif
    case ARK_HIP_BLS12_381_G1: sw_compress_host<BLS12_381_G1>(points_xy, n, bytes); return 0;
  }
  return ARK_HIP_ERR_ARG;
}
// pv_chain_point / pv_add_point (pointvec.cuh) on the calling thread: the HOST builds of the functions the point-vector kernels run,
// no GPU involved.  impl: 0 = the form the device entry runs by default (carry-free limbs for G1, saturated for G2), 1 = saturated.
int ark_hip_test_host_sw_mul(int curve, const uint64_t* points, int form, const uint64_t* scalars, size_t n_scalars,
                             int scalars_are_montgomery, int impl, size_t n, uint64_t* out_xyz) {
  if (curve < 0 || curve > 4 || form < 0 || form > 1 || impl < 0 || impl > 1 || (n_scalars != 1 && n_scalars != n) ||
      (n && (!points || !scalars || !out_xyz)))
    return ARK_HIP_ERR_ARG;
  const size_t ks = n_scalars == 1 ? 0 : 8;
#define CALL(C) pv_chain_host<C, 1>(points, nullptr, form, scalars, ks, nullptr, nullptr, scalars_are_montgomery, impl, n, out_xyz)
  switch (curve) {
#ifndef ARK_HIP_DEV
    case ARK_HIP_BN254_G1: CALL(BN254_G1); return 0;
    case ARK_HIP_BLS12_377_G1: CALL(BLS12_377_G1); return 0;
    case ARK_HIP_BLS12_377_G2: CALL(BLS12_377_G2); return 0;
    case ARK_HIP_BLS12_381_G2: CALL(BLS12_381_G2); return 0;
#endif
    case ARK_HIP_BLS12_381_G1: CALL(BLS12_381_G1); return 0;
  }
  return ARK_HIP_ERR_ARG;
#undef CALL
}
int ark_hip_test_host_sw_fold(int curve, const uint64_t* lo, const uint64_t* hi, int form, const uint64_t a[4], const uint64_t b[4],
                              int scalars_are_montgomery, int impl, size_t n, uint64_t* out_xyz) {
  if (curve < 0 || curve > 4 || form < 0 || form > 1 || impl < 0 || impl > 1 || !a || !b || (n && (!lo || !hi || !out_xyz))) return ARK_HIP_ERR_ARG;
#define CALL(C) pv_chain_host<C, 2>(lo, hi, form, nullptr, 0, a, b, scalars_are_montgomery, impl, n, out_xyz)
  switch (curve) {
#ifndef ARK_HIP_DEV
    case ARK_HIP_BN254_G1: CALL(BN254_G1); return 0;
    case ARK_HIP_BLS12_377_G1: CALL(BLS12_377_G1); return 0;
    case ARK_HIP_BLS12_377_G2: CALL(BLS12_377_G2); return 0;
    case ARK_HIP_BLS12_381_G2: CALL(BLS12_381_G2); return 0;
#endif
    case ARK_HIP_BLS12_381_G1: CALL(BLS12_381_G1); return 0;
  }
  return ARK_HIP_ERR_ARG;
#undef CALL
}
int ark_hip_test_host_sw_add(int curve, const uint64_t* a_xyz, const uint64_t* b_xyz, int negate_b, size_t n, uint64_t* out_xyz) {
  if (curve < 0 || curve > 4 || (n && (!a_xyz || !b_xyz || !out_xyz))) return ARK_HIP_ERR_ARG;
#define CALL(C) pv_add_host<C>(a_xyz, b_xyz, negate_b, n, out_xyz)
  switch (curve) {
#ifndef ARK_HIP_DEV
    case ARK_HIP_BN254_G1: CALL(BN254_G1); return 0;
    case ARK_HIP_BLS12_377_G1: CALL(BLS12_377_G1); return 0;
    case ARK_HIP_BLS12_377_G2: CALL(BLS12_377_G2); return 0;
    case ARK_HIP_BLS12_381_G2: CALL(BLS12_381_G2); return 0;
#endif
    case ARK_HIP_BLS12_381_G1: CALL(BLS12_381_G1); return 0;
  }
  return ARK_HIP_ERR_ARG;
#undef CALL
}
// the square root in the curve's coordinate field (Fp or Fp2): out = the root r with r <= -r, or zero with ok = 0
int ark_hip_test_host_coord_sqrt(int curve, const uint64_t* in, uint64_t* out, uint8_t* ok, size_t n) {
  if (curve < 0 || curve > 4 || (n && (!in || !out || !ok))) return ARK_HIP_ERR_ARG;
  switch (curve) {
#ifndef ARK_HIP_DEV
    case ARK_HIP_BN254_G1: coord_sqrt_host<BN254_G1>(in, out, ok, n); return 0;
    case ARK_HIP_BLS12_377_G1: coord_sqrt_host<BLS12_377_G1>(in, out, ok, n); return 0;
    case ARK_HIP_BLS12_377_G2: coord_sqrt_host<BLS12_377_G2>(in, out, ok, n); return 0;
    case ARK_HIP_BLS12_381_G2: coord_sqrt_host<BLS12_381_G2>(in, out, ok, n); return 0;
#endif
    case ARK_HIP_BLS12_381_G1: coord_sqrt_host<BLS12_381_G1>(in, out, ok, n); return 0;
  }
  return ARK_HIP_ERR_ARG;
}
int ark_hip_test_coord_sqrt(int curve, const uint64_t* in, uint64_t* out, uint8_t* ok, size_t n) {
  if (curve < 0 || curve > 4 || (n && (!in || !out || !ok))) return ARK_HIP_ERR_ARG;
  const TestCurveOps* ops = test_curve_ops(curve);
  if (!ops) return ARK_HIP_ERR_ARG;
  if (n == 0) return 0;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  const size_t fb = (size_t)CURVES[curve].fe_words * 8;
  if (c->stage_a.cap < n * fb || c->stage_b.cap < n || c->stage_c.cap < n * fb)
    if (int rc = sync_compute(c)) return rc;
  if (c->stage_a.ensure(n * fb) || c->stage_b.ensure(n) || c->stage_c.ensure(n * fb)) return ARK_HIP_ERR_NOMEM;
  ARK_HIP_TRY(hipMemcpyAsync(c->stage_a.p, in, n * fb, hipMemcpyHostToDevice, c->stream));
  if (int rc = ops->coord_sqrt(c->stage_a.p, c->stage_c.p, c->stage_b.p, n, c->stream)) return rc;
  ARK_HIP_TRY(hipMemcpyAsync(out, c->stage_c.p, n * fb, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipMemcpyAsync(ok, c->stage_b.p, n, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int ark_hip_test_point_op(int curve, int kind, const uint64_t* acc, const uint64_t* other, uint64_t* out, size_t n) {
  const bool lazy_kind = kind >= 12 && kind <= 15;   // the carry-free forms of kinds 2 / 3 / 4 (testops.cuh)
  if (curve < 0 || curve > 4 || !acc || !out || kind < 2 || (kind > 7 && !lazy_kind)) return ARK_HIP_ERR_ARG;
  size_t fb = (size_t)CURVES[curve].fe_words * 8;
  size_t abytes = n * fb * (kind == 7 ? 2 : 4);
  size_t bbytes = (kind == 2 || kind == 3 || kind == 12 || kind == 13) ? n * fb * 2 : ((kind == 4 || kind >= 14) ? n * fb * 4 : 0);
  size_t rbytes = n * fb * (kind == 6 ? 3 : 4);
  if (bbytes && !other) return ARK_HIP_ERR_ARG;
  return run_elementwise(abytes, bbytes, rbytes, acc, bbytes ? other : nullptr, out, curve_fn(curve, &TestCurveOps::point_op), kind, n);
}

int ark_hip_test_lazy_raw_op(int field, int op, int k, int h, const uint32_t* in, uint32_t* out, size_t n) {
  using namespace arkhip::lazytest;
  if (field < 0 || field > 5 || !in || !out) return ARK_HIP_ERR_ARG;
  const Row* row = row_of(op);
  if (!row || !params_ok(op, k, h)) return ARK_HIP_ERR_ARG;
  const bool x2 = op >= X2_FIRST;
  const TestRawOps* ops = test_raw_ops(field, x2);
  if (!ops || (x2 && (n & 1))) return ARK_HIP_ERR_ARG;
  const size_t L = (size_t)lazy_limbs(field);
  const size_t ibytes = n * (size_t)row->arity * L * 4, obytes = n * (L + 1) * 4;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) return 0;
  if (c->stage_a.ensure(ibytes) || c->stage_c.ensure(obytes)) return ARK_HIP_ERR_NOMEM;
  ARK_HIP_TRY(hipMemcpyAsync(c->stage_a.p, in, ibytes, hipMemcpyHostToDevice, c->stream));
  const int rc = ops->lazy_raw_op(op, k, h, c->stage_a.p, c->stage_c.p, n, c->stream);
  if (rc) return rc == -1 ? ARK_HIP_ERR_ARG : rc;   // -1: not an op of this field's unit (Fft29 outside the scalar fields, ..)
  ARK_HIP_TRY(hipMemcpyAsync(out, c->stage_c.p, obytes, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int ark_hip_test_lazy_acc_op(int curve, int kind, const void* acc, const void* other, void* out, size_t n) {
  using namespace arkhip::lazytest;
  if (curve < 0 || curve > 4 || !acc || !out || kind < 0 || kind >= ACC_KINDS) return ARK_HIP_ERR_ARG;
  const size_t fb = (size_t)CURVES[curve].fe_words * 8;
  const size_t L = curve == 0 ? 9 : 14;
  const size_t slot = (curve >= 3 ? 8 * L + 1 : 4 * L + 1) * 4;   // LazyK::WORDS words
  const size_t abytes = n * (kind == ACC_FROM_BUCKET ? 4 * fb : slot);
  size_t bbytes = 0;
  if (kind <= ACC_MDBL_NEG) bbytes = n * 2 * fb;
  else if (kind == ACC_ADD) bbytes = n * 4 * fb;
  else if (kind == ACC_ADD_ACC) bbytes = n * slot;
  const size_t rbytes = n * (kind == ACC_TO_BUCKET ? 4 * fb : slot);
  if (bbytes && !other) return ARK_HIP_ERR_ARG;
  return run_elementwise(abytes, bbytes, rbytes, acc, bbytes ? other : nullptr, out, curve_fn(curve, &TestCurveOps::lazy_acc_op), kind, n);
}

int ark_hip_test_s30_op(int op, const void* in, void* out, size_t n) {
  using namespace arkhip::s30test;
  if (op < 0 || op >= OPS || !in || !out) return ARK_HIP_ERR_ARG;
  const size_t ibytes = n * (size_t)in_words(op) * 4, obytes = n * (size_t)out_words(op) * 4;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) return 0;
  if (c->stage_a.ensure(ibytes) || c->stage_c.ensure(obytes)) return ARK_HIP_ERR_NOMEM;
  ARK_HIP_TRY(hipMemcpyAsync(c->stage_a.p, in, ibytes, hipMemcpyHostToDevice, c->stream));
  const int rc = test_curve_ops_BLS12_381_G1().s30_raw_op(op, c->stage_a.p, c->stage_c.p, n, c->stream);
  if (rc) return rc == -1 ? ARK_HIP_ERR_ARG : rc;
  ARK_HIP_TRY(hipMemcpyAsync(out, c->stage_c.p, obytes, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int ark_hip_test_relaxed_raw_op(int field, int op, const uint32_t* in, uint32_t* out, size_t n) {
  using namespace arkhip::relaxtest;
  if (field < 0 || field > 5 || !in || !out) return ARK_HIP_ERR_ARG;
  const Row* row = row_of(op);
  if (!row || !served(op, field)) return ARK_HIP_ERR_ARG;
  const bool pair = row->unit != U_FP;
  const TestRawOps* ops = test_raw_ops(field, pair);
  if (!ops || (pair && (n & 1))) return ARK_HIP_ERR_ARG;
  const size_t N = (field == ARK_HIP_BLS12_381_FQ || field == ARK_HIP_BLS12_377_FQ) ? 12 : 8;
  const size_t ibytes = n * (size_t)row->arity * N * 4, obytes = n * (N + 1) * 4;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) return 0;
  if (c->stage_a.ensure(ibytes) || c->stage_c.ensure(obytes)) return ARK_HIP_ERR_NOMEM;
  ARK_HIP_TRY(hipMemcpyAsync(c->stage_a.p, in, ibytes, hipMemcpyHostToDevice, c->stream));
  const int rc = ops->relaxed_raw_op(op, c->stage_a.p, c->stage_c.p, n, c->stream);
  if (rc) return rc == -1 ? ARK_HIP_ERR_ARG : rc;
  ARK_HIP_TRY(hipMemcpyAsync(out, c->stage_c.p, obytes, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// the transcript's 512-bit reduction alone: on the host, or in a one-lane kernel
extern "C++" {
template <class FP>
int transcript_reduce_host(const uint8_t* bytes64, uint64_t* out) {
  u32 w[16];
  memcpy(w, bytes64, 64);
  transcript_reduce512<Fp<FP>>(w).store(out);
  return 0;
}
}
int ark_hip_test_transcript_reduce(int field, const uint8_t* bytes64, int on_device, uint64_t* out) {
  const TestFieldOps* ops = test_field_ops(field);
  if (!ops || !bytes64 || !out) return ARK_HIP_ERR_ARG;
  if (!on_device) {
#define X(NAME) transcript_reduce_host<NAME>(bytes64, out)
    ARK_FIELD_SWITCH(field, X);
#undef X
  }
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (c->stage_a.ensure(64) || c->stage_c.ensure(32)) return ARK_HIP_ERR_NOMEM;
  ARK_HIP_TRY(hipMemcpyAsync(c->stage_a.p, bytes64, 64, hipMemcpyHostToDevice, c->stream));
  if (int rc = ops->transcript_reduce(c->stage_a.p, c->stage_c.p, c->stream)) return rc;
  ARK_HIP_TRY(hipMemcpyAsync(out, c->stage_c.p, 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
// the whole challenge in a one-lane kernel: the counterpart of ark_hip_transcript_challenge
int ark_hip_test_transcript_challenge_device(int field, uint8_t* state, const uint64_t* elements, unsigned count, uint64_t* out) {
  const TestFieldOps* ops = test_field_ops(field);
  if (!ops || !state || !out || (count && !elements) || count > (1u << 16)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  const size_t mbytes = (size_t)transcript_words(count) * 4, ebytes = (size_t)count * 32;
  if (c->stage_a.ensure(mbytes) || c->stage_c.ensure(ebytes + 32)) return ARK_HIP_ERR_NOMEM;
  char *msg = (char*)c->stage_a.p, *el = (char*)c->stage_c.p, *res = el + ebytes;   // [message] and [elements | result]
  ARK_HIP_TRY(hipMemcpyAsync(msg, state, 32, hipMemcpyHostToDevice, c->stream));
  if (count) ARK_HIP_TRY(hipMemcpyAsync(el, elements, ebytes, hipMemcpyHostToDevice, c->stream));
  if (int rc = ops->transcript_challenge(msg, el, count, res, c->stream)) return rc;
  ARK_HIP_TRY(hipMemcpyAsync(out, res, 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipMemcpyAsync(state, msg, 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
// the home slot the lookup kernels give an element: host only, no device
int ark_hip_test_lookup_slot(int field, const uint64_t* element, unsigned capacity_log, uint32_t* slot) {
  const TestFieldOps* ops = test_field_ops(field);
  if (!ops || !element || !slot || capacity_log < 1 || capacity_log > 29) return ARK_HIP_ERR_ARG;
  u32 w[8];
  for (int q = 0; q < 4; q++) { w[2 * q] = (u32)element[q]; w[2 * q + 1] = (u32)(element[q] >> 32); }
  *slot = ops->lookup_slot(w, capacity_log);
  return 0;
}

int ark_hip_test_relaxed_acc_op(int curve, int kind, const void* acc, const void* other, void* out, size_t n) {
  using namespace arkhip::relaxtest;
  if (curve < 0 || curve > 4 || !acc || !out || kind < 0 || kind >= ACC_KINDS) return ARK_HIP_ERR_ARG;
  const size_t fb = (size_t)CURVES[curve].fe_words * 8;
  const size_t bbytes = kind == ACC_MADD ? n * 2 * fb : kind == ACC_ADD ? n * 4 * fb : 0;
  if (bbytes && !other) return ARK_HIP_ERR_ARG;
  return run_elementwise(n * 4 * fb, bbytes, n * 4 * fb, acc, bbytes ? other : nullptr, out, curve_fn(curve, &TestCurveOps::relaxed_acc_op), kind, n);
}

static int host_fold_any(int curve, const uint64_t* parts, int windows, int nbits, u32 l0, const int* widths, uint64_t* out_xyz) {
  switch (curve) {
    case 0: return host_fold<BN254_G1>(parts, windows, nbits, l0, widths, out_xyz);
    case 1: return host_fold<BLS12_381_G1>(parts, windows, nbits, l0, widths, out_xyz);
    case 2: return host_fold<BLS12_377_G1>(parts, windows, nbits, l0, widths, out_xyz);
    case 3: return host_fold<BLS12_377_G2>(parts, windows, nbits, l0, widths, out_xyz);
    case 4: return host_fold<BLS12_381_G2>(parts, windows, nbits, l0, widths, out_xyz);
  }
  return ARK_HIP_ERR_ARG;
}
int ark_hip_test_msm_host_fold(int curve, const uint64_t* parts, int windows, int nbits, int log2_l0, const int* widths,
                               uint64_t* out_xyz) {
  if (!parts || !widths || !out_xyz || windows < 1 || windows > 256 || nbits < 0 || nbits > 31 || log2_l0 < 0 || log2_l0 > 16)
    return ARK_HIP_ERR_ARG;
  return host_fold_any(curve, parts, windows, nbits, 1u << log2_l0, widths, out_xyz);
}
// the same tail with the level-0 chunk length given itself (any integer 1 .. 65536, not only a power of two)
int ark_hip_test_msm_host_fold_l0(int curve, const uint64_t* parts, int windows, int nbits, int l0, const int* widths,
                                  uint64_t* out_xyz) {
  if (!parts || !widths || !out_xyz || windows < 1 || windows > 256 || nbits < 0 || nbits > 31 || l0 < 1 || l0 > 65536)
    return ARK_HIP_ERR_ARG;
  return host_fold_any(curve, parts, windows, nbits, (u32)l0, widths, out_xyz);
}
// Test hook (host only, no device): the bucket reduction's geometry for a plan given as (c, W, narrow, shared), with every
// knob at its default (msm_plan.hpp: msm_reduce_geometry)
int ark_hip_test_msm_reduce_geometry(int curve, int c, int W, int narrow, int shared, size_t resident_lanes, uint32_t out[12]) {
  if (curve < 0 || curve > 4 || !out || c < 2 || c > 26 || W < 1 || W > 256 || narrow < 0 || narrow > W) return ARK_HIP_ERR_ARG;
  const MsmPlan pl{c, W, narrow, (size_t)W << (c - 1), shared != 0};
  const MsmReduceGeom g = msm_reduce_geometry(pl, msm_lanes_per_point(curve), msm_scalar_bits(curve), resident_lanes, MsmKnobs{});
  const uint32_t v[12] = {g.L0, (uint32_t)g.m, (uint32_t)g.mn, (uint32_t)g.nbits, g.Q, g.two_digit ? 1u : 0u, g.d2, g.rows2,
                          (uint32_t)g.nsum2, g.chunk, g.nchunks, (uint32_t)g.npairs};
  for (int k = 0; k < 12; k++) out[k] = v[k];
  return 0;
}
// The explicit knob record of the two hooks below -> MsmKnobs: everything else stays at its default, and no environment
// variable is read.  knobs[8] = c, hb, tile, heavy, groups, big_slices, compact, probe.
static MsmKnobs knobs_of_record(const int32_t* r) {
  MsmKnobs k;
  k.c = r[0] >= 3 && r[0] <= 26 ? r[0] : 0;
  k.hb = r[1];
  k.tile = r[2];
  k.heavy = r[3] >= 64 ? r[3] : 0;
  k.groups = r[4];
  k.big_slices = r[5] != 0;
  k.compact = r[6] != 0;
  k.probe = r[7] != 0;
  return k;
}
// Test hook (host only, no device): the geometry of the partition sort, the order pass and the heavy-run arrays
// (msm_plan.hpp: msm_sort_geometry, msm_heavy_geometry) for n carried scalars under the plan (c, W, narrow, shared); W = 0: the
// window layout of the curve's full-width scalars for c.
int ark_hip_test_msm_sort_geometry(int curve, size_t n, int c, int W, int narrow, int shared, const int32_t knobs[8], uint64_t out[32]) {
  if (curve < 0 || curve > 4 || !out || !knobs || n == 0 || n >= (1ull << 31) || c < 3 || c > 26 || W < 0 || W > 256 || narrow < 0 ||
      (W && narrow > W))
    return ARK_HIP_ERR_ARG;
  if (W == 0) msm_window_layout(c, msm_scalar_bits(curve), &W, &narrow);
  const MsmKnobs k = knobs_of_record(knobs);
  const MsmPlan pl{c, W, narrow, (size_t)W << (c - 1), shared != 0};
  const MsmSortGeom g = msm_sort_geometry(n, pl, k);
  const MsmHeavyGeom h = msm_heavy_geometry(n, pl, k);
  const bool accepted = (size_t)n * (size_t)W < (1ull << 32) && g.lds_a <= PART_SCATTER_LDS_MAX;   // msm_setup's two size checks
  const uint64_t v[32] = {(uint64_t)g.HB, (uint64_t)g.LB, g.nsuper, g.tile, g.ntiles, g.nthist, g.lds_a, g.lds_b, g.stage_cap,
                          g.big_on ? 1u : 0u, g.big_region, g.noblk, g.nohist, g.nsums, h.mean_load, h.forced_thresh, h.max_heavy,
                          h.max_items, (uint64_t)W, (uint64_t)narrow, accepted ? 1u : 0u, PART_LDS_WORDS, PART_SCATTER_LDS_MAX,
                          PART_BIG, SCAN_SMALL_MAX, HEAVY_CHUNK, (uint64_t)SCAN_TILE, (uint64_t)ORDER_TILE, (uint64_t)ORDER_BINS,
                          (uint64_t)msm_window_groups(n, pl, false, k), 0, 0};
  for (int i = 0; i < 32; i++) out[i] = v[i];
  return 0;
}
// Test hook: the integer stages of one plain MSM call, copied out (msm_stage_dump.cuh, which documents header, out and cap).
// scalars: n scalars as the MSM entries take them -- 32-byte field elements, or sbytes-byte unsigned integers with sbits
// significant bits (sbytes = 0: full width) -- in device memory (on_device) or host memory.  Runs on lane 0's workspace and
// stream like a synchronous MSM entry, and returns with both idle.
int ark_hip_test_msm_sort_stages(int curve, const void* scalars, int on_device, size_t n, int mont, int sbytes, int sbits,
                                 const int32_t knobs[8], uint64_t header[32], void* const* out, const size_t* cap_words) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops || !scalars || !knobs || !header || n == 0 || (out && !cap_words)) return ARK_HIP_ERR_ARG;
  if (sbytes == 0 && sbits != 0) return ARK_HIP_ERR_ARG;
  if (sbytes && sbits == 0) sbits = 8 * sbytes;
  const MsmKnobs k = knobs_of_record(knobs);
  ARK_SCOPE(sc);
  Context* c = sc.c;
  hipStream_t st;
  if (int rc = msm_lane_stream(c, 0, &st)) return rc;
  const void* d_scalars = scalars;
  if (!on_device) {
    const size_t bytes = n * (size_t)(sbytes ? sbytes : 32);
    if (c->stage_a.cap < bytes)
      if (int rc = sync_compute(c)) return rc;
    if (c->stage_a.ensure(bytes)) return ARK_HIP_ERR_NOMEM;
    ARK_HIP_TRY(hipMemcpyAsync(c->stage_a.p, scalars, bytes, hipMemcpyHostToDevice, st));
    d_scalars = c->stage_a.p;
  }
  return ops->msm_sort_stages(c->msm[0], d_scalars, n, mont, st, sbytes, sbits, k, header, out, cap_words);
}
// Test hook: one MSM run as explicit pieces that share one plan and one bucket array, the buckets copied out behind every piece
// (msm_piece_dump.cuh, which documents header, hctr_out and buckets_out).  bases / scalars: the n pairs in device memory
// (on_device) or host memory; sizes[npieces] sum to n.  The plan is msm_stream's: msm_default_plan(.., streamed = true) under
// the knobs of the record, and no environment variable is read:
//   knobs[12] = c, heavy, hb, probe, compact, lazy, tile, big_slices, prepared, 0, 0, 0
// (prepared != 0: the plan is handed to msm_enqueue as a prepared set's too, which a piece must refuse with ARK_HIP_ERR_ARG).
// Runs on lane 0's workspace and stream, and returns with both idle and no job slot taken.
int ark_hip_test_msm_pieces(int curve, const void* bases, const void* scalars, int on_device, size_t n, int mont, const size_t* sizes,
                            int npieces, const int32_t knobs[12], uint64_t header[80], uint32_t* hctr_out, size_t hctr_cap_words,
                            void* buckets_out, size_t buckets_cap_bytes, uint64_t* out_xyz) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops || !bases || !scalars || !sizes || !knobs || !header || n == 0 || n >= (1ull << 31) || npieces < 1 ||
      npieces > MPD_MAX_PIECES || knobs[9] || knobs[10] || knobs[11])
    return ARK_HIP_ERR_ARG;
  MsmKnobs k;
  k.c = knobs[0] >= 3 && knobs[0] <= 26 ? knobs[0] : 0;
  k.heavy = knobs[1] >= 64 ? knobs[1] : 0;
  k.hb = knobs[2];
  k.probe = knobs[3] != 0;
  k.compact = knobs[4] != 0;
  k.lazy = knobs[5] != 0;
  k.tile = knobs[6];
  k.big_slices = knobs[7] != 0;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  hipStream_t st;
  if (int rc = msm_lane_stream(c, 0, &st)) return rc;
  // the plan as msm_stream makes it: the window size from a sample of the host scalars where the probe is on and n is large
  MsmWidths widths{};
  bool skewed = false;
  if (k.probe && !on_device && n >= ((size_t)1 << 19)) {
    ops->msm_sample_widths(scalars, n, mont, &widths);
    skewed = msm_widths_skewed(widths);
  }
  const MsmPlan plan = msm_default_plan(curve, n, msm_scalar_bits(curve), false, skewed ? &widths : nullptr, k, /*streamed=*/true);
  size_t step = 0;
  for (int i = 0; i < npieces; i++) step = sizes[i] > step ? sizes[i] : step;
  if ((size_t)step * (size_t)plan.W >= (1ull << 32)) return ARK_HIP_ERR_SIZE;
  const size_t ab = (size_t)CURVES[curve].fe_words * 16;
  const size_t need = plan.nbuckets() * (size_t)CURVES[curve].fe_words * 32;   // XYZZ: four field elements
  const bool grow = c->piece_buckets.cap < need || (!on_device && (c->stage_a.cap < n * 32 || c->stage_b.cap < n * ab));
  if (grow)
    if (int rc = sync_compute(c)) return rc;
  if (c->piece_buckets.ensure(need) || (!on_device && (c->stage_a.ensure(n * 32) || c->stage_b.ensure(n * ab)))) return ARK_HIP_ERR_NOMEM;
  for (int j = 0; j < 2; j++)
    if (!c->piece_ev[j]) ARK_HIP_TRY(hipEventCreateWithFlags(&c->piece_ev[j], hipEventDisableTiming));
  const void *d_bases = bases, *d_scalars = scalars;
  if (!on_device && hctr_out) {
    ARK_HIP_TRY(hipMemcpyAsync(c->stage_a.p, scalars, n * 32, hipMemcpyHostToDevice, st));
    ARK_HIP_TRY(hipMemcpyAsync(c->stage_b.p, bases, n * ab, hipMemcpyHostToDevice, st));
  }
  if (!on_device) {
    d_scalars = c->stage_a.p;
    d_bases = c->stage_b.p;
  }
  return ops->msm_piece_dump(c->msm[0], d_bases, d_scalars, n, mont, st, sizes, npieces, plan, k, knobs[8] != 0, c->piece_buckets.p,
                             c->piece_ev, header, hctr_out, hctr_cap_words, buckets_out, buckets_cap_bytes, out_xyz);
}
// Test hook (host only, no device): the verified cache's tag of `words` u64 words -- tests/test_capi_host.py checks that
// edits the round-4 hash could not see (a two-word edit built from its published constants) change it.
int ark_hip_test_base_hash(const uint64_t* p, size_t words, uint64_t out[2]) {
  if (!out || (words && !p)) return ARK_HIP_ERR_ARG;
  const Hash128 h = base_hash(p, words);
  out[0] = h.lo;
  out[1] = h.hi;
  return 0;
}
/* test hook: msm_sharded's exchange with the ranks emulated in one process (capi_comm.hip: msm_sharded_emulated) */
int ark_hip_test_msm_sharded_emulated(int curve, int world, const void* const* d_bases, const void* const* d_scalars,
                                      const size_t* n_local, int scalars_are_montgomery, uint64_t* out_xyz, int* path) {
  return arkhip::capi::msm_sharded_emulated(curve, world, d_bases, d_scalars, n_local, scalars_are_montgomery, out_xyz, path);
}
// ---- scratch poisoning: what survives between calls (scratch_list.hpp names the buffers) ----
// Fill the whole capacity of every scratch buffer of the calling thread's context, and the pinned staging areas, with `word`;
// remember where each buffer stands; reset the high-water marks (DevBuf::asked, MsmJob::pinned_asked).  ARK_HIP_ERR_ARG while an
// MSM job slot is busy: its result would be read out of a poisoned staging area.
int ark_hip_test_scratch_poison(uint32_t word) {
  ARK_SCOPE(sc);
  return scratch_poison(sc.c, word);
}
// One row per scratch buffer (device buffers first, then the pinned areas): what was asked of it since the poison, whether it
// moved, and how many bytes of its slack [asked, cap) no longer hold the poison.  Only the slack is looked at, on the device.
int ark_hip_test_scratch_report(uint32_t word, ark_hip_scratch_row* rows, size_t cap_rows, size_t* n_rows) {
  if (!n_rows || (cap_rows && !rows)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  return scratch_report(sc.c, word, rows, cap_rows, n_rows);
}
// The harness checking itself, with no product kernel involved: 0 when (a) a poisoned cell that nothing wrote reads back as the
// poison and (b) four bytes planted in a buffer's slack -- inside its capacity -- come back as exactly that buffer's
// dirty_beyond == 4 at the planted offset, every other row clean and none regrown.  A positive value names the step that failed.
int ark_hip_test_scratch_selfcheck(void) {
  const uint32_t word = 0x00000001u;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (c->stage_c.ensure(1024)) return ARK_HIP_ERR_NOMEM;
  if (int rc = scratch_poison(c, word)) return rc;
  uint32_t got = 0;
  ARK_HIP_TRY(hipMemcpy(&got, c->stage_c.p, 4, hipMemcpyDeviceToHost));
  if (got != word) return 1;
  if (c->stage_c.ensure(1024)) return ARK_HIP_ERR_NOMEM;   // no growth: the request is only recorded
  const size_t off = c->stage_c.asked + 8;
  if (c->stage_c.asked != 1024 || off + 4 > c->stage_c.cap) return 2;
  const uint32_t planted = ~word;
  ARK_HIP_TRY(hipMemcpy((char*)c->stage_c.p + off, &planted, 4, hipMemcpyHostToDevice));
  size_t n = 0;
  (void)scratch_report(c, word, nullptr, 0, &n);
  std::vector<ark_hip_scratch_row> rows(n);
  if (int rc = scratch_report(c, word, rows.data(), n, &n)) return rc;
  int hits = 0;
  for (const auto& r : rows) {
    if (r.regrown) return 3;
    if (!strcmp(r.name, "stage_c")) {
      if (r.dirty_beyond != 4 || r.first_dirty_offset != off || r.asked != 1024) return 4;
      hits++;
    } else if (r.dirty_beyond) {
      return 5;
    }
  }
  return hits == 1 ? 0 : 6;
}
// One side of a CSR handle read back array by array: what the host-side stable transposition left on the device.  Waits.
int ark_hip_test_csr_dump(const ark_hip_fr_csr* m, int transpose, size_t* dims, uint32_t* row_ptr, size_t row_ptr_cap, uint32_t* col_idx,
                          uint64_t* vals, size_t nnz_cap) {
  const CsrHandle* h = (const CsrHandle*)m;
  if (!h || !dims || (transpose != 0 && transpose != 1) || (transpose && !h->has_t)) return ARK_HIP_ERR_ARG;
  const CsrSide& s = h->side[transpose];
  dims[0] = s.rows;
  dims[1] = s.cols;
  dims[2] = s.nnz;
  if (!row_ptr && !col_idx && !vals) return 0;   // the sizes only
  if (!row_ptr || row_ptr_cap < s.rows + 1 || nnz_cap < s.nnz || (s.nnz && (!col_idx || !vals))) return ARK_HIP_ERR_SIZE;
  Scope sc;
  if (int rc = sc.enter(h->logical)) return rc;
  if (int rc = sync_compute(sc.c)) return rc;
  ARK_HIP_TRY(hipMemcpy(row_ptr, s.csr_ptr.p, (s.rows + 1) * 4, hipMemcpyDeviceToHost));
  if (s.nnz) {
    ARK_HIP_TRY(hipMemcpy(col_idx, s.csr_idx.p, s.nnz * 4, hipMemcpyDeviceToHost));
    ARK_HIP_TRY(hipMemcpy(vals, s.csr_val.p, s.nnz * 32, hipMemcpyDeviceToHost));
  }
  return 0;
}
// ---- the asynchrony contract (tests/test_gpu_async_contract.py) ----
// *busy = 1 while work enqueued on the context stream has not finished: the non-vacuity check of every case (the blocker was
// still running when the host side of the case was done).  Waits for nothing.
int ark_hip_test_context_busy(int* busy) {
  if (!busy) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  const hipError_t e = hipStreamQuery(sc.c->stream);
  if (e != hipSuccess && e != hipErrorNotReady) return -1000 - (int)e;
  if (e == hipErrorNotReady) (void)hipGetLastError();   // "not ready" is the answer, not an error to leave behind
  *busy = e == hipErrorNotReady ? 1 : 0;
  return 0;
}
// the MSM lane (0 or 1) an asynchronous job was enqueued on; host only
int ark_hip_test_job_lane(const ark_hip_msm_job* job, int* lane) {
  const MsmJobHandle* h = (const MsmJobHandle*)job;
  if (!h || !lane || h->slot < 0 || h->slot >= 2 * MSM_JOBS) return ARK_HIP_ERR_ARG;
  *lane = h->slot / MSM_JOBS;
  return 0;
}
// on = 0: mark_producer records no event from here on (process-wide; default on).  The negative control: what a forgotten
// mark looks like.  Host only.
int ark_hip_test_producer_marks(int on) {
  g_producer_marks.store(on != 0, std::memory_order_relaxed);
  return 0;
}
}  // extern "C"
