// C ABI of libark_hip.so: point vectors on the device (pointvec.cuh) -- elementwise scalar multiplication, elementwise sum,
// two-scalar fold (see include/ark_hip.h for the contract and the reference items replaced).
#include "capi_core.hpp"
#include "pointvec.cuh"
using namespace arkhip;
using namespace arkhip::capi;

namespace {
struct Range {
  uintptr_t lo, len;
};
Range range_of(const void* p, size_t bytes) { return Range{(uintptr_t)p, (uintptr_t)bytes}; }
bool overlap(const Range& a, const Range& b) { return a.len && b.len && a.lo < b.lo + b.len && b.lo < a.lo + a.len; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
size_t point_bytes(int curve, int form) { return (size_t)CURVES[curve].fe_words * 8 * (form == ARK_HIP_FORM_AFFINE ? 2 : 3); }
// `out` (n Projective points) against an input of n points in `form`: exact aliasing is allowed for Projective input (a lane reads
// its element before it writes it); any other overlap -- and any overlap with an Affine input, whose elements have another
// stride -- would let a lane overwrite what another lane has yet to read
bool out_ok(int curve, const void* in, int form, const void* out, size_t n) {
  if (form == ARK_HIP_FORM_PROJECTIVE && in == out) return true;
  return !overlap(range_of(in, n * point_bytes(curve, form)), range_of(out, n * point_bytes(curve, ARK_HIP_FORM_PROJECTIVE)));
}
// lanes per launch and the table scratch for them
int tables(Context* c, int curve, int nt, size_t n, size_t* slab) {
  size_t lanes = pv_slab() / (size_t)nt;
  if (lanes > n) lanes = n;
  const size_t bytes = (size_t)nt * 8 * lanes * (size_t)CURVES[curve].fe_words * 32;   // XYZZ entries
  if (c->pointvec_work.cap < bytes) {
    if (int rc = sync_compute(c)) return rc;   // the buffer it replaces may still be read by a launch in flight
    ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  }
  if (c->pointvec_work.ensure(bytes)) return ARK_HIP_ERR_NOMEM;
  *slab = lanes;
  return 0;
}
int mul_args(int curve, const void* points, int form, const void* scalars, size_t n_scalars, int mont, size_t n, const void* out,
             bool device) {
  if (!curve_ops(curve) || (form != ARK_HIP_FORM_AFFINE && form != ARK_HIP_FORM_PROJECTIVE) || mont < 0 || mont > 1)
    return ARK_HIP_ERR_ARG;
  if (n == 0) return n_scalars <= 1 ? 0 : ARK_HIP_ERR_ARG;
  if (n_scalars != 1 && n_scalars != n) return ARK_HIP_ERR_ARG;
  if (!points || !scalars || !out) return ARK_HIP_ERR_ARG;
  if (device && !(aligned16(points) && aligned16(scalars) && aligned16(out))) return ARK_HIP_ERR_ARG;
  if (!out_ok(curve, points, form, out, n)) return ARK_HIP_ERR_ARG;
  if (overlap(range_of(scalars, n_scalars * 32), range_of(out, n * point_bytes(curve, ARK_HIP_FORM_PROJECTIVE)))) return ARK_HIP_ERR_ARG;
  return 0;
}
}  // namespace

extern "C" {

// asynchronous on the context stream
int ark_hip_sw_mul_device(int curve, const void* d_points, int form, const void* d_scalars, size_t n_scalars, int scalars_are_montgomery,
                          size_t n, void* d_out_xyz) {
  if (int rc = mul_args(curve, d_points, form, d_scalars, n_scalars, scalars_are_montgomery, n, d_out_xyz, true)) return rc;
  if (n == 0) return 0;
  const CurveOps* ops = curve_ops(curve);   // served: mul_args
  ARK_SCOPE(sc);
  Context* c = sc.c;
  size_t slab = 0;
  if (int rc = tables(c, curve, 1, n, &slab)) return rc;
  return ops->sw_vec_mul(d_points, form, d_scalars, n_scalars == 1 && n != 1 ? 0 : 8, scalars_are_montgomery, n, d_out_xyz,
                             c->pointvec_work.p, slab, c->stream);
}

// The same for HOST slices: points and scalars go up in chunks (ARK_HIP_POINTVEC_CHUNK_POINTS points each; default: 64 MiB of
// points), one multiplication per chunk, its Projective results come down behind it.  Synchronises before it returns.
int ark_hip_sw_mul(int curve, const uint64_t* points, int form, const uint64_t* scalars, size_t n_scalars, int scalars_are_montgomery,
                   size_t n, uint64_t* out_xyz) {
  if (int rc = mul_args(curve, points, form, scalars, n_scalars, scalars_are_montgomery, n, out_xyz, false)) return rc;
  if (n == 0) return 0;
  const CurveOps* ops = curve_ops(curve);   // served: mul_args
  ARK_SCOPE(sc);
  Context* c = sc.c;
  const size_t pb = point_bytes(curve, form), ob = point_bytes(curve, ARK_HIP_FORM_PROJECTIVE);
  const size_t chunk = stage_chunk_points("ARK_HIP_POINTVEC_CHUNK_POINTS", ob, n);
  const bool shared = n_scalars == 1 && n != 1;
  const size_t sb = shared ? 32 : chunk * 32;
  if (c->stage_a.cap < chunk * pb || c->stage_b.cap < sb || c->stage_c.cap < chunk * ob)
    if (int rc = sync_compute(c)) return rc;
  if (c->stage_a.ensure(chunk * pb) || c->stage_b.ensure(sb) || c->stage_c.ensure(chunk * ob)) return ARK_HIP_ERR_NOMEM;
  size_t slab = 0;
  if (int rc = tables(c, curve, 1, chunk, &slab)) return rc;
  if (shared)
    if (int rc = c->stager.upload(c->stage_b.p, scalars, 32, c->stream)) return rc;
  for (size_t off = 0; off < n; off += chunk) {
    const size_t m = n - off < chunk ? n - off : chunk;
    if (int rc = c->stager.upload(c->stage_a.p, (const char*)points + off * pb, m * pb, c->stream)) return rc;
    if (!shared)
      if (int rc = c->stager.upload(c->stage_b.p, (const char*)scalars + off * 32, m * 32, c->stream)) return rc;
    if (int rc = ops->sw_vec_mul(c->stage_a.p, form, c->stage_b.p, shared ? 0 : 8, scalars_are_montgomery, m, c->stage_c.p,
                                     c->pointvec_work.p, slab, c->stream))
      return rc;
    ARK_HIP_TRY(hipMemcpyAsync((char*)out_xyz + off * ob, c->stage_c.p, m * ob, hipMemcpyDeviceToHost, c->stream));
  }
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// asynchronous on the context stream
int ark_hip_sw_add_device(int curve, const void* d_a_xyz, const void* d_b_xyz, int negate_b, size_t n, void* d_out_xyz) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops || negate_b < 0 || negate_b > 1) return ARK_HIP_ERR_ARG;
  if (n == 0) return 0;
  if (!d_a_xyz || !d_b_xyz || !d_out_xyz || !aligned16(d_a_xyz) || !aligned16(d_b_xyz) || !aligned16(d_out_xyz)) return ARK_HIP_ERR_ARG;
  if (!out_ok(curve, d_a_xyz, ARK_HIP_FORM_PROJECTIVE, d_out_xyz, n) || !out_ok(curve, d_b_xyz, ARK_HIP_FORM_PROJECTIVE, d_out_xyz, n))
    return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  return ops->sw_vec_add(d_a_xyz, d_b_xyz, negate_b, n, d_out_xyz, sc.c->stream);
}

// asynchronous on the context stream (a and b are read before the call returns: they travel as kernel arguments)
int ark_hip_sw_fold_device(int curve, const void* d_lo, const void* d_hi, int form, const uint64_t a[4], const uint64_t b[4],
                           int scalars_are_montgomery, size_t n, void* d_out_xyz) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops || (form != ARK_HIP_FORM_AFFINE && form != ARK_HIP_FORM_PROJECTIVE) || scalars_are_montgomery < 0 ||
      scalars_are_montgomery > 1 || !a || !b)
    return ARK_HIP_ERR_ARG;
  if (n == 0) return 0;
  if (!d_lo || !d_hi || !d_out_xyz || !aligned16(d_lo) || !aligned16(d_hi) || !aligned16(d_out_xyz)) return ARK_HIP_ERR_ARG;
  if (!out_ok(curve, d_lo, form, d_out_xyz, n) || !out_ok(curve, d_hi, form, d_out_xyz, n)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  size_t slab = 0;
  if (int rc = tables(c, curve, 2, n, &slab)) return rc;
  return ops->sw_vec_fold(d_lo, d_hi, form, a, b, scalars_are_montgomery, n, d_out_xyz, c->pointvec_work.p, slab, c->stream);
}

}  // extern "C"
