// C ABI of the one-word prime fields (ark_hip_sfp_*): host arithmetic, domains and the pass plan as pure host code, the
// transforms and pointwise vectors through SmallFieldOps (sfp_internal.hpp).  DESIGN.md section 27.
#include "capi_sfp.hpp"

using namespace arkhip;
using namespace arkhip::capi;

// shared with capi_fri.hip (capi_sfp.hpp)
namespace arkhip {
namespace capi {

const SmallFieldOps* sfp_ops(int sfield) {
#ifndef ARK_HIP_DEV
  switch (sfield) {
    case ARK_HIP_SFP_GOLDILOCKS: return &sfp_ops_GOLDILOCKS();
    case ARK_HIP_SFP_BABYBEAR: return &sfp_ops_BABYBEAR();
    case ARK_HIP_SFP_KOALABEAR: return &sfp_ops_KOALABEAR();
  }
#endif
  (void)sfield;
  return nullptr;
}
namespace {
template <class Cfg>
int host_of(SfpHost* h) {
  using F = SFp<Cfg>;
  using T = typename Cfg::T;
  h->bytes = (int)sizeof(T);
  h->two_adicity = Cfg::TWO_ADICITY;
  h->p = Cfg::P;
  h->one = Cfg::R1;
  h->mul = [](uint64_t a, uint64_t b) -> uint64_t { return F::mul((T)a, (T)b); };
  h->pow = [](uint64_t a, uint64_t e) -> uint64_t { return F::pow((T)a, e); };
  h->from_canonical = [](uint64_t x) -> uint64_t { return F::mul((T)(x % Cfg::P), (T)Cfg::R2); };
  h->root = Cfg::ROOT;
  return 0;
}
}  // namespace
int sfp_host(int sfield, SfpHost* h) {
#define CALL(NAME) host_of<NAME>(h)
  ARK_SFP_SWITCH(sfield, CALL);
#undef CALL
}

int domain_check(const SfpHost& h, const ark_hip_sfp_radix2_domain* dom) {
  if (!dom || dom->log_size_of_group > (uint32_t)h.two_adicity || dom->size != (uint64_t)1 << dom->log_size_of_group)
    return ARK_HIP_ERR_ARG;
  const uint64_t el[7] = {dom->size_as_field_element, dom->size_inv, dom->group_gen, dom->group_gen_inv, dom->offset, dom->offset_inv,
                          dom->offset_pow_size};
  for (uint64_t e : el)
    if (e >= h.p) return ARK_HIP_ERR_ARG;
  return 0;
}

namespace {
SfpPow32 squares_of(const SfpHost& h, uint64_t x) {
  SfpPow32 pw;
  for (int i = 0; i < 32; i++, x = h.mul(x, x)) pw.v[i] = x;
  return pw;
}
}  // namespace

int powers_for(Context* c, int sfield, const SfpHost& h, const SmallFieldOps* ops, int k, uint64_t g, uint64_t scale, SfpScale* out) {
  const int lo_bits = (k + 1) / 2;
  const size_t nhi = (size_t)1 << (k - lo_bits), nlo = (size_t)1 << lo_bits;
  const auto key = std::make_tuple(sfield, k, g, scale);
  auto it = c->sfp.sfp_powers.find(key);
  if (it == c->sfp.sfp_powers.end()) {
    if (c->sfp.sfp_powers.size() >= 256) {   // a caller that walks through offsets: start over (stream order keeps users apart)
      for (auto& kv : c->sfp.sfp_powers) kv.second.release();
      c->sfp.sfp_powers.clear();
    }
    it = c->sfp.sfp_powers.emplace(key, DevBuf()).first;
    int rc = it->second.ensure((nhi + nlo) * h.bytes) ? ARK_HIP_ERR_NOMEM : 0;
    if (!rc) rc = ops->powers(it->second.p, (char*)it->second.p + nhi * h.bytes, nhi, lo_bits, squares_of(h, g), scale, c->stream);
    if (rc) {
      it->second.release();
      c->sfp.sfp_powers.erase(it);
      return rc;
    }
  }
  out->mode = SFP_SCALE_TABLE;
  out->k = 0;
  out->hi = it->second.p;
  out->lo = (const char*)it->second.p + nhi * h.bytes;
  return 0;
}

}  // namespace capi
}  // namespace arkhip

namespace {

template <class Cfg>
int info_of(uint64_t out[8]) {
  out[0] = sizeof(typename Cfg::T);
  out[1] = Cfg::P;
  out[2] = Cfg::K_BITS;
  out[3] = Cfg::R1;
  out[4] = Cfg::R2;
  out[5] = Cfg::GEN_MONT;
  out[6] = Cfg::TWO_ADICITY;
  out[7] = Cfg::ROOT;
  return 0;
}

// the cached per-stage twiddle tables of (sfield, k, direction); built on the stream on first use
int twiddles_for(Context* c, int sfield, const SfpHost& h, const SmallFieldOps* ops, const ark_hip_sfp_radix2_domain* dom, int inverse,
                 const void** out) {
  const int k = (int)dom->log_size_of_group;
  *out = nullptr;
  if (k == 0) return 0;
  const auto key = std::make_tuple(sfield, k, inverse ? 1 : 0);
  auto it = c->sfp.sfp_twiddles.find(key);
  if (it == c->sfp.sfp_twiddles.end()) {
    it = c->sfp.sfp_twiddles.emplace(key, DevBuf()).first;
    if (it->second.ensure(((size_t)1 << k) * h.bytes)) {
      c->sfp.sfp_twiddles.erase(it);
      return ARK_HIP_ERR_NOMEM;
    }
    // the root is the field's own for this size, not the caller's word: the cache key need not hold it
    uint64_t w = h.root;
    for (int i = k; i < h.two_adicity; i++) w = h.mul(w, w);
    if (inverse) w = h.pow(w, h.p - 2);
    if (int rc = ops->twiddles(it->second.p, k, squares_of(h, w), c->stream)) {
      it->second.release();
      c->sfp.sfp_twiddles.erase(it);
      return rc;
    }
  }
  *out = it->second.p;
  return 0;
}
// arguments checked by the caller; enqueues on the context stream
int fft_enqueue(Context* c, int sfield, const SfpHost& h, const SmallFieldOps* ops, const ark_hip_sfp_radix2_domain* dom, void* d_data,
                size_t count, size_t stride, size_t num_coeffs, int inverse) {
  SfpFftArgs f{};
  f.k = (int)dom->log_size_of_group;
  if (!sfp_fft_plan(h.bytes, f.k, &f.plan)) return ARK_HIP_ERR_SIZE;
  const size_t n = (size_t)dom->size;
  f.data = d_data;
  f.count = count;
  f.stride = stride;
  f.num_coeffs = num_coeffs;
  f.lo_bits = (f.k + 1) / 2;
  if (int rc = twiddles_for(c, sfield, h, ops, dom, inverse, &f.tw)) return rc;
  const bool coset = dom->offset != h.one;
  if (!inverse) {
    if (coset)
      if (int rc = powers_for(c, sfield, h, ops, f.k, dom->offset, h.one, &f.pre)) return rc;
  } else if (coset) {
    if (int rc = powers_for(c, sfield, h, ops, f.k, dom->offset_inv, dom->size_inv, &f.post)) return rc;
  } else {
    f.post.mode = SFP_SCALE_CONST;
    f.post.k = dom->size_inv;
  }
  if (f.plan.npasses > 1) {
    if (count > (~(size_t)0 / h.bytes) / n) return ARK_HIP_ERR_SIZE;
    if (c->sfp.sfp_ping.cap < count * n * h.bytes)
      if (int rc = sync_compute(c)) return rc;   // the buffer is about to be replaced: nothing may still use the old one
    if (c->sfp.sfp_ping.ensure(count * n * h.bytes)) return ARK_HIP_ERR_NOMEM;
    f.ping = c->sfp.sfp_ping.p;
  }
  return ops->fft(f, c->stream);
}

int vec_entry(int sfield, int op, const void* d_a, const void* d_b, uint64_t k, void* d_r, size_t n) {
  SfpHost h;
  if (sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  const SmallFieldOps* ops = sfp_ops(sfield);
  if (!ops) return ARK_HIP_ERR_ARG;
  const bool binary = op == SFP_OP_ADD || op == SFP_OP_SUB || op == SFP_OP_MUL;
  if (n > 0 && (!d_a || !d_r || (binary && !d_b))) return ARK_HIP_ERR_ARG;
  if (op == SFP_OP_SCALE && k >= h.p) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  if (n == 0) return 0;
  if (int rc = ops->vec_op(op, d_a, d_b, k, d_r, n, sc.c->stream)) return rc;
  return mark_producer(sc.c);
}

}  // namespace

extern "C" {

int ark_hip_sfp_info(int sfield, uint64_t out[8]) {
  if (!out) return ARK_HIP_ERR_ARG;
#define CALL(NAME) info_of<NAME>(out)
  ARK_SFP_SWITCH(sfield, CALL);
#undef CALL
}

int ark_hip_sfp_pow(int sfield, uint64_t base, uint64_t exp, uint64_t* out) {
  SfpHost h;
  if (!out || sfp_host(sfield, &h) || base >= h.p) return ARK_HIP_ERR_ARG;
  *out = h.pow(base, exp);
  return 0;
}

int ark_hip_sfp_radix2_domain_new(int sfield, size_t num_coeffs, ark_hip_sfp_radix2_domain* out) {
  SfpHost h;
  if (!out || sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  // checked_next_power_of_two: 0 and 1 give 1; nothing above 2^63 has one
  int log = 0;
  while (log < 64 && ((uint64_t)1 << log) < (uint64_t)num_coeffs) log++;
  if (log > h.two_adicity) return ARK_HIP_ERR_SIZE;
  const uint64_t size = (uint64_t)1 << log;
  uint64_t w = h.root;                       // get_root_of_unity: square the two-adic root down to the size
  for (int i = log; i < h.two_adicity; i++) w = h.mul(w, w);
  out->size = size;
  out->log_size_of_group = (uint32_t)log;
  out->_pad = 0;
  out->size_as_field_element = h.from_canonical(size);
  out->size_inv = h.pow(out->size_as_field_element, h.p - 2);
  out->group_gen = w;
  out->group_gen_inv = h.pow(w, h.p - 2);
  out->offset = out->offset_inv = out->offset_pow_size = h.one;
  return 0;
}

int ark_hip_sfp_radix2_domain_get_coset(int sfield, const ark_hip_sfp_radix2_domain* dom, uint64_t offset,
                                        ark_hip_sfp_radix2_domain* out) {
  SfpHost h;
  if (!out || sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  if (int rc = domain_check(h, dom)) return rc;
  if (offset == 0 || offset >= h.p) return ARK_HIP_ERR_ARG;
  ark_hip_sfp_radix2_domain d = *dom;
  d.offset = offset;
  d.offset_inv = h.pow(offset, h.p - 2);
  d.offset_pow_size = h.pow(offset, d.size);
  *out = d;
  return 0;
}

int ark_hip_sfp_fft_plan(int sfield, unsigned log_n, int out[8]) {
  SfpHost h;
  if (!out || sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  if (log_n > (unsigned)h.two_adicity) return ARK_HIP_ERR_SIZE;
  SfpPlan pl;
  if (!sfp_fft_plan(h.bytes, (int)log_n, &pl)) return ARK_HIP_ERR_SIZE;
  out[0] = pl.single_log;
  out[1] = pl.tile_log;
  out[2] = pl.seg_log;
  out[3] = pl.npasses;
  for (int i = 0; i < SFP_MAX_PASSES; i++) out[4 + i] = pl.stages[i];
  return 0;
}

int ark_hip_sfp_fft_batch_device(int sfield, const ark_hip_sfp_radix2_domain* dom, void* d_data, size_t count, size_t stride,
                                 size_t num_coeffs, int inverse) {
  SfpHost h;
  if (sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  const SmallFieldOps* ops = sfp_ops(sfield);
  if (!ops || !d_data) return ARK_HIP_ERR_ARG;
  if (int rc = domain_check(h, dom)) return rc;
  if (stride < dom->size || num_coeffs < 1 || num_coeffs > dom->size || (inverse && num_coeffs != dom->size)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  if (count == 0) return 0;
  if (int rc = fft_enqueue(sc.c, sfield, h, ops, dom, d_data, count, stride, num_coeffs, inverse)) return rc;
  return mark_producer(sc.c);
}

int ark_hip_sfp_fft_in_place(int sfield, const ark_hip_sfp_radix2_domain* dom, void* host_data, int inverse) {
  SfpHost h;
  if (sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  const SmallFieldOps* ops = sfp_ops(sfield);
  if (!ops || !host_data) return ARK_HIP_ERR_ARG;
  if (int rc = domain_check(h, dom)) return rc;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  const size_t n = (size_t)dom->size, bytes = n * h.bytes;
  if (c->stage_a.cap < bytes)
    if (int rc = sync_compute(c)) return rc;
  if (c->stage_a.ensure(bytes)) return ARK_HIP_ERR_NOMEM;
  if (int rc = c->stager.upload(c->stage_a.p, host_data, bytes, c->stream)) return rc;
  if (int rc = fft_enqueue(c, sfield, h, ops, dom, c->stage_a.p, 1, n, n, inverse)) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  ARK_HIP_TRY(hipMemcpyAsync(host_data, c->stage_a.p, bytes, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int ark_hip_sfp_add_device(int sfield, const void* d_a, const void* d_b, void* d_r, size_t n) {
  return vec_entry(sfield, SFP_OP_ADD, d_a, d_b, 0, d_r, n);
}
int ark_hip_sfp_sub_device(int sfield, const void* d_a, const void* d_b, void* d_r, size_t n) {
  return vec_entry(sfield, SFP_OP_SUB, d_a, d_b, 0, d_r, n);
}
int ark_hip_sfp_mul_device(int sfield, const void* d_a, const void* d_b, void* d_r, size_t n) {
  return vec_entry(sfield, SFP_OP_MUL, d_a, d_b, 0, d_r, n);
}
int ark_hip_sfp_neg_device(int sfield, const void* d_a, void* d_r, size_t n) {
  return vec_entry(sfield, SFP_OP_NEG, d_a, nullptr, 0, d_r, n);
}
int ark_hip_sfp_inverse_device(int sfield, const void* d_a, void* d_r, size_t n) {
  return vec_entry(sfield, SFP_OP_INVERSE, d_a, nullptr, 0, d_r, n);
}
int ark_hip_sfp_scale_device(int sfield, const void* d_a, uint64_t k, void* d_r, size_t n) {
  return vec_entry(sfield, SFP_OP_SCALE, d_a, nullptr, k, d_r, n);
}
int ark_hip_sfp_from_canonical_device(int sfield, const void* d_a, void* d_r, size_t n) {
  return vec_entry(sfield, SFP_OP_FROM_CANONICAL, d_a, nullptr, 0, d_r, n);
}
int ark_hip_sfp_into_canonical_device(int sfield, const void* d_a, void* d_r, size_t n) {
  return vec_entry(sfield, SFP_OP_INTO_CANONICAL, d_a, nullptr, 0, d_r, n);
}

}  // extern "C"
