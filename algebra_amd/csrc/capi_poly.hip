// C ABI of libark_hip.so: polynomial operations on device-resident vectors -- evaluation at a point, division by x - z and
// by the vanishing polynomial of a domain, the Lagrange coefficients of a domain at a point, inner products, prefix products,
// prefix sums and ratio accumulators (prefixscan.cuh) -- and dense
// multilinear extensions: fix_variables, evaluate, relabel, a + k x, the eq table and an opening's quotients -- and the
// sumcheck prover's round over such tables, the product tree of a grand product and its fingerprints, the fraction tree and the
// multiplicities of a lookup (from indices, and from the values themselves: lookup.cuh), the Fiat-Shamir transcript and the whole sumcheck proof in one wait, and the gate expression of a
// univariate prover: sums of products of columns read at rotations (see include/ark_hip.h;
// kernels: polyops.cuh, mle.cuh, mle_open.cuh, sumcheck.cuh, transcript.cuh, grand_product.cuh, fraction_sum.cuh, gateexpr.cuh).
#include "capi_core.hpp"
#include "capi_hostmath.hpp"
#include "polyops.cuh"
#include "prefixscan.cuh"
#include "mle.cuh"
#include "mle_open.cuh"
#include "grand_product.cuh"
#include "fraction_sum.cuh"
#include "lookup.cuh"
#include "sumcheck.cuh"
#include "gateexpr.cuh"
using namespace arkhip;
using namespace arkhip::capi;

namespace {

constexpr int POLY_MAX_LEVELS = 8;   // 2048^6 > 2^64

template <class FP>
FrConst to_const(const Fp<FP>& x) {
  FrConst k;
  for (int j = 0; j < 8; j++) k.l[j] = x.l[j];
  return k;
}
// the powers every scan level needs, by repeated squaring on the host: level l works with z_l = z^(T^l)
template <class FP>
void poly_powers(const uint64_t* z4, int levels, PolyPowers* pw) {
  typedef Fp<FP> F;
  F z = F::load(z4);
  for (int l = 0; l < levels; l++) {
    pw[l].z = to_const(z);
    F t = z;
    int lg = 0;
    for (int e = 1; e < POLY_TILE; e <<= 1, lg++) {   // t = z^e on entry
      if (e >= POLY_E) pw[l].zs[lg - 3] = to_const(t);
      t = F::sqr(t);
    }
    z = t;   // z^T
  }
}
inline int poly_powers_any(int field, const uint64_t* z4, int levels, PolyPowers* pw) {
#define X(NAME) (poly_powers<NAME>(z4, levels, pw), 0)
  ARK_FIELD_SWITCH(field, X);
#undef X
}

// scratch of one call inside Context::poly_work: [result slot | tile values of level 1 | level 2 | ...]
struct PolyLevels {
  int levels = 1;
  size_t len[POLY_MAX_LEVELS] = {};   // coefficients at level l
  size_t off[POLY_MAX_LEVELS] = {};   // element offset of level l's vector in the scratch (l >= 1)
  size_t total = 1;                   // elements of scratch
};
inline PolyLevels poly_levels(size_t n) {
  PolyLevels L;
  L.len[0] = n;
  while (L.len[L.levels - 1] > (size_t)POLY_TILE) {
    L.len[L.levels] = (L.len[L.levels - 1] + POLY_TILE - 1) / POLY_TILE;
    L.off[L.levels] = L.total;
    L.total += L.len[L.levels];
    L.levels++;
  }
  return L;
}
// grows only with every stream idle: earlier asynchronous calls may still be using the buffer
inline int poly_scratch(Context* c, size_t elems) {
  if (c->poly_work.cap < elems * 32)
    if (int rc = sync_compute(c)) return rc;
  return c->poly_work.ensure(elems * 32) ? ARK_HIP_ERR_NOMEM : 0;
}
inline int result_to_host(Context* c, uint64_t* out) {
  ARK_HIP_TRY(hipMemcpyAsync(out, c->poly_work.p, 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

template <class FP>
int lagrange_constants(const ark_hip_radix2_domain* dom, const uint64_t* tau4, size_t lanes, uint64_t a4[4], uint64_t c4[4],
                       uint64_t w4[4], uint64_t wstep4[4], int* onehot) {
  typedef Fp<FP> F;
  const F tau = F::load(tau4), h = F::load(dom->offset);
  uint64_t e[1] = {dom->size};
  const F zh = F::sub(host_pow<FP>(tau, e, 1), F::load(dom->offset_pow_size));   // Z_H(tau) = tau^m - h^m
  uint64_t le[1] = {(uint64_t)lanes};
  if (zh.is_zero()) {   // tau = h g^i for one i: that coefficient is one, the others are zero (domain/mod.rs:175-189)
    const F g = F::load(dom->group_gen);
    h.store(a4);
    tau.store(c4);
    g.store(w4);
    host_pow<FP>(g, le, 1).store(wstep4);
    *onehot = 1;
    return 0;
  }
  // 1 / L_i = l_i r_i with l_i = l_0 g^-i, l_0 = m h^(m-1) / Z_H(tau), r_i = tau - h g^i (:204-215)
  //         = (l_0 tau) g^-i - l_0 h
  uint64_t em[1] = {dom->size - 1};
  const F l0 = F::mul(host_inverse(zh), F::mul(F::load(dom->size_as_field_element), host_pow<FP>(h, em, 1)));
  const F gi = F::load(dom->group_gen_inv);
  F::mul(l0, tau).store(a4);
  F::mul(l0, h).store(c4);
  gi.store(w4);
  host_pow<FP>(gi, le, 1).store(wstep4);
  *onehot = 0;
  return 0;
}

// the launches that bind dim variables of a 2^num_vars table, shared by fix_variables and evaluate: the intermediate tables
// live in Context::poly_work behind the result slot, the last launch writes `last` (nullptr: the result slot)
inline int mle_fold_run(Context* c, const FieldOps* ops, const void* d_evals, unsigned num_vars, const uint64_t* point, unsigned dim, void* last) {
  int widths[MLE_MAX_PASSES];
  const int passes = mle_fold_passes((int)dim, widths);
  size_t scratch = 1;
  for (int p = 0, m = (int)num_vars; p + 1 < passes; p++) scratch += (size_t)1 << (m -= widths[p]);
  if (int rc = poly_scratch(c, scratch)) return rc;
  char* w = (char*)c->poly_work.p + 32;
  const void* cur = d_evals;
  int m = (int)num_vars;
  for (int p = 0; p < passes; p++) {
    MlePoint pt = {};
    for (int j = 0; j < widths[p]; j++, point += 4)
      for (int q = 0; q < 4; q++) { pt.r[j].l[2 * q] = (u32)point[q]; pt.r[j].l[2 * q + 1] = (u32)(point[q] >> 32); }
    void* dst = p + 1 < passes ? (void*)w : last ? last : c->poly_work.p;
    if (int rc = ops->mle_fold(cur, m, widths[p], pt, dst, c->stream)) return rc;
    m -= widths[p];
    w += ((size_t)1 << m) * 32;
    cur = dst;
  }
  return 0;
}
inline void mle_point_fill(MlePoint& pt, const uint64_t* point, int w) {
  for (int j = 0; j < w; j++, point += 4)
    for (int q = 0; q < 4; q++) { pt.r[j].l[2 * q] = (u32)point[q]; pt.r[j].l[2 * q + 1] = (u32)(point[q] >> 32); }
}
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

static_assert(SUMCHECK_MAX_TABLES == ARK_HIP_SUMCHECK_MAX_TABLES && SUMCHECK_MAX_TERMS == ARK_HIP_SUMCHECK_MAX_TERMS &&
                  SUMCHECK_MAX_DEGREE == ARK_HIP_SUMCHECK_MAX_DEGREE, "the header publishes the kernels' limits");
static_assert(SUMCHECK_TAIL_MAX_VARS == ARK_HIP_SUMCHECK_TAIL_MAX_VARS, "the header publishes the tail's ceiling");
static_assert(PROD_TREE_MAX_W == ARK_HIP_PRODUCT_TREE_LEVELS, "the header publishes the levels of a full launch");
static_assert(FRAC_TREE_MAX_W == ARK_HIP_FRACTION_TREE_LEVELS || FRAC_TREE_VARIANT_BUILD, "the header publishes the levels of a full launch");
// the field's one (R mod p) as a host element
template <class FP>
int fr_one(uint64_t* out) {
  Fp<FP>::one().store(out);
  return 0;
}
inline int fr_one_any(int field, uint64_t* out) {
#define X(NAME) fr_one<NAME>(out)
  ARK_FIELD_SWITCH(field, X);
#undef X
}


// The scan of a device vector under one monoid (prefixscan.cuh), reduce-then-scan: the tile totals of every level that has more
// than one tile go up through `w` (room for poly_levels(n).total - 1 elements: [level 1 | level 2 | ...]), each is scanned
// exclusively in place on the way down and is then the carries of the level below it.  The top level is one tile; its launch
// writes the total of the whole vector to `total` when that is not null.  dst may be src.
inline int scan_run(Context* c, const FieldOps* ops, int op, const void* src, size_t n, int exclusive, void* dst, void* total, char* w) {
  const PolyLevels L = poly_levels(n);
  auto vec = [&](int l) -> char* { return w + (L.off[l] - 1) * 32; };   // l >= 1
  for (int l = 0; l + 1 < L.levels; l++)
    if (int rc = ops->scan_tile_total(op, l == 0 ? src : vec(l), L.len[l], vec(l + 1), c->stream)) return rc;
  for (int l = L.levels - 1; l >= 0; l--) {
    const void* carries = l + 1 < L.levels ? vec(l + 1) : nullptr;
    void* tot = l == L.levels - 1 ? total : nullptr;
    if (int rc = ops->scan_tile(op, l == 0 ? src : vec(l), L.len[l], carries, l == 0 ? exclusive : 1, l == 0 ? dst : vec(l), tot, c->stream))
      return rc;
  }
  return 0;
}
// ark_hip_fr_prefix_product_device / _sum_device
inline int prefix_scan_entry(int op, int field, const void* d_a, size_t n, int exclusive, void* d_out, uint64_t* out_total) {
  const FieldOps* ops = field_ops(field);
  if (!ops || (n && (!d_a || !d_out)) || n > ((size_t)-1) / 32) return ARK_HIP_ERR_ARG;
  if (n && d_out != d_a && ranges_overlap(d_a, n * 32, d_out, n * 32)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) {   // the empty product is one, the empty sum zero
    if (!out_total) return 0;
    if (op == SCAN_OP_PRODUCT) return fr_one_any(field, out_total);
    memset(out_total, 0, 32);
    return 0;
  }
  const PolyLevels L = poly_levels(n);
  if (int rc = poly_scratch(c, L.total)) return rc;
  char* w = (char*)c->poly_work.p;
  if (int rc = scan_run(c, ops, op, d_a, n, exclusive ? 1 : 0, d_out, out_total ? (void*)w : nullptr, w + 32)) return rc;
  if (out_total) return result_to_host(c, out_total);
  return mark_producer(c);
}

// the terms of a sumcheck call, checked: shared by the round entry and the whole-proof entry
inline int sumcheck_terms(int field, unsigned ntables, const unsigned* term_len, const unsigned* term_tables, const uint64_t* coeffs,
                          unsigned nterms, SumcheckTerms* tm) {
  tm->ntables = ntables;
  tm->nterms = nterms;
  for (unsigned j = 0, at = 0; j < nterms; j++) {
    const unsigned len = term_len[j];
    if (len == 0 || len > (unsigned)SUMCHECK_MAX_DEGREE) return ARK_HIP_ERR_ARG;
    tm->len[j] = len;
    if (len > tm->degree) tm->degree = len;
    for (unsigned q = 0; q < len; q++, at++) {
      if (term_tables[at] >= ntables) return ARK_HIP_ERR_ARG;
      tm->tab[j] |= term_tables[at] << (8 * q);
    }
    for (int q = 0; q < 4; q++) { tm->coeff[j].l[2 * q] = (u32)coeffs[4 * j + q]; tm->coeff[j].l[2 * q + 1] = (u32)(coeffs[4 * j + q] >> 32); }
    if (field_is_one(field, coeffs + 4 * j)) tm->unit |= 1u << j;
  }
  return 0;
}
// the whole proof: where the tail takes over, and the two alternating sets of bound tables (halves and quarters) in d_work
inline int prove_tail_from(unsigned num_vars, int tail_vars) {
  const int t = tail_vars < 0 ? SUMCHECK_TAIL_DEFAULT_VARS : tail_vars;
  return t > (int)num_vars ? (int)num_vars : t;
}
inline size_t prove_work_elems(unsigned num_vars, unsigned ntables) {
  return (size_t)ntables * (((size_t)1 << (num_vars - 1)) + ((size_t)1 << (num_vars >= 2 ? num_vars - 2 : 0)));
}
// the transcript's one operation on the host: msg holds the state and room for the elements
template <class FP>
int transcript_host(u32* msg, const uint64_t* elements, unsigned count, uint64_t* out) {
  typedef Fp<FP> F;
  for (unsigned i = 0; i < count; i++) transcript_put_element<F>(msg, i, F::load(elements + 4 * (size_t)i));
  transcript_challenge_words<F>(msg, count).store(out);
  return 0;
}
inline int transcript_host_any(int field, u32* msg, const uint64_t* elements, unsigned count, uint64_t* out) {
#define X(NAME) transcript_host<NAME>(msg, elements, count, out)
  ARK_FIELD_SWITCH(field, X);
#undef X
}
}  // namespace

extern "C" {

int ark_hip_prefix_scan_plan(int op, size_t n, int* tile, int* levels) {
  if (!tile || !levels || op < SCAN_OP_PRODUCT || op > SCAN_OP_RATIO) return ARK_HIP_ERR_ARG;
  *tile = POLY_TILE;   // the ratio's two tiles pass through LDS one after the other: the same tile for every op
  *levels = poly_scan_levels(n);
  return 0;
}

int ark_hip_fr_prefix_product_device(int field, const void* d_a, size_t n, int exclusive, void* d_out, uint64_t* out_total) {
  return prefix_scan_entry(SCAN_OP_PRODUCT, field, d_a, n, exclusive, d_out, out_total);
}

int ark_hip_fr_prefix_sum_device(int field, const void* d_a, size_t n, int exclusive, void* d_out, uint64_t* out_total) {
  return prefix_scan_entry(SCAN_OP_SUM, field, d_a, n, exclusive, d_out, out_total);
}

int ark_hip_fr_prefix_ratio_device(int field, const void* d_num, const void* d_den, size_t n, void* d_out, uint64_t* out_last) {
  const FieldOps* ops = field_ops(field);
  if (!ops || (n && (!d_num || !d_den || !d_out)) || n > ((size_t)-1) / 32) return ARK_HIP_ERR_ARG;
  if (n && d_out != d_num && ranges_overlap(d_num, n * 32, d_out, n * 32)) return ARK_HIP_ERR_ARG;
  if (n && d_out != d_den && ranges_overlap(d_den, n * 32, d_out, n * 32)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) return out_last ? fr_one_any(field, out_last) : 0;
  // [result slot | CN: the tile products of num and the levels of their scan | CD: the same for den | the inverses of CD]
  const size_t tiles = (n + POLY_TILE - 1) / POLY_TILE;
  const size_t per = tiles + (poly_levels(tiles).total - 1);
  if (int rc = poly_scratch(c, 1 + 2 * per + tiles)) return rc;
  char* w = (char*)c->poly_work.p;
  char *cn = w + 32, *cd = cn + per * 32, *icd = cd + per * 32;
  if (tiles > 1) {   // the product of num before every tile: a single tile starts from one
    if (int rc = ops->scan_tile_total(SCAN_OP_PRODUCT, d_num, n, cn, c->stream)) return rc;
    if (int rc = scan_run(c, ops, SCAN_OP_PRODUCT, cn, tiles, 1, cn, nullptr, cn + tiles * 32)) return rc;
  }
  // the product of den through every tile, and ONE inversion per tile (zero for zero)
  if (int rc = ops->scan_tile_total(SCAN_OP_PRODUCT, d_den, n, cd, c->stream)) return rc;
  if (tiles > 1)
    if (int rc = scan_run(c, ops, SCAN_OP_PRODUCT, cd, tiles, 0, cd, nullptr, cd + tiles * 32)) return rc;
  if (int rc = ops->fr_div(nullptr, cd, icd, tiles, c->stream)) return rc;
  if (int rc = ops->ratio_tile(d_num, d_den, n, tiles > 1 ? cn : nullptr, cd, icd, d_out, out_last ? (void*)w : nullptr, c->stream)) return rc;
  if (out_last) return result_to_host(c, out_last);
  return mark_producer(c);
}

int ark_hip_poly_scan_plan(size_t n, int* tile, int* levels) {
  if (!tile || !levels) return ARK_HIP_ERR_ARG;
  *tile = POLY_TILE;
  *levels = poly_scan_levels(n);
  return 0;
}

int ark_hip_poly_evaluate_device(int field, const void* d_coeffs, size_t n, const uint64_t* point, uint64_t* out) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !point || !out || (n && !d_coeffs)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) {
    memset(out, 0, 32);
    return 0;
  }
  const PolyLevels L = poly_levels(n);
  PolyPowers pw[POLY_MAX_LEVELS];
  if (int rc = poly_powers_any(field, point, L.levels, pw)) return rc;
  if (int rc = poly_scratch(c, L.total)) return rc;
  char* w = (char*)c->poly_work.p;
  const void* cur = d_coeffs;
  for (int l = 0; l < L.levels; l++) {   // the last level has one tile: its value is p(z), written to the result slot
    void* vals = l + 1 < L.levels ? w + L.off[l + 1] * 32 : w;
    if (int rc = ops->poly_tile_value(cur, L.len[l], pw[l], vals, c->stream)) return rc;
    cur = vals;
  }
  return result_to_host(c, out);
}

int ark_hip_poly_divide_linear_device(int field, const void* d_coeffs, size_t n, const uint64_t* z, void* d_quot, uint64_t* out_rem) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !z || (n && !d_coeffs) || (n > 1 && !d_quot)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) {
    if (out_rem) memset(out_rem, 0, 32);
    return 0;
  }
  const PolyLevels L = poly_levels(n);
  PolyPowers pw[POLY_MAX_LEVELS];
  if (int rc = poly_powers_any(field, z, L.levels, pw)) return rc;
  if (int rc = poly_scratch(c, L.total)) return rc;
  char* w = (char*)c->poly_work.p;
  auto vec = [&](int l) -> void* { return l == 0 ? const_cast<void*>(d_coeffs) : (void*)(w + L.off[l] * 32); };
  // up: tile values of every level that has more than one tile
  for (int l = 0; l + 1 < L.levels; l++)
    if (int rc = ops->poly_tile_value(vec(l), L.len[l], pw[l], vec(l + 1), c->stream)) return rc;
  // down: the top level is one tile with no carry; every level's quotient is the carries of the level below it, written
  // over its own tile values (the last one stays: the last tile's carry is zero by definition)
  for (int l = L.levels - 1; l >= 0; l--) {
    const void* carries = l + 1 < L.levels ? vec(l + 1) : nullptr;
    void* dst = l == 0 ? d_quot : vec(l);
    void* rem = (l == 0 && out_rem) ? (void*)w : nullptr;
    if (int rc = ops->poly_tile_divide(vec(l), L.len[l], pw[l], carries, dst, rem, c->stream)) return rc;
  }
  if (out_rem) return result_to_host(c, out_rem);
  return mark_producer(c);
}

int ark_hip_poly_divide_by_vanishing_device(int field, size_t domain_size, const void* d_coeffs, size_t n, void* d_quot, void* d_rem) {
  const FieldOps* ops = field_ops(field);
  if (!ops || domain_size == 0 || (n && (!d_coeffs || !d_rem)) || (n > domain_size && !d_quot)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) return 0;
  if (n < domain_size) {   // the quotient is zero and the whole polynomial is the remainder (dense.rs:171-173)
    ARK_HIP_TRY(hipMemcpyAsync(d_rem, d_coeffs, n * 32, hipMemcpyDeviceToDevice, c->stream));
    return mark_producer(c);
  }
  if (int rc = ops->poly_vanishing(d_coeffs, n, domain_size, d_quot, d_rem, c->stream)) return rc;
  return mark_producer(c);
}

int ark_hip_domain_lagrange_coefficients_device(int field, const ark_hip_radix2_domain* dom, const uint64_t* tau, void* d_out) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !dom || !tau || !d_out) return ARK_HIP_ERR_ARG;
  if (dom->log_size_of_group > 63 || dom->size != ((uint64_t)1 << dom->log_size_of_group)) return ARK_HIP_ERR_ARG;
  if (!domain_is_of_field(field, dom)) return ARK_HIP_ERR_ARG;
  const size_t n = (size_t)dom->size;
  const size_t lanes = poly_lagrange_lanes(n);   // the kernel's partition: the host supplies its step w^lanes
  uint64_t a4[4], c4[4], w4[4], ws4[4];
  int onehot = 0;
  {
    int rc = ARK_HIP_ERR_ARG;
    switch (field) {
#ifndef ARK_HIP_DEV
      case ARK_HIP_BN254_FR: rc = lagrange_constants<BN254_FR>(dom, tau, lanes, a4, c4, w4, ws4, &onehot); break;
      case ARK_HIP_BLS12_377_FR: rc = lagrange_constants<BLS12_377_FR>(dom, tau, lanes, a4, c4, w4, ws4, &onehot); break;
#endif
      case ARK_HIP_BLS12_381_FR: rc = lagrange_constants<BLS12_381_FR>(dom, tau, lanes, a4, c4, w4, ws4, &onehot); break;
    }
    if (rc) return rc;
  }
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (int rc = ops->poly_lagrange(a4, c4, w4, ws4, onehot, d_out, n, lanes, c->stream)) return rc;
  // batch_inversion of the inverse coefficients (domain/mod.rs:219), lane-batched in place
  if (!onehot)
    if (int rc = ops->fr_div(nullptr, d_out, d_out, n, c->stream)) return rc;
  return mark_producer(c);
}

int ark_hip_fr_inner_product_device(int field, const void* d_a, const void* d_b, size_t n, uint64_t* out) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !out || (n && (!d_a || !d_b))) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) {
    memset(out, 0, 32);
    return 0;
  }
  if (int rc = poly_scratch(c, 1 + INNER_BLOCKS)) return rc;
  char* w = (char*)c->poly_work.p;
  if (int rc = ops->fr_inner_product(d_a, d_b, n, w + 32, w, c->stream)) return rc;
  return result_to_host(c, out);
}

int ark_hip_mle_fold_plan(unsigned num_vars, unsigned dim, int* tile_log, int* passes, int* widths) {
  if (!tile_log || !passes || !widths || num_vars >= 64 || dim > num_vars) return ARK_HIP_ERR_ARG;
  *tile_log = MLE_TILE_LOG;
  for (int p = 0; p < MLE_MAX_PASSES; p++) widths[p] = 0;
  *passes = mle_fold_passes((int)dim, widths);
  return 0;
}

int ark_hip_mle_fold_tiles(unsigned num_vars, unsigned dim, int* tiles_log) {
  if (!tiles_log || num_vars >= 64 || dim > num_vars) return ARK_HIP_ERR_ARG;
  int widths[MLE_MAX_PASSES];
  const int passes = mle_fold_passes((int)dim, widths);
  for (int p = 0, m = (int)num_vars; p < MLE_MAX_PASSES; p++) {
    tiles_log[p] = p < passes ? mle_fold_group_log(m, widths[p]) : 0;
    if (p < passes) m -= widths[p];
  }
  return 0;
}

int ark_hip_mle_fix_variables_device(int field, const void* d_evals, unsigned num_vars, const uint64_t* partial_point, unsigned dim,
                                     void* d_out) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_evals || !d_out || num_vars >= 64 || dim > num_vars || (dim && !partial_point)) return ARK_HIP_ERR_ARG;
  if (num_vars > 58) return ARK_HIP_ERR_ARG;   // the table's bytes must fit a size_t
  const size_t n = (size_t)1 << num_vars, n_out = n >> dim;
  if (ranges_overlap(d_evals, n * 32, d_out, n_out * 32)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (dim == 0) {
    ARK_HIP_TRY(hipMemcpyAsync(d_out, d_evals, n * 32, hipMemcpyDeviceToDevice, c->stream));
    return mark_producer(c);
  }
  if (int rc = mle_fold_run(c, ops, d_evals, num_vars, partial_point, dim, d_out)) return rc;
  return mark_producer(c);
}

int ark_hip_mle_evaluate_device(int field, const void* d_evals, unsigned num_vars, const uint64_t* point, uint64_t* out) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_evals || !out || num_vars >= 64 || (num_vars && !point)) return ARK_HIP_ERR_ARG;
  if (num_vars > 58) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (num_vars == 0) {   // a constant: its one table entry
    ARK_HIP_TRY(hipMemcpyAsync(out, d_evals, 32, hipMemcpyDeviceToHost, c->stream));
    ARK_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  }
  if (int rc = mle_fold_run(c, ops, d_evals, num_vars, point, num_vars, nullptr)) return rc;
  return result_to_host(c, out);
}

int ark_hip_mle_eq_plan(unsigned num_vars, int* tile_log, int* passes, int* widths, int* tiles_log) {
  if (!tile_log || !passes || !widths || !tiles_log || num_vars >= 64) return ARK_HIP_ERR_ARG;
  *tile_log = MLE_TILE_LOG;
  for (int p = 0; p < MLE_MAX_PASSES; p++) widths[p] = tiles_log[p] = 0;
  *passes = mle_eq_passes((int)num_vars, widths);
  for (int p = 0, m = 0; p < *passes; p++) tiles_log[p] = mle_eq_group_log(m += widths[p]);
  return 0;
}

int ark_hip_mle_eq_table_device(int field, const uint64_t* point, unsigned num_vars, const uint64_t* scale, void* d_out) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_out || num_vars >= 64 || (num_vars && !point)) return ARK_HIP_ERR_ARG;
  if (num_vars > 58) return ARK_HIP_ERR_ARG;   // the table's bytes must fit a size_t
  int widths[MLE_MAX_PASSES];
  const int passes = mle_eq_passes((int)num_vars, widths);
  FrConst top = {};
  if (scale)
    for (int q = 0; q < 4; q++) { top.l[2 * q] = (u32)scale[q]; top.l[2 * q + 1] = (u32)(scale[q] >> 32); }
  ARK_SCOPE(sc);
  Context* c = sc.c;
  // [result slot (unused) | the table of the top widths[0] variables | of the top widths[0] + widths[1] | ...]
  size_t scratch = 1;
  for (int p = 0, m = 0; p + 1 < passes; p++) scratch += (size_t)1 << (m += widths[p]);
  if (int rc = poly_scratch(c, scratch)) return rc;
  char* w = (char*)c->poly_work.p + 32;
  const void* hi = nullptr;
  for (int p = 0, m = 0; p < passes; p++) {
    m += widths[p];
    MlePoint pt = {};   // zeros for the variables a short launch lacks
    mle_point_fill(pt, point + 4 * ((size_t)num_vars - m), widths[p]);
    void* dst = p + 1 < passes ? (void*)w : d_out;
    if (int rc = ops->mle_eq(hi, top, scale ? 0 : 1, pt, m, dst, c->stream)) return rc;
    w += ((size_t)1 << m) * 32;
    hi = dst;
  }
  return mark_producer(c);
}

int ark_hip_mle_quotients_plan(unsigned num_vars, int* tile_log, int* passes, int* widths, int* tiles_log) {
  if (!tile_log || !passes || !widths || !tiles_log || num_vars >= 64) return ARK_HIP_ERR_ARG;
  *tile_log = MLE_TILE_LOG;
  for (int p = 0; p < MLE_MAX_PASSES; p++) widths[p] = tiles_log[p] = 0;   // a wave of the quotient kernel takes one tile
  *passes = mle_fold_passes((int)num_vars, widths);
  return 0;
}

int ark_hip_mle_quotients_device(int field, const void* d_evals, unsigned num_vars, const uint64_t* point, void* d_quot,
                                 uint64_t* out_value) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_evals || num_vars >= 64 || (num_vars && (!point || !d_quot))) return ARK_HIP_ERR_ARG;
  if (num_vars > 58) return ARK_HIP_ERR_ARG;
  const size_t n = (size_t)1 << num_vars;
  if (num_vars && ranges_overlap(d_evals, n * 32, d_quot, (n - 1) * 32)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (num_vars == 0) {   // a constant: no quotient, the value is its one table entry
    if (!out_value) return 0;
    ARK_HIP_TRY(hipMemcpyAsync(out_value, d_evals, 32, hipMemcpyDeviceToHost, c->stream));
    ARK_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  }
  int widths[MLE_MAX_PASSES];
  const int passes = mle_fold_passes((int)num_vars, widths);
  // [result slot | the table after launch 0 | after launch 1 | ...], as mle_fold_run
  size_t scratch = 1;
  for (int p = 0, m = (int)num_vars; p + 1 < passes; p++) scratch += (size_t)1 << (m -= widths[p]);
  if (int rc = poly_scratch(c, scratch)) return rc;
  char* w = (char*)c->poly_work.p + 32;
  const void* cur = d_evals;
  int m = (int)num_vars;
  for (int p = 0; p < passes; p++) {
    MlePoint pt = {};
    mle_point_fill(pt, point, widths[p]);
    point += 4 * widths[p];
    void* dst = p + 1 < passes ? (void*)w : c->poly_work.p;
    // the segment of variable i = num_vars - m starts at element 2^num_vars - 2^m
    char* quot = (char*)d_quot + (n - ((size_t)1 << m)) * 32;
    if (int rc = ops->mle_quot(cur, m, widths[p], pt, quot, dst, c->stream)) return rc;
    m -= widths[p];
    w += ((size_t)1 << m) * 32;
    cur = dst;
  }
  if (out_value) return result_to_host(c, out_value);
  return mark_producer(c);
}

int ark_hip_mle_relabel_device(int field, const void* d_evals, unsigned num_vars, unsigned a, unsigned b, unsigned k, void* d_out) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_evals || !d_out || num_vars >= 64) return ARK_HIP_ERR_ARG;
  if (num_vars > 58) return ARK_HIP_ERR_ARG;
  if (a > b) { const unsigned t = a; a = b; b = t; }
  const bool identity = a == b || k == 0;   // the reference returns before its assertions (dense.rs:81-83)
  if (!identity && ((uint64_t)b + k > num_vars || (uint64_t)a + k > b)) return ARK_HIP_ERR_ARG;
  const size_t n = (size_t)1 << num_vars;
  if (d_out != d_evals && ranges_overlap(d_evals, n * 32, d_out, n * 32)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (identity) {
    if (d_out != d_evals) ARK_HIP_TRY(hipMemcpyAsync(d_out, d_evals, n * 32, hipMemcpyDeviceToDevice, c->stream));
    return mark_producer(c);
  }
  if (int rc = ops->mle_relabel(d_evals, n, (int)a, (int)b, (int)k, d_out, c->stream)) return rc;
  return mark_producer(c);
}

int ark_hip_fr_axpy_device(int field, const void* d_a, const uint64_t* k, const void* d_x, void* d_r, size_t n) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !k || (n && (!d_a || !d_x || !d_r))) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (int rc = ops->fr_axpy(d_a, k, d_x, d_r, n, c->stream)) return rc;
  return mark_producer(c);
}

int ark_hip_mle_product_tree_plan(unsigned num_vars, int* passes, int* widths, int* group_log) {
  if (!passes || !widths || !group_log || num_vars >= 64) return ARK_HIP_ERR_ARG;
  for (int p = 0; p < MLE_MAX_PASSES; p++) widths[p] = group_log[p] = 0;
  *passes = prod_tree_plan((int)num_vars, widths);   // one chunk of 64 outputs per wave in every launch: group_log stays 0
  return 0;
}

int ark_hip_mle_product_tree_device(int field, const void* d_evals, unsigned num_vars, void* d_tree, uint64_t* out_product) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_evals || num_vars >= 64 || (num_vars && !d_tree)) return ARK_HIP_ERR_ARG;
  if (num_vars > 58) return ARK_HIP_ERR_ARG;   // the table's bytes must fit a size_t
  const size_t n = (size_t)1 << num_vars;
  if (num_vars && ranges_overlap(d_evals, n * 32, d_tree, (n - 1) * 32)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  const void* product = d_evals;   // a constant: no tree, the product is its one table entry
  if (num_vars) {
    int widths[PROD_TREE_MAX_LAUNCHES];
    const int launches = prod_tree_launches((int)num_vars, widths);
    const void* cur = d_evals;
    int m = (int)num_vars;
    for (int p = 0; p < launches; p++) {
      // L_k starts at element 2^num_vars - 2^(k+1): the launch reads L_m and writes from L_(m-1) on
      char* dst = (char*)d_tree + (n - ((size_t)1 << m)) * 32;
      if (int rc = ops->prod_tree(cur, m, widths[p], dst, c->stream)) return rc;
      m -= widths[p];
      cur = (char*)d_tree + (n - ((size_t)2 << m)) * 32;
    }
    product = cur;
  }
  if (!out_product) return num_vars ? mark_producer(c) : 0;
  ARK_HIP_TRY(hipMemcpyAsync(out_product, product, 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int ark_hip_fr_lincomb_device(int field, const void* const* d_tables, unsigned ntables, const uint64_t* coeffs, const uint64_t* c0,
                              void* d_out, size_t n) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_tables || !coeffs || !d_out || ntables == 0 || ntables > (unsigned)LINCOMB_MAX_TABLES) return ARK_HIP_ERR_ARG;
  if (n > ((size_t)-1) / 32) return ARK_HIP_ERR_ARG;   // the table's bytes must fit a size_t
  FrLincomb lc = {};
  lc.ntables = ntables;
  lc.has_c0 = c0 ? 1 : 0;
  for (unsigned k = 0; k < ntables; k++) {
    if (!d_tables[k]) return ARK_HIP_ERR_ARG;
    if (d_tables[k] != d_out && ranges_overlap(d_tables[k], n * 32, d_out, n * 32)) return ARK_HIP_ERR_ARG;
    lc.tab[k] = (const char*)d_tables[k];
    for (int q = 0; q < 4; q++) { lc.coeff[k].l[2 * q] = (u32)coeffs[4 * k + q]; lc.coeff[k].l[2 * q + 1] = (u32)(coeffs[4 * k + q] >> 32); }
  }
  if (c0)
    for (int q = 0; q < 4; q++) { lc.c0.l[2 * q] = (u32)c0[q]; lc.c0.l[2 * q + 1] = (u32)(c0[q] >> 32); }
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (int rc = ops->fr_lincomb(lc, d_out, n, c->stream)) return rc;
  return mark_producer(c);
}

int ark_hip_mle_fraction_tree_plan(unsigned num_vars, int has_num, int* passes, int* widths, int* group_log) {
  if (!passes || !widths || !group_log || num_vars >= 64) return ARK_HIP_ERR_ARG;
  (void)has_num;   // ones for numerators change the first launch's kernel variant, not the launches
  for (int p = 0; p < MLE_MAX_PASSES; p++) widths[p] = group_log[p] = 0;
  *passes = frac_tree_plan((int)num_vars, widths);   // one chunk of 64 outputs per wave in every launch: group_log stays 0
  return 0;
}

int ark_hip_mle_fraction_tree_device(int field, const void* d_num, const void* d_den, unsigned num_vars, void* d_num_tree,
                                     void* d_den_tree, uint64_t* out_root) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_den || num_vars >= 64 || (num_vars && (!d_num_tree || !d_den_tree))) return ARK_HIP_ERR_ARG;
  if (num_vars > 58) return ARK_HIP_ERR_ARG;   // a table's bytes must fit a size_t
  const size_t n = (size_t)1 << num_vars;
  if (num_vars) {
    const size_t tb = (n - 1) * 32;
    if (ranges_overlap(d_num_tree, tb, d_den_tree, tb) || ranges_overlap(d_den, n * 32, d_num_tree, tb) ||
        ranges_overlap(d_den, n * 32, d_den_tree, tb))
      return ARK_HIP_ERR_ARG;
    if (d_num && (ranges_overlap(d_num, n * 32, d_num_tree, tb) || ranges_overlap(d_num, n * 32, d_den_tree, tb))) return ARK_HIP_ERR_ARG;
  }
  ARK_SCOPE(sc);
  Context* c = sc.c;
  const void *ncur = d_num, *dcur = d_den;   // a constant: no trees, the root is the one fraction
  if (num_vars) {
    int widths[FRAC_TREE_MAX_LAUNCHES];
    const int launches = frac_tree_launches((int)num_vars, widths);
    int m = (int)num_vars;
    for (int p = 0; p < launches; p++) {
      // level k starts at element 2^num_vars - 2^(k+1) of its tree: the launch reads level m and writes from level m - 1 on
      const size_t dst = (n - ((size_t)1 << m)) * 32;
      if (int rc = ops->frac_tree(ncur, dcur, m, widths[p], (char*)d_num_tree + dst, (char*)d_den_tree + dst, c->stream)) return rc;
      m -= widths[p];
      ncur = (char*)d_num_tree + (n - ((size_t)2 << m)) * 32;
      dcur = (char*)d_den_tree + (n - ((size_t)2 << m)) * 32;
    }
  }
  if (!out_root) return num_vars ? mark_producer(c) : 0;
  if (ncur) ARK_HIP_TRY(hipMemcpyAsync(out_root, ncur, 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipMemcpyAsync(out_root + 4, dcur, 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  if (!ncur) return fr_one_any(field, out_root);   // no variables and ones for numerators
  return 0;
}

int ark_hip_fr_count_indices_device(int field, const uint32_t* d_indices, size_t n, void* d_out, size_t table_len) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_out || (n && !d_indices) || table_len == 0) return ARK_HIP_ERR_ARG;
  if ((uint64_t)n >> 32 || table_len > ((size_t)1 << 58)) return ARK_HIP_ERR_ARG;   // a count fits a cell's first word
  if (n && ranges_overlap(d_indices, n * 4, d_out, table_len * 32)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (int rc = ops->fr_count(d_indices, n, d_out, table_len, c->stream)) return rc;
  return mark_producer(c);
}

// ---- lookup by value ----
static_assert(LOOKUP_EMPTY == ARK_HIP_LOOKUP_MISSING, "the header publishes the index of a cell that is not in the table");
int ark_hip_fr_lookup_plan(size_t table_len, unsigned* capacity_log, size_t* scratch_bytes) {
  if (!capacity_log || !scratch_bytes || table_len == 0 || table_len > ((size_t)1 << LOOKUP_MAX_TABLE_LOG)) return ARK_HIP_ERR_ARG;
  *capacity_log = lookup_capacity_log(table_len);
  *scratch_bytes = lookup_scratch_bytes(*capacity_log);
  return 0;
}

int ark_hip_fr_lookup_device(int field, const void* d_table, size_t table_len, const void* d_values, size_t n, uint32_t* d_indices,
                             void* d_mult, uint64_t* out_missing) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_table || (n && !d_values) || table_len == 0 || table_len > ((size_t)1 << LOOKUP_MAX_TABLE_LOG)) return ARK_HIP_ERR_ARG;
  if ((uint64_t)n >> 32 || (!d_indices && !d_mult && !out_missing)) return ARK_HIP_ERR_ARG;
  const size_t tb = table_len * 32;
  if (d_mult && (ranges_overlap(d_mult, tb, d_table, tb) || (n && ranges_overlap(d_mult, tb, d_values, n * 32)))) return ARK_HIP_ERR_ARG;
  if (d_indices && n &&
      (ranges_overlap(d_indices, n * 4, d_table, tb) || ranges_overlap(d_indices, n * 4, d_values, n * 32) ||
       (d_mult && ranges_overlap(d_indices, n * 4, d_mult, tb))))
    return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  FrLookup lk = {};
  lk.capacity_log = lookup_capacity_log(table_len);
  // [result slot | miss counter | slots]
  if (int rc = poly_scratch(c, lookup_scratch_bytes(lk.capacity_log) / 32)) return rc;
  lk.table = d_table;
  lk.table_len = table_len;
  lk.values = d_values;
  lk.n = n;
  lk.indices = d_indices;
  lk.mult = d_mult;
  lk.missing = (unsigned long long*)((char*)c->poly_work.p + 32);
  lk.slots = (u32*)((char*)c->poly_work.p + 64);
  if (int rc = ops->fr_lookup(lk, c->stream)) return rc;
  if (!out_missing) return mark_producer(c);
  ARK_HIP_TRY(hipMemcpyAsync(out_missing, lk.missing, 8, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int ark_hip_sumcheck_plan(unsigned num_vars, unsigned ntables, unsigned degree, int fused, int* blocks, int* pairs_per_lane,
                          int* stages) {
  if (!blocks || !pairs_per_lane || !stages || num_vars == 0 || num_vars >= 64) return ARK_HIP_ERR_ARG;
  if (ntables == 0 || ntables > (unsigned)SUMCHECK_MAX_TABLES || degree == 0 || degree > (unsigned)SUMCHECK_MAX_DEGREE) return ARK_HIP_ERR_ARG;
  unsigned b;
  size_t ppl;
  sumcheck_geometry((int)num_vars - (fused ? 1 : 0), &b, &ppl);
  *blocks = (int)b;
  *pairs_per_lane = ppl > 0x7fffffffu ? 0x7fffffff : (int)ppl;
  *stages = b > 1 ? 2 : 1;
  return 0;
}

int ark_hip_sumcheck_round_device(int field, const void* const* d_tables, unsigned ntables, unsigned num_vars,
                                  const unsigned* term_len, const unsigned* term_tables, const uint64_t* coeffs, unsigned nterms,
                                  const uint64_t* r_prev, void* const* d_out_tables, uint64_t* out_evals) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_tables || !term_len || !term_tables || !coeffs || !out_evals || (r_prev && !d_out_tables)) return ARK_HIP_ERR_ARG;
  if (ntables == 0 || ntables > (unsigned)SUMCHECK_MAX_TABLES || nterms == 0 || nterms > (unsigned)SUMCHECK_MAX_TERMS) return ARK_HIP_ERR_ARG;
  if (num_vars == 0 || num_vars >= 64 || num_vars > 58) return ARK_HIP_ERR_ARG;   // the table's bytes must fit a size_t
  SumcheckRound rd = {};
  if (int rc = sumcheck_terms(field, ntables, term_len, term_tables, coeffs, nterms, &rd.tm)) return rc;
  const size_t n = (size_t)1 << num_vars;
  for (unsigned k = 0; k < ntables; k++) {
    if (!d_tables[k] || (r_prev && !d_out_tables[k])) return ARK_HIP_ERR_ARG;
    rd.tb.src[k] = (const char*)d_tables[k];
    if (!r_prev) continue;
    rd.tb.dst[k] = (char*)d_out_tables[k];
    for (unsigned i = 0; i < ntables; i++)
      if (ranges_overlap(d_tables[i], n * 32, d_out_tables[k], n * 16)) return ARK_HIP_ERR_ARG;
    for (unsigned i = 0; i < k; i++)
      if (ranges_overlap(d_out_tables[i], n * 16, d_out_tables[k], n * 16)) return ARK_HIP_ERR_ARG;
  }
  const unsigned degree = rd.tm.degree;
  rd.fused = r_prev ? 1 : 0;
  rd.last = r_prev && num_vars == 1;
  if (r_prev)
    for (int q = 0; q < 4; q++) { rd.tm.r.l[2 * q] = (u32)r_prev[q]; rd.tm.r.l[2 * q + 1] = (u32)(r_prev[q] >> 32); }
  const int m = (int)num_vars - rd.fused;
  rd.npairs = m >= 1 ? (size_t)1 << (m - 1) : 1;
  size_t ppl;
  sumcheck_geometry(m, &rd.blocks, &ppl);
  ARK_SCOPE(sc);
  Context* c = sc.c;
  // [result area: one element per t | one partial per workgroup and t]
  if (int rc = poly_scratch(c, (size_t)SUMCHECK_EVALS * (1 + (rd.blocks > 1 ? rd.blocks : 0)))) return rc;
  rd.out = c->poly_work.p;
  rd.partials = (char*)c->poly_work.p + SUMCHECK_EVALS * 32;
  if (int rc = ops->sumcheck_round(rd, c->stream)) return rc;
  ARK_HIP_TRY(hipMemcpyAsync(out_evals, c->poly_work.p, (size_t)(degree + 1) * 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- the transcript and the whole proof in one wait ----
int ark_hip_transcript_challenge(int field, uint8_t* state, const uint64_t* elements, unsigned count, uint64_t* out_challenge) {
  if (!field_ops(field) || !state || !out_challenge || (count && !elements)) return ARK_HIP_ERR_ARG;
  if (count > (1u << 24)) return ARK_HIP_ERR_ARG;
  std::vector<u32> msg(transcript_words(count));
  memcpy(msg.data(), state, 32);
  const int rc = transcript_host_any(field, msg.data(), elements, count, out_challenge);
  if (rc == 0) memcpy(state, msg.data(), 32);
  return rc;
}

int ark_hip_sumcheck_prove_plan(unsigned num_vars, unsigned ntables, int tail_vars, size_t* work_elems, int* launches, int* tail_from) {
  if (!work_elems || !launches || !tail_from || num_vars == 0 || num_vars > 58) return ARK_HIP_ERR_ARG;
  if (ntables == 0 || ntables > (unsigned)SUMCHECK_MAX_TABLES || tail_vars < -1 || tail_vars > SUMCHECK_TAIL_MAX_VARS) return ARK_HIP_ERR_ARG;
  const int tf = prove_tail_from(num_vars, tail_vars);
  *work_elems = prove_work_elems(num_vars, ntables);
  *launches = sumcheck_prove_launches(num_vars, tf);
  *tail_from = tf;
  return 0;
}

int ark_hip_sumcheck_prove_device(int field, const void* const* d_tables, unsigned ntables, unsigned num_vars, const unsigned* term_len,
                                  const unsigned* term_tables, const uint64_t* coeffs, unsigned nterms, uint8_t* state, int tail_vars,
                                  void* d_work, uint64_t* out_rounds, uint64_t* out_point, uint64_t* out_finals, uint64_t* out_value) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_tables || !term_len || !term_tables || !coeffs || !state) return ARK_HIP_ERR_ARG;
  if (!out_rounds || !out_point || !out_finals || !out_value) return ARK_HIP_ERR_ARG;
  if (ntables == 0 || ntables > (unsigned)SUMCHECK_MAX_TABLES || nterms == 0 || nterms > (unsigned)SUMCHECK_MAX_TERMS) return ARK_HIP_ERR_ARG;
  if (num_vars == 0 || num_vars > 58) return ARK_HIP_ERR_ARG;   // the table's bytes must fit a size_t
  if (tail_vars < -1 || tail_vars > SUMCHECK_TAIL_MAX_VARS) return ARK_HIP_ERR_ARG;
  SumcheckProve pv = {};
  if (int rc = sumcheck_terms(field, ntables, term_len, term_tables, coeffs, nterms, &pv.tm)) return rc;
  const size_t n = (size_t)1 << num_vars, work = prove_work_elems(num_vars, ntables);
  if (!d_work) return ARK_HIP_ERR_ARG;   // work is never zero: the one-element tables lie there
  for (unsigned k = 0; k < ntables; k++) {
    if (!d_tables[k] || ranges_overlap(d_tables[k], n * 32, d_work, work * 32)) return ARK_HIP_ERR_ARG;
    pv.src[k] = (const char*)d_tables[k];
  }
  const size_t half = (size_t)1 << (num_vars - 1), quarter = (size_t)1 << (num_vars >= 2 ? num_vars - 2 : 0);
  for (unsigned k = 0; k < ntables; k++) {
    pv.set[0][k] = (char*)d_work + k * half * 32;
    pv.set[1][k] = (char*)d_work + (ntables * half + k * quarter) * 32;
  }
  pv.num_vars = num_vars;
  pv.tail_from = prove_tail_from(num_vars, tail_vars);
  memcpy(pv.state0.w, state, 32);
  const unsigned degree = pv.tm.degree;
  unsigned blocks;
  size_t ppl;
  sumcheck_geometry((int)num_vars, &blocks, &ppl);   // the first round has the most workgroups
  ARK_SCOPE(sc);
  Context* c = sc.c;
  // [sums | one partial per workgroup and t | cell | state | point | rounds | finals | value]
  const size_t o_cell = (size_t)SUMCHECK_EVALS * (1 + (blocks > 1 ? blocks : 0)), o_point = o_cell + 2, o_rounds = o_point + num_vars,
               o_finals = o_rounds + (size_t)num_vars * (degree + 1), o_value = o_finals + ntables;
  if (int rc = poly_scratch(c, o_value + 1)) return rc;
  char* w = (char*)c->poly_work.p;
  pv.sums = w;
  pv.partials = w + SUMCHECK_EVALS * 32;
  pv.cell = w + o_cell * 32;
  pv.state = w + (o_cell + 1) * 32;
  pv.point = w + o_point * 32;
  pv.rounds = w + o_rounds * 32;
  pv.finals = w + o_finals * 32;
  pv.value = w + o_value * 32;
  if (int rc = ops->sumcheck_prove(pv, c->stream)) return rc;
  ARK_HIP_TRY(hipMemcpyAsync(out_rounds, pv.rounds, (size_t)num_vars * (degree + 1) * 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipMemcpyAsync(out_point, pv.point, (size_t)num_vars * 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipMemcpyAsync(out_finals, pv.finals, (size_t)ntables * 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipMemcpyAsync(out_value, pv.value, 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipMemcpyAsync(state, pv.state, 32, hipMemcpyDeviceToHost, c->stream));
  ARK_HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- gate expressions: sums of products of columns read at rotations ----
int ark_hip_fr_sum_of_products_plan(size_t n, int* blocks, int* rows_per_lane) {
  if (!blocks || !rows_per_lane) return ARK_HIP_ERR_ARG;
  unsigned b;
  size_t rpl;
  gate_geometry(n, &b, &rpl);
  *blocks = (int)b;
  *rows_per_lane = rpl > 0x7fffffffu ? 0x7fffffff : (int)rpl;
  return 0;
}

int ark_hip_fr_sum_of_products_device(int field, const void* const* d_columns, unsigned ncolumns, size_t n, const unsigned* term_len,
                                      const unsigned* term_columns, const int64_t* term_rotations, const uint64_t* coeffs,
                                      unsigned nterms, const uint64_t* c0, void* d_out) {
  const FieldOps* ops = field_ops(field);
  if (!ops || !d_columns || !term_len || !term_columns || !coeffs || !d_out) return ARK_HIP_ERR_ARG;
  if (ncolumns == 0 || ncolumns > (unsigned)GATE_MAX_COLUMNS || nterms == 0 || nterms > (unsigned)GATE_MAX_TERMS) return ARK_HIP_ERR_ARG;
  if (n > ((size_t)1 << 58)) return ARK_HIP_ERR_ARG;   // a column's bytes must fit a size_t, and i + rot a u64
  GateTerms tm = {};
  tm.nterms = nterms;
  tm.has_c0 = c0 ? 1 : 0;
  bool rotated[GATE_MAX_COLUMNS] = {};   // some factor reads the column at a rotation that is not 0 mod n
  for (unsigned j = 0, at = 0; j < nterms; j++) {
    const unsigned len = term_len[j];
    if (len == 0 || len > (unsigned)GATE_MAX_DEGREE) return ARK_HIP_ERR_ARG;
    tm.len[j] = len;
    for (unsigned q = 0; q < len; q++, at++) {
      const unsigned k = term_columns[at];
      if (k >= ncolumns) return ARK_HIP_ERR_ARG;
      tm.tab[j] |= k << (4 * q);
      if (n && term_rotations) {   // the mathematical mod: INT64_MIN % n is representable, n <= 2^58
        int64_t r = term_rotations[at] % (int64_t)n;
        if (r < 0) r += (int64_t)n;
        tm.rot[j][q] = (unsigned long long)r;
        if (r) rotated[k] = true;
      }
    }
    for (int q = 0; q < 4; q++) { tm.coeff[j].l[2 * q] = (u32)coeffs[4 * j + q]; tm.coeff[j].l[2 * q + 1] = (u32)(coeffs[4 * j + q] >> 32); }
    if (field_is_one(field, coeffs + 4 * j)) tm.unit |= 1u << j;
  }
  if (c0)
    for (int q = 0; q < 4; q++) { tm.c0.l[2 * q] = (u32)c0[q]; tm.c0.l[2 * q + 1] = (u32)(c0[q] >> 32); }
  for (unsigned k = 0; n && k < ncolumns; k++) {
    if (!d_columns[k]) return ARK_HIP_ERR_ARG;
    // in place only where a lane reads the row it writes: with a rotation one workgroup would write what another still reads
    if (d_columns[k] == d_out ? rotated[k] : ranges_overlap(d_columns[k], n * 32, d_out, n * 32)) return ARK_HIP_ERR_ARG;
    tm.col[k] = (const char*)d_columns[k];
  }
  ARK_SCOPE(sc);
  Context* c = sc.c;
  if (n == 0) return 0;
  if (int rc = ops->gate_sum_of_products(tm, d_out, n, c->stream)) return rc;
  return mark_producer(c);
}

}  // extern "C"
