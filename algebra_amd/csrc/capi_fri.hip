// C ABI of the extension fields over the one-word fields (ark_hip_xfp_*) and of FRI over them (ark_hip_fri_*): single elements,
// the fold of one row, the folded domain and the commit-phase plan as pure host code; the pointwise vectors, the combination of
// columns and the fold through SmallFieldOps (sfp_internal.hpp); the commit phase as a chain of the library's own entries.
// DESIGN.md section 30.
#include "capi_sfp.hpp"
#include "sfp_fri.cuh"

using namespace arkhip;
using namespace arkhip::capi;

namespace {

template <class Cfg>
int xinfo_of(uint64_t out[8]) {
  using X = SFpX<Cfg>;
  out[0] = X::D;
  out[1] = SfpXCfg<Cfg>::W;
  out[2] = X::W_MONT;
  // component k is the coefficient of X^out[3 + k] in Fp[X] / (X^D - W)
  const uint64_t order2[4] = {0, 1, 0, 0}, order4[4] = {0, 2, 1, 3};
  for (int k = 0; k < 4; k++) out[3 + k] = X::D == 2 ? order2[k] : order4[k];
  out[7] = 0;
  return 0;
}
int degree_of(int sfield) { return sfield == ARK_HIP_SFP_GOLDILOCKS ? 2 : 4; }

// an element that crosses the interface: D components < p, the words behind them zero
bool elem_ok(const SfpHost& h, int d, const uint64_t* e) {
  if (!e) return false;
  for (int k = 0; k < 4; k++)
    if (k < d ? e[k] >= h.p : e[k] != 0) return false;
  return true;
}
template <class Cfg>
void elem_out(const typename SFpX<Cfg>::E& e, uint64_t out[4]) {
  for (int k = 0; k < 4; k++) out[k] = k < SFpX<Cfg>::D ? (uint64_t)e.c[k] : 0;
}
template <class Cfg>
int xmul_of(const uint64_t* a, const uint64_t* b, uint64_t* out) {
  elem_out<Cfg>(SFpX<Cfg>::mul(sfpx_elem<Cfg>(a), sfpx_elem<Cfg>(b)), out);
  return 0;
}
template <class Cfg>
int xinv_of(const uint64_t* a, uint64_t* out) {
  elem_out<Cfg>(SFpX<Cfg>::inv(sfpx_elem<Cfg>(a)), out);
  return 0;
}
template <class Cfg>
int xpow_of(const uint64_t* a, uint64_t e, uint64_t* out) {
  elem_out<Cfg>(SFpX<Cfg>::pow(sfpx_elem<Cfg>(a), e), out);
  return 0;
}
int xmul_any(int sfield, const uint64_t* a, const uint64_t* b, uint64_t* out) {
#define CALL(NAME) xmul_of<NAME>(a, b, out)
  ARK_SFP_SWITCH(sfield, CALL);
#undef CALL
}
int xpow_any(int sfield, const uint64_t* a, uint64_t e, uint64_t* out) {
#define CALL(NAME) xpow_of<NAME>(a, e, out)
  ARK_SFP_SWITCH(sfield, CALL);
#undef CALL
}

// the fold of one row through the template the kernel instantiates; row[k * 2^a + j] = component k of f[i + j n / 2^a]
template <class Cfg, int A>
int fold_row_a(const uint64_t* row, uint64_t t, const SfpFoldRoots& roots, const uint64_t* beta, uint64_t* out) {
  using X = SFpX<Cfg>;
  typename X::E v[1 << A];
  for (int j = 0; j < (1 << A); j++)
    for (int k = 0; k < X::D; k++) v[j].c[k] = (typename Cfg::T)row[(k << A) + j];
  elem_out<Cfg>(sfpx_fold_row<Cfg, A>(v, (typename Cfg::T)t, roots, sfpx_elem<Cfg>(beta)), out);
  return 0;
}
template <class Cfg>
int fold_row_of(int a, const uint64_t* row, uint64_t t, const SfpFoldRoots& roots, const uint64_t* beta, uint64_t* out) {
  switch (a) {
    case 1: return fold_row_a<Cfg, 1>(row, t, roots, beta, out);
    case 2: return fold_row_a<Cfg, 2>(row, t, roots, beta, out);
    case 3: return fold_row_a<Cfg, 3>(row, t, roots, beta, out);
  }
  return ARK_HIP_ERR_ARG;
}

// (2 h)^-1, and zeta^-e for e < 4 with zeta = w^(n / 2^a)
uint64_t fold_scale(const SfpHost& h, const ark_hip_sfp_radix2_domain* dom) {
  const uint64_t two = h.from_canonical(2);
  return h.mul(h.pow(two, h.p - 2), dom->offset_inv);
}
SfpFoldRoots fold_roots(const SfpHost& h, const ark_hip_sfp_radix2_domain* dom, int a) {
  SfpFoldRoots r;
  const uint64_t zi = h.pow(dom->group_gen_inv, dom->size >> a);
  r.zinv[0] = h.one;
  for (int e = 1; e < 4; e++) r.zinv[e] = h.mul(r.zinv[e - 1], zi);
  return r;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}
// bytes from the first word of an extension vector to the end of its last component; false beyond size_t
bool xvec_extent(const SfpHost& h, int d, size_t stride, size_t n, size_t* bytes) {
  const size_t lim = ~(size_t)0 / (size_t)h.bytes;
  if (n > lim || (size_t)(d - 1) > (lim - n) / (stride ? stride : 1)) return false;
  *bytes = ((size_t)(d - 1) * stride + n) * h.bytes;
  return true;
}

struct FriLayout {
  int layers;                  // num_folds + 1
  int log[34], arity[34], lo_bits[34];
  uint64_t layer_at[34], tree_at[34];   // elements into d_layers (layer 0: the caller's own), bytes into d_trees
  uint64_t copy_at, layer_words, tree_bytes;
};
// ARK_HIP_ERR_ARG unless every fold has at least one level to take
int fri_layout(int d, unsigned log_n, unsigned a, unsigned num_folds, FriLayout* L) {
  if (a < 1 || a > 3 || log_n > 32 || num_folds > log_n) return ARK_HIP_ERR_ARG;
  if (num_folds && (uint64_t)(num_folds - 1) * a >= log_n) return ARK_HIP_ERR_ARG;
  L->layers = (int)num_folds + 1;
  int k = (int)log_n;
  uint64_t words = 0, tbytes = 0;
  for (int l = 0; l <= (int)num_folds; l++) {
    const int al = l < (int)num_folds ? ((int)a < k ? (int)a : k) : 0;
    L->log[l] = k;
    L->arity[l] = al;
    L->lo_bits[l] = al ? (k + 1) / 2 : 0;
    L->layer_at[l] = l ? words : 0;
    if (l) words += (uint64_t)d << k;
    L->tree_at[l] = tbytes;
    if (al) tbytes += ((((uint64_t)1 << (k - al)) << 1) - 1) * ARK_HIP_MERKLE_DIGEST_BYTES;
    k -= al;
  }
  L->copy_at = words;                       // the interpolated copy of the last layer
  words += (uint64_t)d << L->log[num_folds];
  L->layer_words = words;
  L->tree_bytes = tbytes;
  return 0;
}

int xvec_entry(int sfield, int op, const void* d_a, size_t sa, const void* d_b, size_t sb, const uint64_t* k, void* d_r, size_t sr,
               size_t n) {
  SfpHost h;
  if (sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  const SmallFieldOps* ops = sfp_ops(sfield);
  if (!ops) return ARK_HIP_ERR_ARG;
  const int d = degree_of(sfield);
  const bool has_b = op == SFPX_OP_MUL || op == SFPX_OP_MUL_BASE;
  if (n > 0 && (!d_a || !d_r || (has_b && !d_b))) return ARK_HIP_ERR_ARG;
  if (sa < n || sr < n || (op == SFPX_OP_MUL && sb < n)) return ARK_HIP_ERR_ARG;
  if (((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_r) % (uintptr_t)h.bytes) return ARK_HIP_ERR_ARG;   // whole words
  SfpxConst kc{};
  if (op == SFPX_OP_MUL_CONST) {
    if (!elem_ok(h, d, k)) return ARK_HIP_ERR_ARG;
    for (int i = 0; i < 4; i++) kc.c[i] = k[i];
  }
  size_t ea, er, eb = 0;
  if (!xvec_extent(h, d, sa, n, &ea) || !xvec_extent(h, d, sr, n, &er) || (op == SFPX_OP_MUL && !xvec_extent(h, d, sb, n, &eb)))
    return ARK_HIP_ERR_SIZE;
  ARK_SCOPE(sc);
  if (n == 0) return 0;
  if (int rc = ops->xvec_op(op, d_a, sa, d_b, sb, kc, d_r, sr, n, sc.c->stream)) return rc;
  return mark_producer(sc.c);
}

}  // namespace

extern "C" {

int ark_hip_xfp_info(int sfield, uint64_t out[8]) {
  if (!out) return ARK_HIP_ERR_ARG;
#define CALL(NAME) xinfo_of<NAME>(out)
  ARK_SFP_SWITCH(sfield, CALL);
#undef CALL
}

int ark_hip_xfp_mul(int sfield, const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {
  SfpHost h;
  if (sfp_host(sfield, &h) || !out) return ARK_HIP_ERR_ARG;
  const int d = degree_of(sfield);
  if (!elem_ok(h, d, a) || !elem_ok(h, d, b)) return ARK_HIP_ERR_ARG;
  return xmul_any(sfield, a, b, out);
}

int ark_hip_xfp_inverse(int sfield, const uint64_t a[4], uint64_t out[4]) {
  SfpHost h;
  if (sfp_host(sfield, &h) || !out || !elem_ok(h, degree_of(sfield), a)) return ARK_HIP_ERR_ARG;
#define CALL(NAME) xinv_of<NAME>(a, out)
  ARK_SFP_SWITCH(sfield, CALL);
#undef CALL
}

int ark_hip_xfp_pow(int sfield, const uint64_t a[4], uint64_t exp, uint64_t out[4]) {
  SfpHost h;
  if (sfp_host(sfield, &h) || !out || !elem_ok(h, degree_of(sfield), a)) return ARK_HIP_ERR_ARG;
  return xpow_any(sfield, a, exp, out);
}

int ark_hip_xfp_vec_mul(int sfield, const void* d_a, size_t stride_a, const void* d_b, size_t stride_b, void* d_r, size_t stride_r,
                        size_t n) {
  return xvec_entry(sfield, SFPX_OP_MUL, d_a, stride_a, d_b, stride_b, nullptr, d_r, stride_r, n);
}
int ark_hip_xfp_vec_inverse(int sfield, const void* d_a, size_t stride_a, void* d_r, size_t stride_r, size_t n) {
  return xvec_entry(sfield, SFPX_OP_INVERSE, d_a, stride_a, nullptr, 0, nullptr, d_r, stride_r, n);
}
int ark_hip_xfp_vec_mul_const(int sfield, const void* d_a, size_t stride_a, const uint64_t k[4], void* d_r, size_t stride_r, size_t n) {
  return xvec_entry(sfield, SFPX_OP_MUL_CONST, d_a, stride_a, nullptr, 0, k, d_r, stride_r, n);
}
int ark_hip_xfp_vec_mul_base(int sfield, const void* d_a, size_t stride_a, const void* d_b, void* d_r, size_t stride_r, size_t n) {
  return xvec_entry(sfield, SFPX_OP_MUL_BASE, d_a, stride_a, d_b, 0, nullptr, d_r, stride_r, n);
}

int ark_hip_xfp_combine_columns(int sfield, const void* d_cols, size_t count, size_t stride, size_t rows, const uint64_t alpha[4],
                                uint64_t first_power, void* d_out, size_t stride_out, int accumulate) {
  SfpHost h;
  if (sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  const SmallFieldOps* ops = sfp_ops(sfield);
  if (!ops) return ARK_HIP_ERR_ARG;
  const int d = degree_of(sfield);
  if (!d_cols || !d_out || count < 1 || stride < rows || stride_out < rows || !elem_ok(h, d, alpha)) return ARK_HIP_ERR_ARG;
  if (((uintptr_t)d_cols | (uintptr_t)d_out) % (uintptr_t)h.bytes) return ARK_HIP_ERR_ARG;   // whole words
  const size_t lim = ~(size_t)0 / (size_t)h.bytes;
  size_t eout;
  if (rows > lim || count - 1 > (lim - rows) / (stride ? stride : 1) || !xvec_extent(h, d, stride_out, rows, &eout)) return ARK_HIP_ERR_SIZE;
  if (rows && overlaps(d_cols, ((count - 1) * stride + rows) * h.bytes, d_out, eout)) return ARK_HIP_ERR_ARG;
  SfpCombineArgs ar{};
  uint64_t one[4] = {h.one, 0, 0, 0};
  for (int k = 0; k < 4; k++) ar.pw[0][k] = one[k];
  for (int j = 1; j <= SFPX_COMBINE_BLOCK; j++) xmul_any(sfield, ar.pw[j - 1], alpha, ar.pw[j]);
  xpow_any(sfield, alpha, first_power, ar.first);
  ARK_SCOPE(sc);
  if (rows == 0) return 0;
  if (int rc = ops->xcombine(d_cols, count, stride, rows, ar, d_out, stride_out, accumulate ? 1 : 0, sc.c->stream)) return rc;
  return mark_producer(sc.c);
}

int ark_hip_fri_folded_domain(int sfield, const ark_hip_sfp_radix2_domain* dom, unsigned log_arity, ark_hip_sfp_radix2_domain* out) {
  SfpHost h;
  if (!out || sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  if (int rc = domain_check(h, dom)) return rc;
  if (log_arity < 1 || log_arity > 3 || log_arity > dom->log_size_of_group || dom->offset == 0) return ARK_HIP_ERR_ARG;
  ark_hip_sfp_radix2_domain plain;
  if (int rc = ark_hip_sfp_radix2_domain_new(sfield, (size_t)(dom->size >> log_arity), &plain)) return rc;
  return ark_hip_sfp_radix2_domain_get_coset(sfield, &plain, h.pow(dom->offset, (uint64_t)1 << log_arity), out);
}

int ark_hip_fri_fold_row(int sfield, const ark_hip_sfp_radix2_domain* dom, unsigned log_arity, uint64_t index, const uint64_t* row,
                         const uint64_t beta[4], uint64_t out[4]) {
  SfpHost h;
  if (!row || !out || sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  if (int rc = domain_check(h, dom)) return rc;
  const int d = degree_of(sfield);
  if (log_arity < 1 || log_arity > 3 || log_arity > dom->log_size_of_group || index >= (dom->size >> log_arity) || !elem_ok(h, d, beta))
    return ARK_HIP_ERR_ARG;
  for (int i = 0; i < (d << log_arity); i++)
    if (row[i] >= h.p) return ARK_HIP_ERR_ARG;
  const uint64_t t = h.mul(fold_scale(h, dom), h.pow(dom->group_gen_inv, index));
  const SfpFoldRoots roots = fold_roots(h, dom, (int)log_arity);
#define CALL(NAME) fold_row_of<NAME>((int)log_arity, row, t, roots, beta, out)
  ARK_SFP_SWITCH(sfield, CALL);
#undef CALL
}

int ark_hip_fri_plan(int sfield, unsigned log_n, unsigned log_arity, unsigned num_folds, uint64_t* out) {
  SfpHost h;
  if (!out || sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  if (log_n > (unsigned)h.two_adicity) return ARK_HIP_ERR_SIZE;
  FriLayout L;
  const int d = degree_of(sfield);
  if (int rc = fri_layout(d, log_n, log_arity, num_folds, &L)) return rc;
  out[0] = (uint64_t)d;
  out[1] = (uint64_t)L.layers;
  out[2] = L.layer_words;
  out[3] = L.tree_bytes;
  out[4] = 1;   // launches of one fold (its power table is built once per (size, offset) by one more)
  out[5] = (uint64_t)1 << L.log[num_folds];
  out[6] = L.copy_at;
  out[7] = 0;
  for (int l = 0; l < L.layers; l++) {
    uint64_t* o = out + 8 + 5 * l;
    o[0] = (uint64_t)L.log[l];
    o[1] = (uint64_t)L.arity[l];
    o[2] = L.layer_at[l];
    o[3] = L.tree_at[l];
    o[4] = (uint64_t)L.lo_bits[l];
  }
  return 0;
}

int ark_hip_fri_fold(int sfield, const ark_hip_sfp_radix2_domain* dom, unsigned log_arity, const uint64_t beta[4], const void* d_in,
                     size_t stride_in, void* d_out, size_t stride_out) {
  SfpHost h;
  if (sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  const SmallFieldOps* ops = sfp_ops(sfield);
  if (!ops || !d_in || !d_out) return ARK_HIP_ERR_ARG;
  if (int rc = domain_check(h, dom)) return rc;
  const int d = degree_of(sfield);
  if (log_arity < 1 || log_arity > 3 || log_arity > dom->log_size_of_group || !elem_ok(h, d, beta)) return ARK_HIP_ERR_ARG;
  const size_t n = (size_t)dom->size, m = n >> log_arity;
  if (stride_in < n || stride_out < m) return ARK_HIP_ERR_ARG;
  if ((uintptr_t)d_in % h.bytes || (uintptr_t)d_out % h.bytes) return ARK_HIP_ERR_ARG;
  size_t ein, eout;
  if (!xvec_extent(h, d, stride_in, n, &ein) || !xvec_extent(h, d, stride_out, m, &eout)) return ARK_HIP_ERR_SIZE;
  if (overlaps(d_in, ein, d_out, eout)) return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);
  Context* c = sc.c;
  SfpFoldArgs f{};
  f.in = d_in;
  f.out = d_out;
  f.stride_in = stride_in;
  f.stride_out = stride_out;
  f.k = (int)dom->log_size_of_group;
  f.lo_bits = (f.k + 1) / 2;
  SfpScale tab;
  if (int rc = powers_for(c, sfield, h, ops, f.k, dom->group_gen_inv, fold_scale(h, dom), &tab)) return rc;
  f.hi = tab.hi;
  f.lo = tab.lo;
  f.roots = fold_roots(h, dom, (int)log_arity);
  for (int k = 0; k < 4; k++) f.beta.c[k] = beta[k];
  if (int rc = ops->xfold(f, (int)log_arity, c->stream)) return rc;
  return mark_producer(c);
}

int ark_hip_fri_commit_phase(int sfield, const ark_hip_sfp_radix2_domain* dom, unsigned log_arity, unsigned num_folds,
                             const void* d_layer0, void* d_layers, void* d_trees, ark_hip_fri_next_beta next_beta, void* user,
                             uint8_t* out_roots, void* out_final) {
  SfpHost h;
  if (sfp_host(sfield, &h)) return ARK_HIP_ERR_ARG;
  if (!sfp_ops(sfield) || !d_layer0 || !d_layers || !out_final) return ARK_HIP_ERR_ARG;
  if (num_folds && (!d_trees || !next_beta || !out_roots)) return ARK_HIP_ERR_ARG;
  if (int rc = domain_check(h, dom)) return rc;
  const int d = degree_of(sfield);
  FriLayout L;
  if (int rc = fri_layout(d, dom->log_size_of_group, log_arity, num_folds, &L)) return rc;
  if ((uintptr_t)d_layer0 % 16 || (uintptr_t)d_layers % 16 || (uintptr_t)d_trees % 16) return ARK_HIP_ERR_ARG;
  const size_t n = (size_t)dom->size, eb = (size_t)h.bytes;
  const size_t bytes0 = (size_t)d * n * eb, layer_bytes = (size_t)L.layer_words * eb, tree_bytes = (size_t)L.tree_bytes;
  if (overlaps(d_layer0, bytes0, d_layers, layer_bytes) || (tree_bytes && overlaps(d_layer0, bytes0, d_trees, tree_bytes)) ||
      (tree_bytes && overlaps(d_layers, layer_bytes, d_trees, tree_bytes)))
    return ARK_HIP_ERR_ARG;
  ARK_SCOPE(sc);   // held across the chain: the entries below take the same (recursive) lock
  Context* c = sc.c;
  auto fail = [&](int rc) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  };
  ark_hip_sfp_radix2_domain cur_dom = *dom;
  const char* cur = (const char*)d_layer0;
  for (unsigned l = 0; l < num_folds; l++) {
    const int a = L.arity[l];
    const size_t rows = (size_t)1 << (L.log[l] - a);
    uint8_t* root = out_roots + (size_t)l * ARK_HIP_MERKLE_DIGEST_BYTES;
    // the row view: d 2^a columns of `rows` elements, one whole row of the fold in a leaf; the root is this layer's one wait
    if (int rc = ark_hip_merkle_commit_sfp_device(sfield, cur, (size_t)d << a, rows, rows, (char*)d_trees + L.tree_at[l], root))
      return fail(rc);
    uint64_t beta[4] = {0, 0, 0, 0};
    if (int rc = next_beta(user, root, beta)) return fail(rc);
    char* next = (char*)d_layers + (size_t)L.layer_at[l + 1] * eb;
    if (int rc = ark_hip_fri_fold(sfield, &cur_dom, (unsigned)a, beta, cur, (size_t)1 << L.log[l], next, rows)) return fail(rc);
    ark_hip_sfp_radix2_domain nd;
    if (int rc = ark_hip_fri_folded_domain(sfield, &cur_dom, (unsigned)a, &nd)) return fail(rc);
    cur_dom = nd;
    cur = next;
  }
  // the last layer's coefficients: the inverse coset transform of a copy, so that the layer itself stays
  const size_t last = (size_t)1 << L.log[num_folds], last_bytes = (size_t)d * last * eb;
  char* copy = (char*)d_layers + (size_t)L.copy_at * eb;
  if (int rc = ark_hip_memcpy_d2d(copy, cur, last_bytes)) return fail(rc);
  if (int rc = ark_hip_sfp_fft_batch_device(sfield, &cur_dom, copy, (size_t)d, last, last, 1)) return fail(rc);
  return ark_hip_memcpy_d2h(out_final, copy, last_bytes);
}

}  // extern "C"
