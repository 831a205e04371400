// Point vectors: out[i] = [k_i] P_i (a different point per lane), out[i] = A_i +- B_i, out[i] = [a] Lo_i + [b] Hi_i.
//
// The reference has no batch form: `Projective *= ScalarField` (ec/src/models/short_weierstrass/group.rs:556-570) goes through
// mul_bigint to SWCurveConfig::mul_projective / mul_affine (short_weierstrass/mod.rs:101-109) and double_and_add(_affine)
// (ec/src/scalar_mul/mod.rs:29-60), and callers map it over a vector with rayon; `Projective += Projective` is group.rs:450-538.
// Results are group elements: the Projective representative differs from the reference's, into_affine() agrees.
//
// One lane per point.  pv_chain is ONE host/device function: the kernels below and the host twins behind
// ark_hip_test_host_sw_mul / _fold run the same code.
//
// Algorithm (the recoding of gfft.cuh): the canonical 256-bit integer k plus 0x88..8 has the nibbles n_w with
//   k = sum_w (n_w - 8) 16^w + carry 16^64,  digits in [-8, 7], carry in {0, 1},
// so EVERY 256-bit value is multiplied exactly (an unreduced scalar included).  A lane builds the table [1..8] P, then walks 65
// windows MSB first (window 64 is the carry): four doublings, then at most one addition of +-[|d|] P per table -- 256 effective
// doublings + ~60 additions per scalar.  With NT = 2 tables the two chains of a fold share the doublings (Straus): the fold
// costs 256 doublings + ~120 additions instead of 512 + ~120 + 1.
//
// Table: canonical XYZZ entries (Montgomery residues, the form a bucket has in memory) in device memory, laid out
// [table][entry][lane] over the `nlanes` lanes of one launch, so that a wave's load of one entry is contiguous per limb vector.
// Dynamic indexing into registers would go through scratch; a 192-byte load per window is nothing beside its ~70 products.
// Entry 1 is the point itself: the chain never keeps the input alive in registers.
//
// Two arithmetic forms behind one chain (the policy O):
//   PvSat   saturated 32-bit limbs, XYZZ<F> with xyzz_dbl / xyzz_add (ec.cuh): every curve; the only form over Fp2 (one whole
//           Fp2 element per lane), and the G1 form under ARK_HIP_MSM_LAZY=0.
//   PvLazy  carry-free limbs (fp28.cuh / ec28.cuh: 14 x 28 bits for the Fp384 curves, 9 x 29 bits for BN254), the default for
//           the three G1 curves.  The accumulator is an XYZZL; table entries enter as multiplication operands by repacking only.
// gfft_scalar_mul (gfft.cuh) is the same algorithm, but device-only and for Montgomery scalars only (a canonical scalar >= r cannot
// pass through it unchanged); the saturated chain here takes the canonical integer and compiles for the host as well.
//
// Value bounds of the carry-free chain, in units of p; "n" = normalised limbs.  First figure: 14 x 28 bits (R' / p >= 2520 in
// ec28.cuh's products with a 256 p operand, >= 2048 otherwise), in brackets 9 x 29 bits (R' / p >= 169, operands below 32 p):
//   table entry as operands (lazy_operands_of: canonical limbs repacked)    x, y, zz, zzz < 256 [32]  (n)
//   accumulator after from_stored (lazy_from_bucket)                        x, y, zz, zzz < 1.13 [1.21]
//   accumulator after an addition (xyzz_add_lazy, operand b as above)       x in (0.97, 5.01) [5.07], y < 1.02 [1.15], zz, zzz < 1.01
//   accumulator after a doubling (xyzz_dbl_lazy)                            x in (1.9, 5.01) [5.07], y < 1.02 [1.15], zz, zzz < 1.01
// xyzz_dbl_lazy asks x, y < 256 [32] and xyzz_add_lazy asks acc.x < 5.01 [5.07], acc.y < 1.13 [1.23], zz, zzz < 1.13 [1.21]: every
// output above is a legal input of both, so "four doublings, then one addition per table" is closed for any number of windows,
// and both limb geometries share it.  lazy_to_bucket asks x < 5.01 [5.07]: shr_mod output < x / 2^SH + 1 < 2.
// A doubling of a point of order two (y = 0) leaves ZZ = 0 mod p without a flag: ZZ < 2 after every doubling and addition, so
// is_zero_or_p() is exact there and sets the accumulator's infinity flag (PvLazy::settle).
#pragma once
#include "msm.cuh"

namespace arkhip {

enum { PV_FORM_AFFINE = 0, PV_FORM_PROJECTIVE = 1 };   // ARK_HIP_FORM_* of include/ark_hip.h

// lanes of one launch: a launch's tables are NT * 8 * lanes XYZZ points (ARK_HIP_POINTVEC_SLAB_LOG = 6..17 lowers the cap: the
// tests cross slab seams at small sizes with it)
static constexpr int PV_SLAB_LOG = 17;
static inline size_t pv_slab() {
  const char* e = getenv("ARK_HIP_POINTVEC_SLAB_LOG");
  const int l = e ? atoi(e) : PV_SLAB_LOG;
  return (size_t)1 << (l >= 6 && l <= PV_SLAB_LOG ? l : PV_SLAB_LOG);
}

// NT scalars handed over by value (a fold's a and b): canonical or Montgomery limbs, as the entry received them
template <int NT>
struct PvImm { u32 w[NT][8]; };
static inline PvImm<2> pv_imm2(const uint64_t* a4, const uint64_t* b4) {
  PvImm<2> r;
  for (int i = 0; i < 4; i++) {
    r.w[0][2 * i] = (u32)a4[i];
    r.w[0][2 * i + 1] = (u32)(a4[i] >> 32);
    r.w[1][2 * i] = (u32)b4[i];
    r.w[1][2 * i + 1] = (u32)(b4[i] >> 32);
  }
  return r;
}

template <class C>
struct PvSat {
  typedef typename C::F F;
  typedef XYZZ<F> Pt;
  typedef XYZZ<F> Acc;
  ARK_HD static Acc zero() { return Pt::zero(); }
  ARK_HD static Acc from_stored(const Pt& p) { return p; }
  ARK_HD static Pt to_stored(const Acc& a) { return a; }
  ARK_HD static void dbl(Acc& a) { a = xyzz_dbl<F>(a); }
  ARK_HD static void add(Acc& a, const Pt& q) { xyzz_add<F>(a, q); }
};

template <class C>
struct PvLazy {
  typedef typename C::F F;
  typedef typename F::P P;
  typedef FpL<P> FL;
  typedef XYZZ<F> Pt;
  typedef XYZZL<P> Acc;
  ARK_HD static Acc zero() {
    Acc a;
    a.inf = true;
    a.x = a.y = a.zz = a.zzz = FL::zero();
    return a;
  }
  ARK_HD static Acc from_stored(const Pt& p) { return lazy_from_bucket<P>(p); }   // < 1.13 [1.21]
  ARK_HD static Pt to_stored(const Acc& a) { return lazy_to_bucket<P>(a); }       // a.x < 5.01 [5.07]
  ARK_HD static void settle(Acc& a) {   // ZZ < 2: 0 mod p is 0 or p (a doubled point of order two)
    if (!a.inf && a.zz.is_zero_or_p()) a.inf = true;
  }
  ARK_HD static void dbl(Acc& a) {      // in: x < 5.01 [5.07], y < 1.13 [1.23]; out: x < 5.01 [5.07], y < 1.02 [1.15], zz, zzz < 1.01
    if (a.inf) return;
    xyzz_dbl_lazy<P>(a);
    settle(a);
  }
  ARK_HD static void add(Acc& a, const Pt& q) {   // q: canonical, repacked below 256 [32]; out as after dbl
    const XYZZOperands<P> o = lazy_operands_of<P>(q);
    xyzz_add_lazy<P>(a, o.x, o.y, o.zz, o.zzz, o.inf);   // equal points double in place, opposite points set a.inf
    settle(a);
  }
};

// sum_t [k_t] P_t for NT <= 2 points of one lane.  p[t]: canonical XYZZ; kc[t]: the canonical integer of k_t, 8 x 32 bits.
// tab: NT * 8 * nlanes entries, this lane's column.  Returns the canonical XYZZ sum.
template <class O, int NT>
ARK_HD typename O::Pt pv_chain(const typename O::Pt (&p)[NT], const u32 (&kc)[NT][8], char* tab, size_t lane, size_t nlanes) {
  typedef typename O::Pt Pt;
  typedef typename O::Acc Acc;
  auto slot = [&](int t, int e) { return tab + ((size_t)(t * 8 + e - 1) * nlanes + lane) * Pt::BYTES; };
  u32 kw[NT][8], top[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    p[t].store(slot(t, 1));
    u32 carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const u64 v = (u64)kc[t][i] + 0x88888888u + carry;
      kw[t][i] = (u32)v;
      carry = (u32)(v >> 32);
    }
    top[t] = carry;
  }
  // [2..8] P_t: 2P = dbl(P), 3P = 2P + P, 4P = dbl(2P), ... (one doubling site and one addition site for every table)
#pragma unroll 1
  for (int j = 0; j < NT * 7; j++) {
    const int t = j / 7, e = 2 + j % 7;
    Acc a;
    if (e & 1) {
      a = O::from_stored(Pt::load(slot(t, e - 1)));
      O::add(a, Pt::load(slot(t, 1)));
    } else {
      a = O::from_stored(Pt::load(slot(t, e >> 1)));
      O::dbl(a);
    }
    O::to_stored(a).store(slot(t, e));
  }
  Acc acc = O::zero();
#pragma unroll 1
  for (int w = 64; w >= 0; w--) {
#pragma unroll 1
    for (int j = 0; j < 4; j++) O::dbl(acc);
#pragma unroll 1
    for (int t = 0; t < NT; t++) {
      u32 word = 0;
#pragma unroll
      for (int tt = 0; tt < NT; tt++) {
#pragma unroll
        for (int i = 0; i < 8; i++) word = (t == tt && (w >> 3) == i) ? kw[tt][i] : word;   // (no dynamic indexing into registers)
      }
      int d = (int)((word >> ((w & 7) * 4)) & 15u) - 8;
      if (w == 64) {
        d = 0;
#pragma unroll
        for (int tt = 0; tt < NT; tt++) d = t == tt ? (int)top[tt] : d;
      }
      if (d != 0) {
        Pt q = Pt::load(slot(t, d < 0 ? -d : d));
        if (d < 0) q = Pt::neg(q);   // canonical negation of y; the identity (zz = 0) stays the identity
        O::add(acc, q);
      }
    }
  }
  return O::to_stored(acc);
}

// Affine (x | y, identity (0, 0)) or Projective (Jacobian x | y | z, identity z = 0) -> XYZZ (x, y, z^2, z^3)
template <class C>
ARK_HD XYZZ<typename C::F> pv_load_point(const char* p, int form) {
  typedef typename C::F F;
  if (form == PV_FORM_AFFINE) return XYZZ<F>::from_affine(Affine<F>::load(p));
  const F z = F::load(p + 2 * F::FULL_BYTES);
  if (z.is_zero()) return XYZZ<F>::zero();
  XYZZ<F> q;
  q.x = F::load(p);
  q.y = F::load(p + F::FULL_BYTES);
  q.zz = F::sqr(z);
  q.zzz = F::mul(q.zz, z);
  return q;
}
template <class C>
ARK_HD size_t pv_point_bytes(int form) {
  return form == PV_FORM_AFFINE ? (size_t)Affine<typename C::F>::BYTES : (size_t)Jac<typename C::F>::BYTES;
}

// one lane of the multiplication (NT = 1) / the fold (NT = 2): load, scalars to canonical integers, chain, store Jacobian.
// kraw[t]: the scalar's 8 x 32-bit limbs as the entry received them (Montgomery residue or canonical integer).
template <class C, bool LAZY, int NT>
ARK_HD void pv_chain_point(const char* in0, const char* in1, int form, const u32 (&kraw)[NT][8], int mont, char* out, char* tab,
                           size_t lane, size_t nlanes) {
  typedef typename C::F F;
  typedef Fp<typename C::S> S;
  static_assert(S::N == 8, "256-bit scalar fields");
  XYZZ<F> p[NT];
  u32 kc[NT][8];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    p[t] = pv_load_point<C>(t == 0 ? in0 : in1, form);
    S s;
#pragma unroll
    for (int i = 0; i < 8; i++) s.l[i] = kraw[t][i];
    if (mont) s = S::from_mont(s);   // group.rs: into_bigint
#pragma unroll
    for (int i = 0; i < 8; i++) kc[t][i] = s.l[i];
  }
  XYZZ<F> r;
  if constexpr (LAZY) r = pv_chain<PvLazy<C>, NT>(p, kc, tab, lane, nlanes);
  else r = pv_chain<PvSat<C>, NT>(p, kc, tab, lane, nlanes);
  xyzz_to_jac<F>(r).store(out);
}

// out = a +- b, Projective in and out: the full addition with all its branches (either side at infinity, a = b, a = -b)
template <class C>
ARK_HD void pv_add_point(const char* a, const char* b, int negate_b, char* out) {
  typedef typename C::F F;
  XYZZ<F> p = pv_load_point<C>(a, PV_FORM_PROJECTIVE);
  XYZZ<F> q = pv_load_point<C>(b, PV_FORM_PROJECTIVE);
  if (negate_b) q = XYZZ<F>::neg(q);
  xyzz_add<F>(p, q);
  xyzz_to_jac<F>(p).store(out);
}

// lanes [first, first + nlanes) of a vector of n.  k: n scalars (kstride = 8 words), one shared scalar (kstride = 0), or null:
// the scalars come by value in imm (always so for a fold; then they sit in scalar registers and the digits are wave-uniform).
template <class C, bool LAZY, int NT>
__global__ void __launch_bounds__(64) pv_chain_kernel(const char* in0, const char* in1, int form, const u32* k, size_t kstride,
                                                      PvImm<NT> imm, int mont, size_t first, size_t n, char* out, char* tab,
                                                      size_t nlanes) {
  typedef typename C::F F;
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = first + lane;
  if (lane >= nlanes || i >= n) return;
  const size_t pb = pv_point_bytes<C>(form);
  u32 kraw[NT][8];
#pragma unroll
  for (int t = 0; t < NT; t++) {
#pragma unroll
    for (int j = 0; j < 8; j++) kraw[t][j] = imm.w[t][j];
  }
  if (k) {
#pragma unroll
    for (int j = 0; j < 8; j++) kraw[0][j] = k[i * kstride + j];
  }
  pv_chain_point<C, LAZY, NT>(in0 + i * pb, NT > 1 ? in1 + i * pb : nullptr, form, kraw, mont, out + i * Jac<F>::BYTES, tab, lane,
                              nlanes);
}

template <class C>
__global__ void __launch_bounds__(128) pv_add_kernel(const char* a, const char* b, int negate_b, size_t n, char* out) {
  typedef typename C::F F;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pv_add_point<C>(a + i * Jac<F>::BYTES, b + i * Jac<F>::BYTES, negate_b, out + i * Jac<F>::BYTES);
}

// the carry-free form serves the G1 curves (one Fp element per lane); over Fp2 a lane holds a whole element on saturated limbs
template <class C>
constexpr bool pv_has_lazy() { return C::LAZY_A && C::FA::LANES == 1; }

// bytes of table scratch for `lanes` lanes of a launch with nt tables
template <class C>
size_t pv_table_bytes(int nt, size_t lanes) { return (size_t)nt * 8 * lanes * XYZZ<typename C::F>::BYTES; }

// d_tab: pv_table_bytes<C>(NT, slab) bytes.  The vector is walked in slabs of `slab` lanes, one launch each, all on `s`: a slab's
// lanes read and write their own elements only, so d_out may be d_in0 / d_in1 when the form is Projective.
template <class C, int NT>
int pv_chain_launch(const void* d_in0, const void* d_in1, int form, const void* d_k, size_t kstride, const PvImm<NT>& imm, int mont,
                    size_t n, void* d_out, void* d_tab, size_t slab, hipStream_t s) {
  if (n == 0) return 0;
  if (slab > n) slab = n;
  bool lazy = false;
  if constexpr (pv_has_lazy<C>()) lazy = msm_lazy_enabled();
  const unsigned nb = (unsigned)((slab + 63) / 64);
  for (size_t f = 0; f < n; f += slab) {
    if constexpr (pv_has_lazy<C>()) {
      if (lazy)
        hipLaunchKernelGGL((pv_chain_kernel<C, true, NT>), dim3(nb), dim3(64), 0, s, (const char*)d_in0, (const char*)d_in1, form,
                           (const u32*)d_k, kstride, imm, mont, f, n, (char*)d_out, (char*)d_tab, slab);
    }
    if (!lazy)
      hipLaunchKernelGGL((pv_chain_kernel<C, false, NT>), dim3(nb), dim3(64), 0, s, (const char*)d_in0, (const char*)d_in1, form,
                         (const u32*)d_k, kstride, imm, mont, f, n, (char*)d_out, (char*)d_tab, slab);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

template <class C>
int pv_add_launch(const void* d_a, const void* d_b, int negate_b, size_t n, void* d_out, hipStream_t s) {
  if (n == 0) return 0;
  const size_t blocks = (n + 127) / 128;
  if (blocks > 0x7fffffffull) return -2;   // ARK_HIP_ERR_SIZE
  hipLaunchKernelGGL((pv_add_kernel<C>), dim3((unsigned)blocks), dim3(128), 0, s, (const char*)d_a, (const char*)d_b, negate_b, n,
                     (char*)d_out);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// ---- the host twins: the same per-lane functions on the calling thread, no device involved ----
// impl: 0 = the form the device entry runs by default (carry-free for G1, saturated for G2), 1 = saturated
template <class C, int NT>
void pv_chain_host(const uint64_t* in0, const uint64_t* in1, int form, const uint64_t* k, size_t kstride_words, const uint64_t* a4,
                   const uint64_t* b4, int mont, int impl, size_t n, uint64_t* out_xyz) {
  typedef typename C::F F;
  std::vector<char> tab(pv_table_bytes<C>(NT, 1));
  const size_t pb = pv_point_bytes<C>(form);
  for (size_t i = 0; i < n; i++) {
    u32 kraw[NT][8];
    for (int j = 0; j < 8; j++) {
      kraw[0][j] = k ? ((const u32*)k)[i * kstride_words + j] : ((const u32*)a4)[j];
      if (NT > 1) kraw[NT - 1][j] = ((const u32*)b4)[j];
    }
    const char* p0 = (const char*)in0 + i * pb;
    const char* p1 = NT > 1 ? (const char*)in1 + i * pb : nullptr;
    char* o = (char*)out_xyz + i * Jac<F>::BYTES;
    if constexpr (pv_has_lazy<C>()) {
      if (impl == 0) {
        pv_chain_point<C, true, NT>(p0, p1, form, kraw, mont, o, tab.data(), 0, 1);
        continue;
      }
    }
    pv_chain_point<C, false, NT>(p0, p1, form, kraw, mont, o, tab.data(), 0, 1);
  }
}
template <class C>
void pv_add_host(const uint64_t* a, const uint64_t* b, int negate_b, size_t n, uint64_t* out_xyz) {
  typedef typename C::F F;
  for (size_t i = 0; i < n; i++)
    pv_add_point<C>((const char*)a + i * Jac<F>::BYTES, (const char*)b + i * Jac<F>::BYTES, negate_b, (char*)out_xyz + i * Jac<F>::BYTES);
}

}  // namespace arkhip
