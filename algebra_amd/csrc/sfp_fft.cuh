// Radix-2 transforms and pointwise kernels over the one-word fields of sfp.cuh.  DESIGN.md section 27.
//
// Decimation in frequency, natural order in and out.  Stage s (0 first) pairs positions i and i + h, h = n >> (s + 1), and
// multiplies the difference by w^((i mod h) << s); after log n stages position i holds X[bitrev(i)].  A pass (sfp_plan.hpp) runs
// consecutive stages s0 .. s0 + m - 1 on a tile in LDS:
//   strided pass:  the tile is 2^m rows, 2^L apart (L = log n - s0 - m), by 2^cb consecutive positions; rows are transformed,
//                  the columns only make the global accesses contiguous.  Reads and writes the same positions: in place.
//   last pass:     the tile is 2^cb sub-transforms of 2^m consecutive positions, 2^(log n - cb) apart, so that after the bit
//                  reversal their outputs are 2^cb neighbours: the bit-reversed write-back moves whole segments.  It reads one
//                  buffer and writes another (or, with one workgroup per column, its own column).
// Fused: the coset's h^i into the first pass's loads (together with the zero padding behind num_coeffs), n^-1 * h^-i into the
// last pass's stores.  Twiddles: one compact table per stage, w^(j << s) for j < n >> (s + 1) at offset n - (n >> s) of one array.
// Powers: g^i = hi[i >> lo_bits] * lo[i & mask], two tables of about sqrt(n) entries, the constant folded into hi.
#pragma once
#include "sfp.cuh"
#include "sfp_plan.hpp"
#include "../../include/ark_hip.h"
#include <stdio.h>

namespace arkhip {

#define SFP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      fprintf(stderr, "ark_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return -(int)_e - 1000;                                                                      \
    }                                                                                              \
  } while (0)

struct SfpPow32 { uint64_t v[32]; };   // x^(2^i), as stored

enum { SFP_SCALE_NONE = 0, SFP_SCALE_CONST = 1, SFP_SCALE_TABLE = 2 };
struct SfpScale {
  int mode;            // SFP_SCALE_*
  uint64_t k;          // CONST: the factor, as stored
  const void* hi;      // TABLE: k * g^(u << lo_bits)
  const void* lo;      //        g^v, v < 2^lo_bits
};
struct SfpPassArgs {
  const void* src;
  void* dst;
  size_t src_stride, dst_stride;   // elements between columns
  size_t num_coeffs;               // positions >= num_coeffs of a column read as zero
  int k, s0, m, cb;
  unsigned groups;                 // workgroups per column: n >> (m + cb)
  const void* tw;                  // the per-stage tables
  SfpScale ld, st;                 // applied to the loads (by natural position) and to the stores (last pass: by output position)
  int lo_bits;
};
// one call: what SmallFieldOps::fft gets
struct SfpFftArgs {
  void* data;
  void* ping;                      // count * n elements, used when the plan has more than one pass
  size_t count, stride, num_coeffs;
  int k;
  SfpPlan plan;
  const void* tw;
  SfpScale pre, post;              // the first pass's loads, the last pass's stores
  int lo_bits;
};

template <class F>
__device__ inline typename F::T sfp_scaled(typename F::T v, size_t i, const SfpScale& sc, int lo_bits) {
  using T = typename F::T;
  if (sc.mode == SFP_SCALE_CONST) return F::mul(v, (T)sc.k);
  if (sc.mode == SFP_SCALE_TABLE)
    return F::mul(v, F::mul(((const T*)sc.hi)[i >> lo_bits], ((const T*)sc.lo)[i & (((size_t)1 << lo_bits) - 1)]));
  return v;
}
__device__ inline unsigned sfp_bitrev(unsigned x, int bits) { return bits ? __brev(x) >> (32 - bits) : 0u; }

template <class Cfg, bool LAST, int THREADS>
__global__ __launch_bounds__(THREADS) void sfp_fft_pass_kernel(const SfpPassArgs a) {
  using F = SFp<Cfg>;
  using T = typename Cfg::T;
  constexpr int TILE_LOG = sizeof(T) == 8 ? 12 : 13, SEG_LOG = sizeof(T) == 8 ? 4 : 5;
  __shared__ T sh[((size_t)1 << TILE_LOG) + ((size_t)1 << SEG_LOG)];
  const unsigned tid = threadIdx.x;
  const unsigned g = blockIdx.x % a.groups;
  const size_t col = blockIdx.x / a.groups;
  const int k = a.k, m = a.m, cb = a.cb;
  const size_t n = (size_t)1 << k;
  const unsigned tile = 1u << (m + cb);
  const T* src = (const T*)a.src + col * a.src_stride;
  T* dst = (T*)a.dst + col * a.dst_stride;
  const T* tw = (const T*)a.tw;
  if constexpr (!LAST) {
    const int L = k - a.s0 - m;
    const unsigned cmask = (1u << cb) - 1;
    const size_t lblk = g & (((size_t)1 << (L - cb)) - 1), H = g >> (L - cb);
    const size_t base = (H << (k - a.s0)) | (lblk << cb);
    for (unsigned e = tid; e < tile; e += THREADS) {
      const size_t i = base | ((size_t)(e >> cb) << L) | (e & cmask);
      T v = i < a.num_coeffs ? src[i] : (T)0;
      sh[e] = sfp_scaled<F>(v, i, a.ld, a.lo_bits);
    }
    __syncthreads();
    for (int t = 0; t < m; t++) {
      const int s = a.s0 + t;
      const unsigned hr = 1u << (m - 1 - t);
      const T* tws = tw + (n - (n >> s));
#pragma unroll 4
      for (unsigned b = tid; b < (tile >> 1); b += THREADS) {
        const unsigned c = b & cmask, q = b >> cb, rlow = q & (hr - 1);
        const unsigned r = ((q >> (m - 1 - t)) << (m - t)) | rlow;
        const unsigned e0 = (r << cb) | c, e1 = e0 + (hr << cb);
        const size_t j = ((size_t)rlow << L) | (lblk << cb) | c;
        const T x = sh[e0], y = sh[e1];
        sh[e0] = F::add(x, y);
        sh[e1] = F::mul(F::sub(x, y), tws[j]);
      }
      __syncthreads();
    }
    for (unsigned e = tid; e < tile; e += THREADS) {
      const size_t i = base | ((size_t)(e >> cb) << L) | (e & cmask);
      dst[i] = sh[e];
    }
  } else {
    // sub-transform cc of the tile starts at natural position cc << (k - cb) | g << m; LDS row pitch 2^m + 1 keeps the column
    // reads of the write-back off one bank
    const unsigned pitch = cb ? (1u << m) + 1 : (1u << m);
    const unsigned rmask = (1u << m) - 1;
    for (unsigned x = tid; x < tile; x += THREADS) {
      const unsigned r = x & rmask, cc = x >> m;
      const size_t i = ((size_t)cc << (k - cb)) | ((size_t)g << m) | r;
      const T v = i < a.num_coeffs ? src[i] : (T)0;
      sh[cc * pitch + r] = sfp_scaled<F>(v, i, a.ld, a.lo_bits);
    }
    __syncthreads();
    for (int t = 0; t < m; t++) {
      const int s = a.s0 + t;
      const unsigned hr = 1u << (m - 1 - t);
      const T* tws = tw + (n - (n >> s));
#pragma unroll 4
      for (unsigned b = tid; b < (tile >> 1); b += THREADS) {
        const unsigned p = b & (rmask >> 1), cc = b >> (m - 1), rlow = p & (hr - 1);
        const unsigned r = ((p >> (m - 1 - t)) << (m - t)) | rlow;
        const unsigned e0 = cc * pitch + r, e1 = e0 + hr;
        const T x = sh[e0], y = sh[e1];
        sh[e0] = F::add(x, y);
        sh[e1] = F::mul(F::sub(x, y), tws[rlow]);
      }
      __syncthreads();
    }
    const unsigned grev = sfp_bitrev(g, k - m - cb);
    for (unsigned x = tid; x < tile; x += THREADS) {
      const unsigned oc = x & ((1u << cb) - 1), orow = x >> cb;
      const unsigned cc = sfp_bitrev(oc, cb), r = sfp_bitrev(orow, m);
      const size_t o = ((size_t)orow << (k - m)) | ((size_t)grev << cb) | oc;
      dst[o] = sfp_scaled<F>(sh[cc * pitch + r], o, a.st, a.lo_bits);
    }
  }
}

// every transform of one call: count columns of n = 2^k elements
template <class Cfg>
int sfp_fft_run(const SfpFftArgs& f, hipStream_t st) {
  const SfpPlan& pl = f.plan;
  const size_t n = (size_t)1 << f.k;
  int s0 = 0;
  for (int pass = 0; pass < pl.npasses; pass++) {
    const int m = pl.stages[pass];
    const bool last = pass == pl.npasses - 1;
    SfpPassArgs a{};
    a.k = f.k;
    a.s0 = s0;
    a.m = m;
    a.tw = f.tw;
    a.num_coeffs = pass == 0 ? f.num_coeffs : n;
    a.lo_bits = f.lo_bits;
    // buffers: in place up to the last two passes, which go data -> ping -> data
    const bool from_ping = last && pl.npasses > 1, to_ping = pass == pl.npasses - 2;
    a.src = from_ping ? f.ping : f.data;
    a.src_stride = from_ping ? n : f.stride;
    a.dst = to_ping ? f.ping : f.data;
    a.dst_stride = to_ping ? n : f.stride;
    if (pass == 0) a.ld = f.pre;
    if (last) {
      a.cb = pl.npasses > 1 ? pl.seg_log : 0;
      a.st = f.post;
    } else {
      const int L = f.k - s0 - m;
      a.cb = pl.tile_log - m < L ? pl.tile_log - m : L;
    }
    const size_t groups = n >> (m + a.cb), blocks = groups * f.count;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return ARK_HIP_ERR_SIZE;
    a.groups = (unsigned)groups;
    const bool wide = sfp_pass_threads(blocks) == SFP_THREADS_WIDE;
    if (last && wide)
      hipLaunchKernelGGL((sfp_fft_pass_kernel<Cfg, true, SFP_THREADS_WIDE>), dim3((unsigned)blocks), dim3(SFP_THREADS_WIDE), 0, st, a);
    else if (last)
      hipLaunchKernelGGL((sfp_fft_pass_kernel<Cfg, true, SFP_THREADS>), dim3((unsigned)blocks), dim3(SFP_THREADS), 0, st, a);
    else if (wide)
      hipLaunchKernelGGL((sfp_fft_pass_kernel<Cfg, false, SFP_THREADS_WIDE>), dim3((unsigned)blocks), dim3(SFP_THREADS_WIDE), 0, st, a);
    else
      hipLaunchKernelGGL((sfp_fft_pass_kernel<Cfg, false, SFP_THREADS>), dim3((unsigned)blocks), dim3(SFP_THREADS), 0, st, a);
    SFP_TRY(hipGetLastError());
    s0 += m;
  }
  return 0;
}

// ---- tables ---------------------------------------------------------------------------------------------------------------
template <class F>
__device__ inline typename F::T sfp_pow_bits(const SfpPow32& pw, uint64_t e) {   // x^e from x^(2^i): one product per set bit
  typename F::T r = F::ONE;
  for (int i = 0; e; e >>= 1, i++)
    if (e & 1) r = F::mul(r, (typename F::T)pw.v[i]);
  return r;
}
// out[n - (n >> s) + j] = w^(j << s), j < n >> (s + 1), s < k: n - 1 entries
template <class Cfg>
__global__ __launch_bounds__(256) void sfp_twiddle_kernel(typename Cfg::T* out, int k, const SfpPow32 pw) {
  using F = SFp<Cfg>;
  const size_t n = (size_t)1 << k;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx + 1 >= n) return;
  const size_t r = n - idx;                              // in (n >> (s + 1), n >> s]
  const int s = k - 1 - (63 - __clzll((unsigned long long)(r - 1)));
  const size_t j = idx - (n - (n >> s));
  out[idx] = sfp_pow_bits<F>(pw, (uint64_t)j << s);
}
// hi[u] = scale * g^(u << lo_bits), u < nhi; lo[v] = g^v, v < 2^lo_bits
template <class Cfg>
__global__ __launch_bounds__(256) void sfp_power_kernel(typename Cfg::T* hi, typename Cfg::T* lo, size_t nhi, int lo_bits,
                                                        const SfpPow32 pw, uint64_t scale) {
  using F = SFp<Cfg>;
  using T = typename Cfg::T;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t nlo = (size_t)1 << lo_bits;
  if (idx < nhi)
    hi[idx] = F::mul((T)scale, sfp_pow_bits<F>(pw, (uint64_t)idx << lo_bits));
  else if (idx - nhi < nlo)
    lo[idx - nhi] = sfp_pow_bits<F>(pw, (uint64_t)(idx - nhi));
}
template <class Cfg>
int sfp_twiddles_run(void* d_out, int k, const SfpPow32& pw, hipStream_t st) {
  const size_t n = (size_t)1 << k;
  if (n < 2) return 0;
  const size_t blocks = (n - 1 + 255) / 256;
  if (blocks > 0x7FFFFFFFull) return ARK_HIP_ERR_SIZE;
  hipLaunchKernelGGL((sfp_twiddle_kernel<Cfg>), dim3((unsigned)blocks), dim3(256), 0, st, (typename Cfg::T*)d_out, k, pw);
  SFP_TRY(hipGetLastError());
  return 0;
}
template <class Cfg>
int sfp_powers_run(void* d_hi, void* d_lo, size_t nhi, int lo_bits, const SfpPow32& pw, uint64_t scale, hipStream_t st) {
  const size_t total = nhi + ((size_t)1 << lo_bits);
  hipLaunchKernelGGL((sfp_power_kernel<Cfg>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (typename Cfg::T*)d_hi,
                     (typename Cfg::T*)d_lo, nhi, lo_bits, pw, scale);
  SFP_TRY(hipGetLastError());
  return 0;
}

// ---- pointwise kernels ----------------------------------------------------------------------------------------------------
// V elements per thread and access: 16 bytes (one dwordx4) when every pointer is 16-byte aligned, else 1.  r may alias a or b:
// a thread reads its own chunk of both before it writes it.
template <class F, int OP, int V>
__device__ inline void sfp_vec_apply(const typename F::T* x, const typename F::T* y, typename F::T k, typename F::T* out) {
  using T = typename F::T;
  if constexpr (OP == SFP_OP_INVERSE) {
    // Montgomery's trick over the run, zeros stepped over: one Fermat inversion per V elements
    T pre[V];
    T acc = F::ONE;
    for (int i = 0; i < V; i++) {
      pre[i] = acc;
      if (x[i]) acc = F::mul(acc, x[i]);
    }
    T inv = F::inv(acc);
    for (int i = V - 1; i >= 0; i--) {
      if (x[i]) {
        out[i] = F::mul(inv, pre[i]);
        inv = F::mul(inv, x[i]);
      } else {
        out[i] = 0;
      }
    }
  } else {
    for (int i = 0; i < V; i++) {
      if constexpr (OP == SFP_OP_ADD) out[i] = F::add(x[i], y[i]);
      if constexpr (OP == SFP_OP_SUB) out[i] = F::sub(x[i], y[i]);
      if constexpr (OP == SFP_OP_MUL) out[i] = F::mul(x[i], y[i]);
      if constexpr (OP == SFP_OP_NEG) out[i] = F::neg(x[i]);
      if constexpr (OP == SFP_OP_SCALE) out[i] = F::mul(x[i], k);
      if constexpr (OP == SFP_OP_FROM_CANONICAL) out[i] = F::from_canonical(x[i]);
      if constexpr (OP == SFP_OP_INTO_CANONICAL) out[i] = F::into_canonical(x[i]);
    }
  }
}
template <class Cfg, int OP, int V>
__global__ __launch_bounds__(256) void sfp_vec_kernel(const typename Cfg::T* a, const typename Cfg::T* b, typename Cfg::T k,
                                                      typename Cfg::T* r, size_t n) {
  using F = SFp<Cfg>;
  using T = typename Cfg::T;
  typedef T VT __attribute__((ext_vector_type(V)));
  constexpr bool BINARY = OP == SFP_OP_ADD || OP == SFP_OP_SUB || OP == SFP_OP_MUL;
  const size_t chunks = n / V, step = (size_t)gridDim.x * 256;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t ch = gid; ch < chunks; ch += step) {
    T x[V], y[V], o[V];
    if constexpr (V > 1) {
      const VT vx = ((const VT*)a)[ch];
      for (int i = 0; i < V; i++) x[i] = vx[i];
      if constexpr (BINARY) {
        const VT vy = ((const VT*)b)[ch];
        for (int i = 0; i < V; i++) y[i] = vy[i];
      }
    } else {
      x[0] = a[ch];
      if constexpr (BINARY) y[0] = b[ch];
    }
    sfp_vec_apply<F, OP, V>(x, y, k, o);
    if constexpr (V > 1) {
      VT vo;
      for (int i = 0; i < V; i++) vo[i] = o[i];
      ((VT*)r)[ch] = vo;
    } else {
      r[ch] = o[0];
    }
  }
  if constexpr (V > 1) {   // the tail behind the last whole chunk: one element per thread
    const size_t i = chunks * V + gid;
    if (i < n) {
      T x = a[i], y = 0, o;
      if constexpr (BINARY) y = b[i];
      sfp_vec_apply<F, OP, 1>(&x, &y, k, &o);
      r[i] = o;
    }
  }
}
template <class Cfg, int OP>
int sfp_vec_launch_op(const void* a, const void* b, uint64_t k, void* r, size_t n, hipStream_t st) {
  using T = typename Cfg::T;
  if (n == 0) return 0;
  constexpr int V = 16 / (int)sizeof(T);
  const bool aligned = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)r) & 15) == 0;
  const size_t work = aligned ? (n + V - 1) / V : n;
  size_t blocks = (work + 255) / 256;
  if (blocks > (1u << 16)) blocks = 1u << 16;   // grid-stride beyond
  if (blocks * 256 < (size_t)V) blocks = 1;
  if (aligned)
    hipLaunchKernelGGL((sfp_vec_kernel<Cfg, OP, V>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)a, (const T*)b, (T)k, (T*)r, n);
  else
    hipLaunchKernelGGL((sfp_vec_kernel<Cfg, OP, 1>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)a, (const T*)b, (T)k, (T*)r, n);
  SFP_TRY(hipGetLastError());
  return 0;
}
template <class Cfg>
int sfp_vec_launch(int op, const void* a, const void* b, uint64_t k, void* r, size_t n, hipStream_t st) {
  switch (op) {
    case SFP_OP_ADD: return sfp_vec_launch_op<Cfg, SFP_OP_ADD>(a, b, k, r, n, st);
    case SFP_OP_SUB: return sfp_vec_launch_op<Cfg, SFP_OP_SUB>(a, b, k, r, n, st);
    case SFP_OP_MUL: return sfp_vec_launch_op<Cfg, SFP_OP_MUL>(a, b, k, r, n, st);
    case SFP_OP_NEG: return sfp_vec_launch_op<Cfg, SFP_OP_NEG>(a, b, k, r, n, st);
    case SFP_OP_SCALE: return sfp_vec_launch_op<Cfg, SFP_OP_SCALE>(a, b, k, r, n, st);
    case SFP_OP_INVERSE: return sfp_vec_launch_op<Cfg, SFP_OP_INVERSE>(a, b, k, r, n, st);
    case SFP_OP_FROM_CANONICAL: return sfp_vec_launch_op<Cfg, SFP_OP_FROM_CANONICAL>(a, b, k, r, n, st);
    case SFP_OP_INTO_CANONICAL: return sfp_vec_launch_op<Cfg, SFP_OP_INTO_CANONICAL>(a, b, k, r, n, st);
  }
  return ARK_HIP_ERR_ARG;
}

}  // namespace arkhip
