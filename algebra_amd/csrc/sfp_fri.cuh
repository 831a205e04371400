// Kernels on extension-field vectors over the one-word fields (sfpx.cuh): pointwise products and inverses, the combination of
// base-field columns by powers of an extension challenge, and the FRI fold.  DESIGN.md section 30.
//
// An extension vector of n elements is D columns of n base-field words: component k of element i at p[k * stride + i],
// stride >= n -- the matrix layout of sfp_fft.cuh and merkle.cuh.  Every kernel runs 256 threads per workgroup, one lane per
// chunk of V consecutive elements: V words are one 16-byte access when every pointer and every stride is 16-byte aligned, V = 1 otherwise
// (and always for the arity-8 fold).  Challenges and constants travel in the kernel
// arguments: no host memory is read after a launch returns.  No LDS, no scratch memory, no atomics.
#pragma once
#include "sfp_fft.cuh"
#include "sfpx.cuh"

namespace arkhip {

enum { SFPX_OP_MUL = 0, SFPX_OP_INVERSE = 1, SFPX_OP_MUL_CONST = 2, SFPX_OP_MUL_BASE = 3 };
struct SfpxConst { uint64_t c[4]; };   // one extension element as stored, the upper words zero for D = 2
enum { SFPX_COMBINE_BLOCK = 8 };
struct SfpCombineArgs {
  uint64_t pw[SFPX_COMBINE_BLOCK + 1][4];   // alpha^0 .. alpha^8
  uint64_t first[4];                        // alpha^first_power
};
struct SfpFoldArgs {
  const void* in;
  void* out;
  size_t stride_in, stride_out;
  int k;                 // log n of the input layer
  int lo_bits;           // the power table's split: (2 h w^i)^-1 = hi[i >> lo_bits] * lo[i & mask]
  const void* hi;
  const void* lo;
  SfpFoldRoots roots;
  SfpxConst beta;
};

template <class Cfg>
__host__ __device__ inline typename SFpX<Cfg>::E sfpx_elem(const uint64_t* w) {
  typename SFpX<Cfg>::E e;
#pragma unroll
  for (int k = 0; k < SFpX<Cfg>::D; k++) e.c[k] = (typename Cfg::T)w[k];
  return e;
}

// V consecutive elements of an extension vector, component by component
template <class Cfg, int V>
__device__ inline void sfpx_load(const typename Cfg::T* p, size_t stride, size_t first, typename SFpX<Cfg>::E* x) {
  using T = typename Cfg::T;
  typedef T VT __attribute__((ext_vector_type(V)));
#pragma unroll
  for (int k = 0; k < SFpX<Cfg>::D; k++) {
    if constexpr (V > 1) {
      const VT v = *(const VT*)(p + k * stride + first);
#pragma unroll
      for (int i = 0; i < V; i++) x[i].c[k] = v[i];
    } else {
      x[0].c[k] = p[k * stride + first];
    }
  }
}
template <class Cfg, int V>
__device__ inline void sfpx_store(typename Cfg::T* p, size_t stride, size_t first, const typename SFpX<Cfg>::E* x) {
  using T = typename Cfg::T;
  typedef T VT __attribute__((ext_vector_type(V)));
#pragma unroll
  for (int k = 0; k < SFpX<Cfg>::D; k++) {
    if constexpr (V > 1) {
      VT v;
#pragma unroll
      for (int i = 0; i < V; i++) v[i] = x[i].c[k];
      *(VT*)(p + k * stride + first) = v;
    } else {
      p[k * stride + first] = x[0].c[k];
    }
  }
}
template <class Cfg, int V>
__device__ inline void sfpx_load_base(const typename Cfg::T* p, size_t first, typename Cfg::T* x) {
  using T = typename Cfg::T;
  typedef T VT __attribute__((ext_vector_type(V)));
  if constexpr (V > 1) {
    const VT v = *(const VT*)(p + first);
#pragma unroll
    for (int i = 0; i < V; i++) x[i] = v[i];
  } else {
    x[0] = p[first];
  }
}

// ---- pointwise ------------------------------------------------------------------------------------------------------------
template <class Cfg, int OP, int V>
__device__ inline void sfpx_vec_chunk(const typename Cfg::T* a, size_t sa, const typename Cfg::T* b, size_t sb,
                                      const typename SFpX<Cfg>::E& k, typename Cfg::T* r, size_t sr, size_t first) {
  using X = SFpX<Cfg>;
  using E = typename X::E;
  using T = typename Cfg::T;
  E x[V], o[V];
  sfpx_load<Cfg, V>(a, sa, first, x);
  if constexpr (OP == SFPX_OP_MUL) {
    E y[V];
    sfpx_load<Cfg, V>(b, sb, first, y);
#pragma unroll
    for (int i = 0; i < V; i++) o[i] = X::mul(x[i], y[i]);
  } else if constexpr (OP == SFPX_OP_MUL_BASE) {
    T y[V];
    sfpx_load_base<Cfg, V>(b, first, y);
#pragma unroll
    for (int i = 0; i < V; i++) o[i] = X::mul_base(x[i], y[i]);
  } else if constexpr (OP == SFPX_OP_MUL_CONST) {
#pragma unroll
    for (int i = 0; i < V; i++) o[i] = X::mul(x[i], k);
  } else if constexpr (V == 1) {
    o[0] = X::inv(x[0]);
  } else {
    // Montgomery's trick over the chunk, zeros stepped over: one inversion (one base-field inversion) per V elements
    E pre[V];
    E acc = X::one();
#pragma unroll
    for (int i = 0; i < V; i++) {
      pre[i] = acc;
      if (!X::is_zero(x[i])) acc = X::mul(acc, x[i]);
    }
    E inv = X::inv(acc);
#pragma unroll
    for (int i = V - 1; i >= 0; i--) {
      if (!X::is_zero(x[i])) {
        o[i] = X::mul(inv, pre[i]);
        inv = X::mul(inv, x[i]);
      } else {
        o[i] = X::zero();
      }
    }
  }
  sfpx_store<Cfg, V>(r, sr, first, o);
}
// r may be a or b itself: a lane reads its own chunk of both before it writes it
template <class Cfg, int OP, int V>
__global__ __launch_bounds__(256) void sfpx_vec_kernel(const typename Cfg::T* a, size_t sa, const typename Cfg::T* b, size_t sb,
                                                       const SfpxConst kc, typename Cfg::T* r, size_t sr, size_t n) {
  const typename SFpX<Cfg>::E k = sfpx_elem<Cfg>(kc.c);
  const size_t chunks = n / V, step = (size_t)gridDim.x * 256;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t ch = gid; ch < chunks; ch += step) sfpx_vec_chunk<Cfg, OP, V>(a, sa, b, sb, k, r, sr, ch * V);
  if constexpr (V > 1) {   // the tail behind the last whole chunk: one element per lane
    const size_t i = chunks * V + gid;
    if (i < n) sfpx_vec_chunk<Cfg, OP, 1>(a, sa, b, sb, k, r, sr, i);
  }
}
inline unsigned sfpx_blocks(size_t work) {
  size_t blocks = (work + 255) / 256;
  if (blocks > (1u << 16)) blocks = 1u << 16;   // grid-stride beyond
  return blocks ? (unsigned)blocks : 1u;
}
inline bool sfpx_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
template <class Cfg, int OP>
int sfpx_vec_launch_op(const void* a, size_t sa, const void* b, size_t sb, const SfpxConst& k, void* r, size_t sr, size_t n,
                       hipStream_t st) {
  using T = typename Cfg::T;
  if (n == 0) return 0;
  constexpr int V = 16 / (int)sizeof(T);
  bool aligned = sfpx_aligned16(a) && sfpx_aligned16(r) && (sa * sizeof(T)) % 16 == 0 && (sr * sizeof(T)) % 16 == 0;
  if (OP == SFPX_OP_MUL) aligned = aligned && sfpx_aligned16(b) && (sb * sizeof(T)) % 16 == 0;
  if (OP == SFPX_OP_MUL_BASE) aligned = aligned && sfpx_aligned16(b);
  // the tail of the wide kernel runs one element per lane of the same grid: at least V - 1 lanes
  const unsigned blocks = sfpx_blocks(aligned ? (n + V - 1) / V : n);
  if (aligned)
    hipLaunchKernelGGL((sfpx_vec_kernel<Cfg, OP, V>), dim3(blocks), dim3(256), 0, st, (const T*)a, sa, (const T*)b, sb, k, (T*)r, sr, n);
  else
    hipLaunchKernelGGL((sfpx_vec_kernel<Cfg, OP, 1>), dim3(blocks), dim3(256), 0, st, (const T*)a, sa, (const T*)b, sb, k, (T*)r, sr, n);
  SFP_TRY(hipGetLastError());
  return 0;
}
template <class Cfg>
int sfpx_vec_launch(int op, const void* a, size_t sa, const void* b, size_t sb, const SfpxConst& k, void* r, size_t sr, size_t n,
                    hipStream_t st) {
  switch (op) {
    case SFPX_OP_MUL: return sfpx_vec_launch_op<Cfg, SFPX_OP_MUL>(a, sa, b, sb, k, r, sr, n, st);
    case SFPX_OP_INVERSE: return sfpx_vec_launch_op<Cfg, SFPX_OP_INVERSE>(a, sa, b, sb, k, r, sr, n, st);
    case SFPX_OP_MUL_CONST: return sfpx_vec_launch_op<Cfg, SFPX_OP_MUL_CONST>(a, sa, b, sb, k, r, sr, n, st);
    case SFPX_OP_MUL_BASE: return sfpx_vec_launch_op<Cfg, SFPX_OP_MUL_BASE>(a, sa, b, sb, k, r, sr, n, st);
  }
  return ARK_HIP_ERR_ARG;
}

// ---- combine: out[i] (+)= alpha^first_power * sum_j alpha^j col_j[i] ------------------------------------------------------------
// Horner over blocks of eight columns from the last block: inside a block a column costs D base-field products by the constant
// alpha^j, a block one extension product by alpha^8.
template <class Cfg, int V>
__device__ inline void sfpx_combine_chunk(const typename Cfg::T* cols, size_t count, size_t stride, const SfpCombineArgs& ar,
                                          typename Cfg::T* out, size_t so, int accumulate, size_t first) {
  using X = SFpX<Cfg>;
  using F = SFp<Cfg>;
  using E = typename X::E;
  using T = typename Cfg::T;
  constexpr int B = SFPX_COMBINE_BLOCK;
  const E a8 = sfpx_elem<Cfg>(ar.pw[B]);
  E acc[V];
  const size_t nb = (count + B - 1) / B;
  for (size_t b = nb; b-- > 0;) {
    E inner[V];
#pragma unroll
    for (int i = 0; i < V; i++) inner[i] = X::zero();
#pragma unroll
    for (int j = 0; j < B; j++) {
      const size_t col = b * B + j;
      if (col < count) {
        T c[V];
        sfpx_load_base<Cfg, V>(cols + col * stride, first, c);
#pragma unroll
        for (int i = 0; i < V; i++) {
          if (j == 0) {
            inner[i].c[0] = F::add(inner[i].c[0], c[i]);
          } else {
#pragma unroll
            for (int k = 0; k < X::D; k++) inner[i].c[k] = F::add(inner[i].c[k], F::mul((T)ar.pw[j][k], c[i]));
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < V; i++) acc[i] = b == nb - 1 ? inner[i] : X::add(X::mul(acc[i], a8), inner[i]);
  }
  const E fp = sfpx_elem<Cfg>(ar.first);
#pragma unroll
  for (int i = 0; i < V; i++) acc[i] = X::mul(acc[i], fp);
  if (accumulate) {
    E old[V];
    sfpx_load<Cfg, V>(out, so, first, old);
#pragma unroll
    for (int i = 0; i < V; i++) acc[i] = X::add(acc[i], old[i]);
  }
  sfpx_store<Cfg, V>(out, so, first, acc);
}
template <class Cfg, int V>
__global__ __launch_bounds__(256) void sfpx_combine_kernel(const typename Cfg::T* cols, size_t count, size_t stride, size_t rows,
                                                           const SfpCombineArgs ar, typename Cfg::T* out, size_t so, int accumulate) {
  const size_t chunks = rows / V, step = (size_t)gridDim.x * 256;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t ch = gid; ch < chunks; ch += step) sfpx_combine_chunk<Cfg, V>(cols, count, stride, ar, out, so, accumulate, ch * V);
  if constexpr (V > 1) {
    const size_t i = chunks * V + gid;
    if (i < rows) sfpx_combine_chunk<Cfg, 1>(cols, count, stride, ar, out, so, accumulate, i);
  }
}
template <class Cfg>
int sfpx_combine_launch(const void* cols, size_t count, size_t stride, size_t rows, const SfpCombineArgs& ar, void* out, size_t so,
                        int accumulate, hipStream_t st) {
  using T = typename Cfg::T;
  if (rows == 0) return 0;
  constexpr int V = 16 / (int)sizeof(T);
  const bool aligned = sfpx_aligned16(cols) && sfpx_aligned16(out) && (stride * sizeof(T)) % 16 == 0 && (so * sizeof(T)) % 16 == 0;
  const unsigned blocks = sfpx_blocks(aligned ? (rows + V - 1) / V : rows);
  if (aligned)
    hipLaunchKernelGGL((sfpx_combine_kernel<Cfg, V>), dim3(blocks), dim3(256), 0, st, (const T*)cols, count, stride, rows, ar, (T*)out, so,
                       accumulate);
  else
    hipLaunchKernelGGL((sfpx_combine_kernel<Cfg, 1>), dim3(blocks), dim3(256), 0, st, (const T*)cols, count, stride, rows, ar, (T*)out, so,
                       accumulate);
  SFP_TRY(hipGetLastError());
  return 0;
}

// ---- fold -----------------------------------------------------------------------------------------------------------------
// One lane per V outputs i .. i + V - 1 < m = n >> A: it reads the 2^A inputs i + j m of every output (a wave's loads are
// consecutive for each j and component), folds them in registers (sfpx_fold_row) and writes V outputs.
template <class Cfg, int A, int V>
__global__ __launch_bounds__(256) void sfpx_fold_kernel(const SfpFoldArgs a) {
  using X = SFpX<Cfg>;
  using F = SFp<Cfg>;
  using E = typename X::E;
  using T = typename Cfg::T;
  constexpr int R = 1 << A;
  const size_t m = (size_t)1 << (a.k - A);
  const size_t chunks = m / V, step = (size_t)gridDim.x * 256;   // the launcher picks a V that divides m
  const size_t lo_mask = ((size_t)1 << a.lo_bits) - 1;
  const T* in = (const T*)a.in;
  T* out = (T*)a.out;
  const E beta = sfpx_elem<Cfg>(a.beta.c);
  for (size_t ch = (size_t)blockIdx.x * 256 + threadIdx.x; ch < chunks; ch += step) {
    const size_t i0 = ch * V;
    E v[V][R];
#pragma unroll
    for (int j = 0; j < R; j++) {
      E x[V];
      sfpx_load<Cfg, V>(in, a.stride_in, i0 + (size_t)j * m, x);
#pragma unroll
      for (int i = 0; i < V; i++) v[i][j] = x[i];
    }
    E g[V];
#pragma unroll
    for (int i = 0; i < V; i++) {
      const size_t pos = i0 + i;
      const T t = F::mul(((const T*)a.hi)[pos >> a.lo_bits], ((const T*)a.lo)[pos & lo_mask]);
      g[i] = sfpx_fold_row<Cfg, A>(v[i], t, a.roots, beta);
    }
    sfpx_store<Cfg, V>(out, a.stride_out, i0, g);
  }
}
template <class Cfg, int A>
int sfpx_fold_launch_a(const SfpFoldArgs& a, hipStream_t st) {
  using T = typename Cfg::T;
  // arity 8 keeps 8 D words per output in registers: one output per lane (a wave's loads are still 256 or 512 consecutive bytes)
  constexpr int V = A <= 2 ? 16 / (int)sizeof(T) : 1;
  const size_t m = (size_t)1 << (a.k - A);
  const bool wide = V > 1 && sfpx_aligned16(a.in) && sfpx_aligned16(a.out) && (a.stride_in * sizeof(T)) % 16 == 0 &&
                    (a.stride_out * sizeof(T)) % 16 == 0 && (m * sizeof(T)) % 16 == 0;
  const unsigned blocks = sfpx_blocks(wide ? m / V : m);
  if (wide)
    hipLaunchKernelGGL((sfpx_fold_kernel<Cfg, A, V>), dim3(blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((sfpx_fold_kernel<Cfg, A, 1>), dim3(blocks), dim3(256), 0, st, a);
  SFP_TRY(hipGetLastError());
  return 0;
}
template <class Cfg>
int sfpx_fold_launch(const SfpFoldArgs& a, int log_arity, hipStream_t st) {
  switch (log_arity) {
    case 1: return sfpx_fold_launch_a<Cfg, 1>(a, st);
    case 2: return sfpx_fold_launch_a<Cfg, 2>(a, st);
    case 3: return sfpx_fold_launch_a<Cfg, 3>(a, st);
  }
  return ARK_HIP_ERR_ARG;
}

}  // namespace arkhip
