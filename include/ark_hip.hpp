// ark_hip.hpp -- C++17 host-side mirror of the two reference interfaces that libark_hip.so replaces, written over
// the C ABI of ark_hip.h (header only).  The reference is Rust; this image has no Rust toolchain, so this header is
// the compiled-language host side (the same surface exists as Rust source in rust/ and as a Python mirror in
// algebra_amd/).  Names, argument meaning and error behaviour follow the reference:
//
//   ark_hip::VariableBaseMSM<Curve>      <- ark_ec::VariableBaseMSM for Projective<P>
//        msm(bases, scalars)   -> Result: Err(min_len) when the lengths differ   (ec/src/scalar_mul/variable_base/mod.rs:67-78,
//                                                                                  short_weierstrass/mod.rs:112-119)
//        msm_unchecked(...)    -> truncates to the shorter input                   (mod.rs:59-64)
//        msm_bigint(...)       -> scalars are canonical BigInt<4>                  (mod.rs:80-85)
//        msm_chunks(...)       -> streams aligned at their end, 2^20-pair steps    (mod.rs:119-150)
//   ark_hip::ChunkedPippenger<Curve>, ark_hip::HashMapPippenger<Curve>             (stream_pippenger.rs:10-128)
//   ark_hip::PreparedBases<Curve>        a fixed base set resident on the GPU (ark_hip_msm_bases_*): msm / msm_unchecked /
//                                        msm_bigint over it, synchronous or as ark_hip::MsmJob (asynchronous)
//   ark_hip::Radix2EvaluationDomain<F>   <- ark_poly::Radix2EvaluationDomain<F> / EvaluationDomain<F>
//        new_(num_coeffs) -> optional (None when log2(size) > TWO_ADICITY)         (poly/src/domain/radix2/mod.rs:55-83)
//        get_coset, size, log_size_of_group, size_inv, group_gen, group_gen_inv, coset_offset, coset_offset_inv,
//        coset_offset_pow_size, fft, fft_in_place, ifft, ifft_in_place             (radix2/mod.rs:85-153, domain/mod.rs:92-112)
//   ark_hip::DeviceVec<F>, ark_hip::DeviceEvaluations<F>, ark_hip::evaluate_over_domain   (round 5)
//        coefficient / evaluation vectors that stay in HBM: evaluate_over_domain -> pointwise +, -, * -> interpolate
//        (polynomial/univariate/mod.rs:305-360, evaluations/univariate/mod.rs:40-50, :104-180) with ONE upload and ONE
//        download instead of two PCIe crossings per transform
//
// Element types are plain limb arrays in the reference's in-memory layout (Montgomery, little-endian u64 limbs).
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <optional>
#include <stdexcept>
#include <utility>
#include <vector>
#include "ark_hip.h"

namespace ark_hip {

// ---- element types ------------------------------------------------------------------------------------------------
template <int WORDS>
struct FieldElement {  // Fp (WORDS = 4 or 6) or Fp2 (WORDS = 12): c0 | c1
  std::array<uint64_t, WORDS> limbs{};
  bool operator==(const FieldElement& o) const { return limbs == o.limbs; }
  bool is_zero() const {
    for (auto l : limbs)
      if (l) return false;
    return true;
  }
};
using Fr = FieldElement<4>;      // scalar-field element (Montgomery)
using BigInt4 = FieldElement<4>; // canonical 256-bit integer (PrimeField::BigInt)

template <int WORDS>
struct Affine {  // short_weierstrass::Affine with ZeroFlag = (): identity is (0, 0)
  FieldElement<WORDS> x, y;
  bool is_zero() const { return x.is_zero() && y.is_zero(); }
  bool operator==(const Affine& o) const { return x == o.x && y == o.y; }
};
template <int WORDS>
struct Projective {  // Jacobian (x, y, z)
  FieldElement<WORDS> x, y, z;
};

struct Error : std::runtime_error {
  int code;
  Error(int c, const char* what) : std::runtime_error(what), code(c) {}
};
inline void check(int rc, const char* what) {
  if (rc != 0) throw Error(rc, what);
}

// ---- curve tags -----------------------------------------------------------------------------------------------------
template <int CURVE_ID, int FE_WORDS, int SCALAR_FIELD_ID>
struct CurveTag {
  static constexpr int ID = CURVE_ID;
  static constexpr int WORDS = FE_WORDS;
  static constexpr int SCALAR_FIELD = SCALAR_FIELD_ID;
  using AffineT = Affine<FE_WORDS>;
  using ProjectiveT = Projective<FE_WORDS>;
};
using Bn254G1 = CurveTag<ARK_HIP_BN254_G1, 4, ARK_HIP_BN254_FR>;
using Bls12_381G1 = CurveTag<ARK_HIP_BLS12_381_G1, 6, ARK_HIP_BLS12_381_FR>;
using Bls12_377G1 = CurveTag<ARK_HIP_BLS12_377_G1, 6, ARK_HIP_BLS12_377_FR>;
using Bls12_377G2 = CurveTag<ARK_HIP_BLS12_377_G2, 12, ARK_HIP_BLS12_377_FR>;
using Bls12_381G2 = CurveTag<ARK_HIP_BLS12_381_G2, 12, ARK_HIP_BLS12_381_FR>;

// VariableBaseMSM<..>::msm / msm_bigint are functions of their two spans (a cached device copy of the bases is
// re-validated on every call by a hash of the span's full content: base_cache_config below).
// ResidentBases pins a base vector on the GPU for its lifetime: while it lives the caller does not modify the vector, and
// every msm / msm_bigint / msm_u* whose bases lie inside it runs against the resident copy (ark_hip_msm_bases_pin).
template <class Curve>
class ResidentBases {
 public:
  ResidentBases(const typename Curve::AffineT* bases, size_t n) : p_(bases), n_(n) {
    check(ark_hip_msm_bases_pin(Curve::ID, reinterpret_cast<const uint64_t*>(bases), n), "ark_hip_msm_bases_pin");
  }
  explicit ResidentBases(const std::vector<typename Curve::AffineT>& bases) : ResidentBases(bases.data(), bases.size()) {}
  ResidentBases(const ResidentBases&) = delete;
  ResidentBases& operator=(const ResidentBases&) = delete;
  ~ResidentBases() { (void)ark_hip_msm_bases_unpin(Curve::ID, reinterpret_cast<const uint64_t*>(p_), n_); }

 private:
  const typename Curve::AffineT* p_;
  size_t n_;
};
// The verified cache (ark_hip_msm_cache_* in ark_hip.h; on by default): base vectors passed again at the same address stay
// on the GPU, validated on every call by a hash of their full content.
struct BaseCacheStats { uint64_t entries, bytes, hits, misses, refreshed, evicted, pinned, pinned_hits; };
inline void base_cache_config(long long budget_bytes = -1, int auto_prepare_after = -1) {
  check(ark_hip_msm_cache_config(budget_bytes, auto_prepare_after), "ark_hip_msm_cache_config");
}
inline void base_cache_clear() { check(ark_hip_msm_cache_clear(), "ark_hip_msm_cache_clear"); }
inline BaseCacheStats base_cache_stats() {
  uint64_t o[8];
  check(ark_hip_msm_cache_stats(o), "ark_hip_msm_cache_stats");
  return BaseCacheStats{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]};
}

// Result<Projective, usize> of VariableBaseMSM::msm
template <class T>
struct MsmResult {
  bool ok;
  T value;         // valid when ok
  size_t min_len;  // the reference's Err payload when !ok
};

template <class Curve>
struct VariableBaseMSM {
  using A = typename Curve::AffineT;
  using P = typename Curve::ProjectiveT;
  static_assert(sizeof(A) == 2 * Curve::WORDS * 8 && sizeof(P) == 3 * Curve::WORDS * 8, "layout must be packed limbs");

  // msm: length check, then msm_unchecked (scalars are Fr elements in Montgomery form)
  static MsmResult<P> msm(const std::vector<A>& bases, const std::vector<Fr>& scalars) {
    if (bases.size() != scalars.size()) return {false, P{}, bases.size() < scalars.size() ? bases.size() : scalars.size()};
    return {true, msm_unchecked(bases, scalars), 0};
  }
  static P msm_unchecked(const std::vector<A>& bases, const std::vector<Fr>& scalars) {
    return run(bases.data(), reinterpret_cast<const uint64_t*>(scalars.data()),
               bases.size() < scalars.size() ? bases.size() : scalars.size(), 1);
  }
  static P msm_bigint(const std::vector<A>& bases, const std::vector<BigInt4>& bigints) {
    return run(bases.data(), reinterpret_cast<const uint64_t*>(bigints.data()),
               bases.size() < bigints.size() ? bases.size() : bigints.size(), 0);
  }
  // msm_chunks: Fr scalars, streams aligned at their END, steps of 2^20 pairs (0) or `step`
  static P msm_chunks(const std::vector<A>& bases, const std::vector<Fr>& scalars, size_t step = 0) {
    if (scalars.size() > bases.size()) throw Error(ARK_HIP_ERR_ARG, "scalars_stream.len() <= bases_stream.len()");
    P out;
    check(ark_hip_msm_sw_chunks(Curve::ID, reinterpret_cast<const uint64_t*>(bases.data()), bases.size(),
                                reinterpret_cast<const uint64_t*>(scalars.data()), scalars.size(), step,
                                reinterpret_cast<uint64_t*>(&out)),
          "ark_hip_msm_sw_chunks");
    return out;
  }
  // Projective: Sum (group.rs:659-663)
  static P sum(const std::vector<P>& pts) {
    P out;
    check(ark_hip_sw_sum(Curve::ID, reinterpret_cast<const uint64_t*>(pts.data()), pts.size(),
                         reinterpret_cast<uint64_t*>(&out)),
          "ark_hip_sw_sum");
    return out;
  }
  // CurveGroup::into_affine
  static A into_affine(const P& p) {
    A out;
    check(ark_hip_sw_into_affine(Curve::ID, reinterpret_cast<const uint64_t*>(&p), 1, reinterpret_cast<uint64_t*>(&out)),
          "ark_hip_sw_into_affine");
    return out;
  }

 private:
  static P run(const A* bases, const uint64_t* scalars, size_t n, int montgomery) {
    P out;
    check(ark_hip_msm_sw(Curve::ID, reinterpret_cast<const uint64_t*>(bases), scalars, n, montgomery,
                         reinterpret_cast<uint64_t*>(&out)),
          "ark_hip_msm_sw");
    return out;
  }
};

// ---- base-set validation (ark_hip_sw_check / ark_hip_sw_check_device) ------------------------------------------------
// What establishes the precondition of every MSM entry above: coordinates are field elements, points are on the curve
// (Affine::is_on_curve) and, with subgroup = true, in the prime-order subgroup
// (SWCurveConfig::is_in_correct_subgroup_assuming_on_curve).  Nothing validates by default: these calls do.
struct BaseCheck {
  bool ok;               // every point passed
  uint64_t first_bad;    // smallest index with a non-zero status (n if none)
  uint64_t not_reduced, off_curve, off_subgroup;   // points with status 1, 2, 3
  std::vector<uint8_t> status;                     // per point, when asked for (host form)
};
enum class CheckMethod : int { Auto = 0, Ladder = 1, Endomorphism = 2 };
template <class Curve>
inline BaseCheck check_bases(const typename Curve::AffineT* bases, size_t n, bool subgroup = true,
                             CheckMethod method = CheckMethod::Auto, bool return_status = false) {
  BaseCheck r{};
  if (return_status) r.status.assign(n, 0);
  uint64_t out[4];
  check(ark_hip_sw_check(Curve::ID, reinterpret_cast<const uint64_t*>(bases), n, subgroup ? 3 : 1, static_cast<int>(method),
                         return_status ? r.status.data() : nullptr, out),
        "ark_hip_sw_check");
  r.first_bad = out[0], r.not_reduced = out[1], r.off_curve = out[2], r.off_subgroup = out[3];
  r.ok = out[1] + out[2] + out[3] == 0;
  return r;
}
template <class Curve>
inline BaseCheck check_bases(const std::vector<typename Curve::AffineT>& bases, bool subgroup = true,
                             CheckMethod method = CheckMethod::Auto, bool return_status = false) {
  return check_bases<Curve>(bases.data(), bases.size(), subgroup, method, return_status);
}
// the same for n Affine points in device memory; d_status: n bytes of device memory, or nullptr
template <class Curve>
inline BaseCheck check_bases_device(const void* d_bases, size_t n, bool subgroup = true, CheckMethod method = CheckMethod::Auto,
                                    void* d_status = nullptr) {
  BaseCheck r{};
  uint64_t out[4];
  check(ark_hip_sw_check_device(Curve::ID, d_bases, n, subgroup ? 3 : 1, static_cast<int>(method), d_status, out),
        "ark_hip_sw_check_device");
  r.first_bad = out[0], r.not_reduced = out[1], r.off_curve = out[2], r.off_subgroup = out[3];
  r.ok = out[1] + out[2] + out[3] == 0;
  return r;
}

// ---- compressed points (ark_hip_sw_decompress* / ark_hip_sw_compress*) ------------------------------------------------
// Affine::deserialize_with_mode(.., Compress::Yes, ..) over n encodings of compressed_size<Curve>() bytes each, and its inverse.
struct BaseDecode {
  bool ok;               // every encoding was accepted
  uint64_t first_bad;    // smallest index with a non-zero status (n if none)
  uint64_t bad_flags, not_reduced, no_root, off_subgroup;   // encodings with status 1, 2, 3, 4
  std::vector<uint8_t> status;                               // per encoding, when asked for (host form)
};
template <class Curve>
inline size_t compressed_size() {
  return static_cast<size_t>(ark_hip_sw_compressed_size(Curve::ID));
}
namespace detail {
inline BaseDecode base_decode(const uint64_t out[5], std::vector<uint8_t> status = {}) {
  BaseDecode r{};
  r.first_bad = out[0], r.bad_flags = out[1], r.not_reduced = out[2], r.no_root = out[3], r.off_subgroup = out[4];
  r.ok = out[1] + out[2] + out[3] + out[4] == 0;
  r.status = std::move(status);
  return r;
}
}  // namespace detail
// n encodings in host memory -> n Affine points in `points` (a refused encoding gives the identity)
template <class Curve>
inline BaseDecode decompress_bases(const uint8_t* bytes, size_t n, std::vector<typename Curve::AffineT>& points, bool validate = true,
                                   CheckMethod method = CheckMethod::Auto, bool return_status = false) {
  points.resize(n);
  std::vector<uint8_t> status(return_status ? n : 0);
  uint64_t out[5];
  check(ark_hip_sw_decompress(Curve::ID, bytes, n, validate ? 1 : 0, static_cast<int>(method), reinterpret_cast<uint64_t*>(points.data()),
                              return_status ? status.data() : nullptr, out),
        "ark_hip_sw_decompress");
  return detail::base_decode(out, std::move(status));
}
// the same in device memory; d_status: n bytes of device memory, or nullptr
template <class Curve>
inline BaseDecode decompress_bases_device(const void* d_bytes, size_t n, void* d_points, bool validate = true,
                                          CheckMethod method = CheckMethod::Auto, void* d_status = nullptr) {
  uint64_t out[5];
  check(ark_hip_sw_decompress_device(Curve::ID, d_bytes, n, validate ? 1 : 0, static_cast<int>(method), d_points, d_status, out),
        "ark_hip_sw_decompress_device");
  return detail::base_decode(out);
}
// the canonical encodings of n points whose coordinates are reduced (what check_bases establishes)
template <class Curve>
inline std::vector<uint8_t> compress_bases(const typename Curve::AffineT* bases, size_t n) {
  std::vector<uint8_t> bytes(n * compressed_size<Curve>());
  check(ark_hip_sw_compress(Curve::ID, reinterpret_cast<const uint64_t*>(bases), n, bytes.data()), "ark_hip_sw_compress");
  return bytes;
}
template <class Curve>
inline std::vector<uint8_t> compress_bases(const std::vector<typename Curve::AffineT>& bases) {
  return compress_bases<Curve>(bases.data(), bases.size());
}
// device memory to device memory, asynchronous on the context stream
template <class Curve>
inline void compress_bases_device(const void* d_bases, size_t n, void* d_bytes) {
  check(ark_hip_sw_compress_device(Curve::ID, d_bases, n, d_bytes), "ark_hip_sw_compress_device");
}

// ---- an MSM in flight (ark_hip_msm_job) -------------------------------------------------------------------------------
template <class Curve>
class MsmJob {
 public:
  using P = typename Curve::ProjectiveT;
  explicit MsmJob(ark_hip_msm_job* j) : j_(j) {}
  MsmJob(MsmJob&& o) noexcept : j_(o.j_) { o.j_ = nullptr; }
  MsmJob(const MsmJob&) = delete;
  ~MsmJob() {
    if (j_) (void)ark_hip_msm_wait(j_, nullptr);  // never leak a device job slot
  }
  P wait() {
    P out;
    ark_hip_msm_job* j = j_;
    j_ = nullptr;
    check(ark_hip_msm_wait(j, reinterpret_cast<uint64_t*>(&out)), "ark_hip_msm_wait");
    return out;
  }

 private:
  ark_hip_msm_job* j_;
};

// ---- a fixed base set (SRS) resident on the GPU with its per-window multiples -----------------------------------------
template <class Curve>
class PreparedBases {
 public:
  using A = typename Curve::AffineT;
  using P = typename Curve::ProjectiveT;
  explicit PreparedBases(const std::vector<A>& bases) : n_(bases.size()) {
    check(ark_hip_msm_bases_prepare(Curve::ID, reinterpret_cast<const uint64_t*>(bases.data()), bases.size(), &h_),
          "ark_hip_msm_bases_prepare");
  }
  PreparedBases(const PreparedBases&) = delete;
  ~PreparedBases() { (void)ark_hip_msm_bases_free(h_); }
  size_t size() const { return n_; }
  MsmResult<P> msm(const std::vector<Fr>& scalars) const {
    if (scalars.size() != n_) return {false, P{}, scalars.size() < n_ ? scalars.size() : n_};
    return {true, run(reinterpret_cast<const uint64_t*>(scalars.data()), n_, 1), 0};
  }
  P msm_unchecked(const std::vector<Fr>& scalars) const {
    return run(reinterpret_cast<const uint64_t*>(scalars.data()), scalars.size() < n_ ? scalars.size() : n_, 1);
  }
  P msm_bigint(const std::vector<BigInt4>& bigints) const {
    return run(reinterpret_cast<const uint64_t*>(bigints.data()), bigints.size() < n_ ? bigints.size() : n_, 0);
  }
  // the scalars must outlive the job
  MsmJob<Curve> msm_bigint_async(const std::vector<BigInt4>& bigints) const {
    ark_hip_msm_job* j = nullptr;
    check(ark_hip_msm_prepared_async(h_, reinterpret_cast<const uint64_t*>(bigints.data()),
                                     bigints.size() < n_ ? bigints.size() : n_, 0, &j),
          "ark_hip_msm_prepared_async");
    return MsmJob<Curve>(j);
  }

 private:
  P run(const uint64_t* scalars, size_t n, int montgomery) const {
    P out;
    check(ark_hip_msm_prepared(h_, scalars, n, montgomery, reinterpret_cast<uint64_t*>(&out)), "ark_hip_msm_prepared");
    return out;
  }
  ark_hip_msm_bases* h_ = nullptr;
  size_t n_;
};

// ---- streaming accumulators (stream_pippenger.rs) ---------------------------------------------------------------------
template <class Curve>
class ChunkedPippenger {  // stream_pippenger.rs:10-66
 public:
  using A = typename Curve::AffineT;
  using P = typename Curve::ProjectiveT;
  explicit ChunkedPippenger(size_t max_msm_buffer) : buf_size_(max_msm_buffer) {
    bases_.reserve(max_msm_buffer);
    scalars_.reserve(max_msm_buffer);
  }
  static ChunkedPippenger with_size(size_t buf_size) { return ChunkedPippenger(buf_size); }
  void add(const A& base, const BigInt4& scalar) {
    bases_.push_back(base);
    scalars_.push_back(scalar);
    if (scalars_.size() == buf_size_) flush();
  }
  P finalize() {
    if (!scalars_.empty()) flush();
    return VariableBaseMSM<Curve>::sum(partials_);  // empty -> identity
  }

 private:
  void flush() {
    partials_.push_back(VariableBaseMSM<Curve>::msm_bigint(bases_, scalars_));
    bases_.clear();
    scalars_.clear();
  }
  size_t buf_size_;
  std::vector<A> bases_;
  std::vector<BigInt4> scalars_;
  std::vector<P> partials_;
};

// HashMapPippenger (stream_pippenger.rs:68-128): scalars of equal bases are added in Fr before the MSM.  The modular
// addition is supplied by the host (`AddFr`: Fr x Fr -> Fr on Montgomery residues), as the reference uses its own
// field type; a flush runs one MSM over the distinct bases with the Fr -> BigInt conversion on the device.
template <class Curve, class AddFr>
class HashMapPippenger {
 public:
  using A = typename Curve::AffineT;
  using P = typename Curve::ProjectiveT;
  HashMapPippenger(size_t max_msm_buffer, AddFr add) : buf_size_(max_msm_buffer), add_(std::move(add)) {}
  void add(const A& base, const Fr& scalar) {
    Key k;
    std::memcpy(k.data(), &base, sizeof(A));
    auto it = map_.find(k);
    if (it == map_.end()) map_.emplace(k, scalar);
    else it->second = add_(it->second, scalar);
    if (map_.size() == buf_size_) flush();
  }
  P finalize() {
    if (!map_.empty()) flush();
    return VariableBaseMSM<Curve>::sum(partials_);
  }

 private:
  using Key = std::array<unsigned char, sizeof(A)>;
  void flush() {
    std::vector<A> bases;
    std::vector<Fr> scalars;
    for (auto& kv : map_) {
      A a;
      std::memcpy(&a, kv.first.data(), sizeof(A));
      bases.push_back(a);
      scalars.push_back(kv.second);
    }
    partials_.push_back(VariableBaseMSM<Curve>::msm_unchecked(bases, scalars));
    map_.clear();
  }
  size_t buf_size_;
  AddFr add_;
  std::map<Key, Fr> map_;
  std::vector<P> partials_;
};

// ---- one process per GPU: the library's RCCL communicator ------------------------------------------------------------
// Rank 0 creates the id, the host ships its bytes to the other ranks (MPI_Bcast, a socket ...), every rank constructs a
// Communicator on its device (collective).  While it lives, msm_sharded / fft_sharded_in_place_device are collective
// calls; the reference's counterpart of the split is its own chunking by base range (variable_base/mod.rs:521-557).
class Communicator {
 public:
  using Id = std::array<unsigned char, ARK_HIP_COMM_ID_BYTES>;
  static Id unique_id() {
    Id id{};
    check(ark_hip_comm_unique_id(id.data()), "ark_hip_comm_unique_id");
    return id;
  }
  Communicator(const Id& id, int rank, int world) { check(ark_hip_comm_init(id.data(), rank, world), "ark_hip_comm_init"); }
  ~Communicator() { (void)ark_hip_comm_destroy(); }
  Communicator(const Communicator&) = delete;
  Communicator& operator=(const Communicator&) = delete;
  int rank() const { int r = 0, w = 1; check(ark_hip_comm_info(&r, &w), "ark_hip_comm_info"); return r; }
  int world() const { int r = 0, w = 1; check(ark_hip_comm_info(&r, &w), "ark_hip_comm_info"); return w; }
  // the sum over ALL ranks' (base, scalar) shards; d_bases / d_scalars: this rank's shard in device memory
  template <class Curve>
  typename Curve::ProjectiveT msm_bigint_sharded(const void* d_bases, const void* d_scalars, size_t n_local) const {
    typename Curve::ProjectiveT out;
    check(ark_hip_msm_sw_device_sharded(Curve::ID, d_bases, d_scalars, n_local, 0, reinterpret_cast<uint64_t*>(&out)),
          "ark_hip_msm_sw_device_sharded");
    return out;
  }
};

// ---- Radix2EvaluationDomain ------------------------------------------------------------------------------------------
template <int FIELD_ID>
class DeviceVec;
template <int FIELD_ID>
class Radix2EvaluationDomain {
 public:
  // EvaluationDomain::new
  static std::optional<Radix2EvaluationDomain> new_(size_t num_coeffs) {
    Radix2EvaluationDomain d;
    int rc = ark_hip_radix2_domain_new(FIELD_ID, num_coeffs, &d.s_);
    if (rc == ARK_HIP_ERR_SIZE) return std::nullopt;
    check(rc, "ark_hip_radix2_domain_new");
    return d;
  }
  std::optional<Radix2EvaluationDomain> get_coset(const Fr& offset) const {
    Radix2EvaluationDomain d;
    int rc = ark_hip_radix2_domain_get_coset(FIELD_ID, &s_, offset.limbs.data(), &d.s_);
    if (rc == ARK_HIP_ERR_ARG) return std::nullopt;
    check(rc, "ark_hip_radix2_domain_get_coset");
    return d;
  }
  static std::optional<size_t> compute_size_of_domain(size_t num_coeffs) {
    auto d = new_(num_coeffs);
    if (!d) return std::nullopt;
    return d->size();
  }
  size_t size() const { return (size_t)s_.size; }
  uint64_t log_size_of_group() const { return s_.log_size_of_group; }
  Fr size_as_field_element() const { return fe(s_.size_as_field_element); }
  Fr size_inv() const { return fe(s_.size_inv); }
  Fr group_gen() const { return fe(s_.group_gen); }
  Fr group_gen_inv() const { return fe(s_.group_gen_inv); }
  Fr coset_offset() const { return fe(s_.offset); }
  Fr coset_offset_inv() const { return fe(s_.offset_inv); }
  Fr coset_offset_pow_size() const { return fe(s_.offset_pow_size); }

  // fft_in_place / ifft_in_place: the Vec is resized to the domain size (zero-extended) first, as in radix2/mod.rs:140-153
  // (a vector of at most size/4 coefficients takes the degree-aware path, radix2/mod.rs:141: only the coefficients
  // are uploaded and the leading butterfly stages are skipped)
  void fft_in_place(std::vector<Fr>& coeffs) const {
    const size_t len = coeffs.size();
    resize(coeffs);
    check(ark_hip_fft_in_place_degree_aware(FIELD_ID, &s_, reinterpret_cast<uint64_t*>(coeffs.data()), len),
          "ark_hip_fft_in_place_degree_aware");
  }
  void ifft_in_place(std::vector<Fr>& evals) const {
    resize(evals);
    check(ark_hip_ifft_in_place(FIELD_ID, &s_, reinterpret_cast<uint64_t*>(evals.data())), "ark_hip_ifft_in_place");
  }
  std::vector<Fr> fft(const std::vector<Fr>& coeffs) const {
    std::vector<Fr> v(coeffs);
    fft_in_place(v);
    return v;
  }
  std::vector<Fr> ifft(const std::vector<Fr>& evals) const {
    std::vector<Fr> v(evals);
    ifft_in_place(v);
    return v;
  }
  // Several polynomials over this domain at once, each size() elements in THIS GPU's memory, transformed in place with up
  // to three transforms in flight (no counterpart in the reference: its callers loop over fft_in_place).  Asynchronous:
  // ark_hip_synchronize() before the results are read.
  void fft_batch_in_place_device(const std::vector<void*>& d_polys, bool inverse = false) const {
    check(ark_hip_fft_batch_in_place_device(FIELD_ID, &s_, d_polys.data(), d_polys.size(), inverse ? 1 : 0),
          "ark_hip_fft_batch_in_place_device");
  }
  // One process per GPU (Communicator below): this rank's m = size() / world elements, in THIS GPU's memory, of ONE
  // transform over all ranks -- forward: d_local[i2] = x[rank + world i2] in, d_local[j1 sub + t] = X[j1 m + rank sub + t]
  // out (sub = m / world); inverse: the other way round.  One all-to-all over RCCL inside the library.  Collective;
  // asynchronous on the device (ark_hip_synchronize() before the results are read).
  void fft_sharded_in_place_device(void* d_local, bool inverse = false) const {
    check(ark_hip_fft_sharded_device(FIELD_ID, &s_, d_local, inverse ? 1 : 0), "ark_hip_fft_sharded_device");
  }
  // fft_in_place / ifft_in_place for T = Projective<P> (poly/src/domain/mod.rs:332-362; poly/src/test.rs:57): points of a
  // curve whose scalar field is this domain's; resized to the domain size with identities (z = 0) first
  template <class Curve>
  void fft_group_in_place(std::vector<typename Curve::ProjectiveT>& pts, bool inverse = false) const {
    static_assert(Curve::SCALAR_FIELD == FIELD_ID, "the domain must be over the curve's scalar field");
    if (pts.size() > size()) throw Error(ARK_HIP_ERR_ARG, "more coefficients than the domain size");
    typename Curve::ProjectiveT zero{};   // all-zero limbs: z = 0, the identity the transform expects
    pts.resize(size(), zero);
    check(ark_hip_fft_group_in_place(Curve::ID, &s_, reinterpret_cast<uint64_t*>(pts.data()), inverse ? 1 : 0),
          "ark_hip_fft_group_in_place");
  }
  // evaluate_vanishing_polynomial (poly/src/domain/mod.rs:231-239) is host arithmetic of the caller's field type; what the
  // device offers is evaluate_all_lagrange_coefficients (domain/mod.rs:157-222): L_i(tau) for the size() points h g^i, as a
  // device vector -- with DeviceVec::inner_product and the evaluations of P over this domain that is P(tau).  Asynchronous.
  DeviceVec<FIELD_ID> evaluate_all_lagrange_coefficients(const Fr& tau) const;
  const ark_hip_radix2_domain& raw() const { return s_; }

 private:
  ark_hip_radix2_domain s_{};
  static Fr fe(const uint64_t* p) {
    Fr r;
    for (int i = 0; i < 4; i++) r.limbs[i] = p[i];
    return r;
  }
  void resize(std::vector<Fr>& v) const {
    if (v.size() > size()) throw Error(ARK_HIP_ERR_ARG, "more coefficients than the domain size");
    v.resize(size());
  }
};

// ---- device-resident vectors of Fr: DensePolynomial coefficients / Evaluations that stay in HBM -----------------------
// The reference's callers chain transforms: DensePolynomial::evaluate_over_domain (polynomial/univariate/mod.rs:305-360:
// zero-extend + fft_in_place -> Evaluations), the pointwise +, -, * of Evaluations over one domain
// (evaluations/univariate/mod.rs:104-180) and Evaluations::interpolate (mod.rs:40-50: ifft_in_place -> coefficients).
// Through the host-pointer entries every link of such a chain crosses PCIe twice (2 x 128 MiB at 2^22: 5.3 ms around a
// 0.5 ms transform).  DeviceVec owns ark_hip_malloc memory; the chain below costs ONE upload and ONE download.
// All operations are asynchronous on the library's stream of the current device and ordered with each other; to_vec()
// waits.  A DeviceVec belongs to the device that was current when it was made.
template <int FIELD_ID>
class DeviceVec {
 public:
  DeviceVec() = default;
  explicit DeviceVec(size_t len) { alloc(len); zero_from(0); }                       // vec![F::zero(); len]
  static DeviceVec from_slice(const Fr* x, size_t len) {
    DeviceVec v;
    v.alloc(len);
    check(ark_hip_memcpy_h2d(v.p_, x, len * 32), "ark_hip_memcpy_h2d");
    return v;
  }
  static DeviceVec from_vec(const std::vector<Fr>& x) { return from_slice(x.data(), x.size()); }
  DeviceVec(DeviceVec&& o) noexcept : p_(o.p_), len_(o.len_), cap_(o.cap_), dev_(o.dev_), view_(o.view_) { o.p_ = nullptr; o.len_ = o.cap_ = 0; }
  DeviceVec& operator=(DeviceVec&& o) noexcept {
    if (this != &o) { release(); p_ = o.p_; len_ = o.len_; cap_ = o.cap_; dev_ = o.dev_; view_ = o.view_; o.p_ = nullptr; o.len_ = o.cap_ = 0; }
    return *this;
  }
  // len elements from element offset of `owner` on: a VIEW, no copy -- it frees nothing and must not outlive or outgrow its
  // owner (the halves of a product tree's level as the evaluations of a DenseMultilinearExtension)
  static DeviceVec view(const DeviceVec& owner, size_t offset, size_t len) {
    owner.here();
    if (offset > owner.len_ || len > owner.len_ - offset) throw Error(ARK_HIP_ERR_ARG, "the view leaves its owner");
    DeviceVec v;
    v.p_ = len ? (char*)owner.p_ + 32 * offset : nullptr;
    v.len_ = v.cap_ = len;
    v.dev_ = owner.dev_;
    v.view_ = true;
    return v;
  }
  bool is_view() const { return view_; }
  DeviceVec(const DeviceVec&) = delete;
  DeviceVec& operator=(const DeviceVec&) = delete;
  ~DeviceVec() { release(); }
  DeviceVec clone() const {
    here();
    DeviceVec v;
    v.alloc(len_);
    check(ark_hip_memcpy_d2d(v.p_, p_, len_ * 32), "ark_hip_memcpy_d2d");
    return v;
  }
  std::vector<Fr> to_vec() const {
    here();
    std::vector<Fr> out(len_);
    check(ark_hip_memcpy_d2h(out.data(), p_, len_ * 32), "ark_hip_memcpy_d2h");
    return out;
  }
  size_t len() const { return len_; }
  bool is_empty() const { return len_ == 0; }
  void* device_ptr() { return p_; }
  const void* device_ptr() const { return p_; }
  // Vec::resize(new_len, F::zero()) / Vec::truncate
  void resize_zeroed(size_t new_len) {
    here();
    if (new_len > cap_) {
      DeviceVec v;
      v.alloc(new_len);
      check(ark_hip_memcpy_d2d(v.p_, p_, len_ * 32), "ark_hip_memcpy_d2d");
      const size_t keep = len_;
      *this = std::move(v);
      len_ = keep;
    }
    const size_t old = len_;
    len_ = new_len;
    if (new_len > old) zero_from(old);
  }
  // pointwise: self = self (op) other, element by element (lengths must agree, as Evaluations over one domain do)
  DeviceVec& operator+=(const DeviceVec& o) { same(o); check(ark_hip_fr_add_device(FIELD_ID, p_, o.p_, p_, len_), "ark_hip_fr_add_device"); return *this; }
  DeviceVec& operator-=(const DeviceVec& o) { same(o); check(ark_hip_fr_sub_device(FIELD_ID, p_, o.p_, p_, len_), "ark_hip_fr_sub_device"); return *this; }
  DeviceVec& operator*=(const DeviceVec& o) { same(o); check(ark_hip_fr_mul_device(FIELD_ID, p_, o.p_, p_, len_), "ark_hip_fr_mul_device"); return *this; }
  DeviceVec& operator/=(const DeviceVec& o) { same(o); check(ark_hip_fr_div_device(FIELD_ID, p_, o.p_, p_, len_), "ark_hip_fr_div_device"); return *this; }
  void batch_inverse() { here(); check(ark_hip_fr_inverse_device(FIELD_ID, p_, p_, len_), "ark_hip_fr_inverse_device"); }   // zeros stay zero
  DeviceVec& operator*=(const Fr& k) { here(); check(ark_hip_fr_scale_device(FIELD_ID, p_, k.limbs.data(), p_, len_), "ark_hip_fr_scale_device"); return *this; }
  void negate() { here(); check(ark_hip_fr_neg_device(FIELD_ID, p_, p_, len_), "ark_hip_fr_neg_device"); }

  // ---- the O(n) steps between the transforms and the MSM, without leaving the device ----
  // len elements of device memory whose content is whatever the allocator left (for results written in full)
  static DeviceVec uninit(size_t len) { DeviceVec v; v.alloc(len); return v; }
  // DensePolynomial::evaluate (dense.rs:42-92); waits for its result
  Fr evaluate(const Fr& point) const {
    here();
    Fr out;
    check(ark_hip_poly_evaluate_device(FIELD_ID, p_, len_, point.limbs.data(), out.limbs.data()), "ark_hip_poly_evaluate_device");
    return out;
  }
  // (quotient, remainder) of the division by x - z (divide_with_q_and_r for a degree-1 divisor, univariate/mod.rs:145-159);
  // the quotient has max(len, 1) - 1 coefficients, the remainder is p(z)
  std::pair<DeviceVec, Fr> divide_by_linear(const Fr& z) const {
    here();
    DeviceVec q = uninit(len_ ? len_ - 1 : 0);
    Fr rem;
    check(ark_hip_poly_divide_linear_device(FIELD_ID, p_, len_, z.limbs.data(), q.p_, rem.limbs.data()), "ark_hip_poly_divide_linear_device");
    return {std::move(q), rem};
  }
  // the same with the quotient written over this vector, which becomes one element shorter; returns the remainder
  Fr divide_by_linear_in_place(const Fr& z) {
    here();
    Fr rem;
    check(ark_hip_poly_divide_linear_device(FIELD_ID, p_, len_, z.limbs.data(), p_, rem.limbs.data()), "ark_hip_poly_divide_linear_device");
    if (len_) len_--;
    return rem;
  }
  // DensePolynomial::divide_by_vanishing_poly (dense.rs:168-211): (quotient, remainder); only the domain's size enters
  std::pair<DeviceVec, DeviceVec> divide_by_vanishing_poly(const Radix2EvaluationDomain<FIELD_ID>& domain) const {
    here();
    const size_t m = domain.size();
    DeviceVec q = uninit(len_ > m ? len_ - m : 0), r = uninit(len_ < m ? len_ : m);
    check(ark_hip_poly_divide_by_vanishing_device(FIELD_ID, m, p_, len_, q.p_, r.p_), "ark_hip_poly_divide_by_vanishing_device");
    return {std::move(q), std::move(r)};
  }
  // sum_i self[i] * other[i]; waits for its result
  Fr inner_product(const DeviceVec& o) const {
    same(o);
    Fr out;
    check(ark_hip_fr_inner_product_device(FIELD_ID, p_, o.p_, len_, out.limbs.data()), "ark_hip_fr_inner_product_device");
    return out;
  }
  // ---- running products and sums: the accumulator column of a univariate prover ----
  // (vector, total): out[i] = prod_{j <= i} self[j] (exclusive: j < i, out[0] = 1) and the product of everything; waits for it
  std::pair<DeviceVec, Fr> prefix_product(bool exclusive = false) const {
    here();
    DeviceVec out = uninit(len_);
    Fr total;
    check(ark_hip_fr_prefix_product_device(FIELD_ID, p_, len_, exclusive ? 1 : 0, out.p_, total.limbs.data()), "ark_hip_fr_prefix_product_device");
    return {std::move(out), total};
  }
  // (vector, total): out[i] = sum_{j <= i} self[j] (exclusive: j < i, out[0] = 0) and the sum of everything; waits for it
  std::pair<DeviceVec, Fr> prefix_sum(bool exclusive = false) const {
    here();
    DeviceVec out = uninit(len_);
    Fr total;
    check(ark_hip_fr_prefix_sum_device(FIELD_ID, p_, len_, exclusive ? 1 : 0, out.p_, total.limbs.data()), "ark_hip_fr_prefix_sum_device");
    return {std::move(out), total};
  }
  // (z, last) with self the numerators: z[0] = 1, z[i+1] = z[i] self[i] / den[i] and last = prod_j self[j] / den[j], the value
  // that is one for a valid permutation; waits for it.  From the first zero denominator on the outputs are zero (operator/=).
  std::pair<DeviceVec, Fr> prefix_ratio(const DeviceVec& den) const {
    same(den);
    DeviceVec out = uninit(len_);
    Fr last;
    check(ark_hip_fr_prefix_ratio_device(FIELD_ID, p_, den.p_, len_, out.p_, last.limbs.data()), "ark_hip_fr_prefix_ratio_device");
    return {std::move(out), last};
  }
  // ---- the rotated copy: the one-term case of a gate expression (SumOfProducts below) ----
  // out[i] = self[(i + k) mod len], k any int64_t: one unit term of one factor, a product-free copy
  DeviceVec rotate(int64_t k) const {
    DeviceVec out = uninit(len_);
    rotate(k, out);
    return out;
  }
  // the same into `out` (not this vector unless k is 0 mod len)
  void rotate(int64_t k, DeviceVec& out) const {
    same(out);
    if (!len_) return;
    Fr one, any{};
    check(ark_hip_fr_pow(FIELD_ID, any.limbs.data(), 0, one.limbs.data()), "ark_hip_fr_pow");
    const void* col = p_;
    const unsigned len = 1, idx = 0;
    check(ark_hip_fr_sum_of_products_device(FIELD_ID, &col, 1, len_, &len, &idx, &k, one.limbs.data(), 1, nullptr, out.p_),
          "ark_hip_fr_sum_of_products_device");
  }

 private:
  void* p_ = nullptr;
  size_t len_ = 0, cap_ = 0;
  int dev_ = -1;
  bool view_ = false;
  void alloc(size_t len) {
    dev_ = ark_hip_get_device();
    len_ = cap_ = len;
    if (len) check(ark_hip_malloc(len * 32, &p_), "ark_hip_malloc");
  }
  void zero_from(size_t from) {
    if (len_ > from) check(ark_hip_memset_device((char*)p_ + from * 32, 0, (len_ - from) * 32), "ark_hip_memset_device");
  }
  // every operation runs on the stream of the thread's CURRENT device: refuse a vector that lives elsewhere
  void here() const {
    if (p_ && ark_hip_get_device() != dev_) throw Error(ARK_HIP_ERR_ARG, "the device vector lives on another device than the current one");
  }
  void same(const DeviceVec& o) const {
    here();
    o.here();
    if (o.len_ != len_) throw Error(ARK_HIP_ERR_ARG, "domains are unequal");   // the reference's assert_eq!(self.domain, other.domain)
  }
  void release() {
    if (!p_) return;
    if (view_) { p_ = nullptr; return; }   // a view owns nothing
    const int cur = ark_hip_get_device();
    if (dev_ >= 0 && cur != dev_) (void)ark_hip_set_device(dev_);   // freed on the device that owns it
    (void)ark_hip_free(p_);
    if (dev_ >= 0 && cur != dev_ && cur >= 0) (void)ark_hip_set_device(cur);
    p_ = nullptr;
  }
};

template <int FIELD_ID>
DeviceVec<FIELD_ID> Radix2EvaluationDomain<FIELD_ID>::evaluate_all_lagrange_coefficients(const Fr& tau) const {
  DeviceVec<FIELD_ID> out = DeviceVec<FIELD_ID>::uninit(size());
  check(ark_hip_domain_lagrange_coefficients_device(FIELD_ID, &s_, tau.limbs.data(), out.device_ptr()),
        "ark_hip_domain_lagrange_coefficients_device");
  return out;
}

// Evaluations<F, Radix2EvaluationDomain<F>> resident on the device (evaluations/univariate/mod.rs:18-29)
template <int FIELD_ID>
struct DeviceEvaluations {
  DeviceVec<FIELD_ID> evals;
  Radix2EvaluationDomain<FIELD_ID> domain;
  // Evaluations::interpolate (mod.rs:47-50): the coefficients, still on the device (size() of them; the reference's
  // from_coefficients_vec drops leading zeros on the host -- do that after to_vec() if a DensePolynomial is wanted)
  DeviceVec<FIELD_ID> interpolate() && {
    check(ark_hip_ifft_in_place_device(FIELD_ID, &domain.raw(), evals.device_ptr()), "ark_hip_ifft_in_place_device");
    return std::move(evals);
  }
  DeviceEvaluations& operator+=(const DeviceEvaluations& o) { evals += o.evals; return *this; }
  DeviceEvaluations& operator-=(const DeviceEvaluations& o) { evals -= o.evals; return *this; }
  DeviceEvaluations& operator*=(const DeviceEvaluations& o) { evals *= o.evals; return *this; }
  DeviceEvaluations& operator/=(const DeviceEvaluations& o) { evals /= o.evals; return *this; }
};
// DensePolynomial::evaluate_over_domain (polynomial/univariate/mod.rs:305-360) for coefficients already on the device:
// zero-extension and transform in place; at most size/4 coefficients take the degree-aware path (radix2/mod.rs:141).
// More coefficients than the domain holds is the reference's folding case (mod.rs:330-352): not served here.
template <int FIELD_ID>
DeviceEvaluations<FIELD_ID> evaluate_over_domain(DeviceVec<FIELD_ID>&& coeffs, const Radix2EvaluationDomain<FIELD_ID>& domain) {
  const size_t have = coeffs.len();
  if (have > domain.size()) throw Error(ARK_HIP_ERR_ARG, "more coefficients than the domain size");
  coeffs.resize_zeroed(domain.size());
  check(ark_hip_fft_in_place_degree_aware_device(FIELD_ID, &domain.raw(), coeffs.device_ptr(), have),
        "ark_hip_fft_in_place_degree_aware_device");
  return DeviceEvaluations<FIELD_ID>{std::move(coeffs), domain};
}

// A rows x cols matrix over Fr in CSR form, resident on the device: the constraint matrices of an R1CS /
// CCS instance.  Built once per circuit from host arrays, which are validated there and copied; with_transpose also keeps
// M^T (stable order), which mul_t needs.  Products are asynchronous on the library's stream; bilinear waits.
struct CsrPlan { int tile, max_rows; size_t blocks, long_rows, long_chunks; };
// how a handle with these row_ptr (rows + 1 entries) is cut into work; host only
inline CsrPlan csr_plan(size_t rows, const uint32_t* row_ptr) {
  CsrPlan p{};
  check(ark_hip_csr_plan(rows, row_ptr, &p.tile, &p.max_rows, &p.blocks, &p.long_rows, &p.long_chunks), "ark_hip_csr_plan");
  return p;
}
template <int FIELD_ID>
class CsrMatrix {
 public:
  CsrMatrix(size_t rows, size_t cols, const uint32_t* row_ptr, const uint32_t* col_idx, const Fr* vals, size_t nnz,
            bool with_transpose = false)
      : rows_(rows), cols_(cols), nnz_(nnz), has_t_(with_transpose) {
    check(ark_hip_fr_csr_create(FIELD_ID, rows, cols, row_ptr, col_idx, nnz ? vals->limbs.data() : nullptr, nnz,
                                with_transpose ? ARK_HIP_CSR_WITH_TRANSPOSE : 0u, &h_), "ark_hip_fr_csr_create");
  }
  CsrMatrix(size_t rows, size_t cols, const std::vector<uint32_t>& row_ptr, const std::vector<uint32_t>& col_idx,
            const std::vector<Fr>& vals, bool with_transpose = false)
      : CsrMatrix(rows, cols, row_ptr.data(), col_idx.data(), vals.data(), vals.size(), with_transpose) {
    if (row_ptr.size() != rows + 1 || col_idx.size() != vals.size()) { free(); throw Error(ARK_HIP_ERR_ARG, "row_ptr: rows + 1 entries; one value per column index"); }
  }
  CsrMatrix(CsrMatrix&& o) noexcept : h_(o.h_), rows_(o.rows_), cols_(o.cols_), nnz_(o.nnz_), has_t_(o.has_t_) { o.h_ = nullptr; }
  CsrMatrix(const CsrMatrix&) = delete;
  CsrMatrix& operator=(const CsrMatrix&) = delete;
  ~CsrMatrix() { free(); }
  void free() {
    if (h_) (void)ark_hip_fr_csr_free(h_);
    h_ = nullptr;
  }
  size_t rows() const { return rows_; }
  size_t cols() const { return cols_; }
  size_t nnz() const { return nnz_; }
  bool has_transpose() const { return has_t_; }
  // y = M x: x has cols elements, y rows
  DeviceVec<FIELD_ID> mul(const DeviceVec<FIELD_ID>& x) const {
    DeviceVec<FIELD_ID> y = DeviceVec<FIELD_ID>::uninit(rows_);
    mul(x, y);
    return y;
  }
  void mul(const DeviceVec<FIELD_ID>& x, DeviceVec<FIELD_ID>& out) const {
    check(ark_hip_fr_csr_mul_device(h_, 0, x.device_ptr(), x.len(), out.device_ptr(), out.len()), "ark_hip_fr_csr_mul_device");
  }
  // y = M^T x: x has rows elements, y cols; needs with_transpose
  DeviceVec<FIELD_ID> mul_t(const DeviceVec<FIELD_ID>& x) const {
    DeviceVec<FIELD_ID> y = DeviceVec<FIELD_ID>::uninit(cols_);
    mul_t(x, y);
    return y;
  }
  void mul_t(const DeviceVec<FIELD_ID>& x, DeviceVec<FIELD_ID>& out) const {
    check(ark_hip_fr_csr_mul_device(h_, 1, x.device_ptr(), x.len(), out.device_ptr(), out.len()), "ark_hip_fr_csr_mul_device");
  }
  // u^T M v; with u = eq(rx, .), v = eq(ry, .) the value of the matrix's sparse multilinear extension at (rx, ry); waits for it
  Fr bilinear(const DeviceVec<FIELD_ID>& u, const DeviceVec<FIELD_ID>& v) const { return u.inner_product(mul(v)); }

 private:
  ark_hip_fr_csr* h_ = nullptr;
  size_t rows_ = 0, cols_ = 0, nnz_ = 0;
  bool has_t_ = false;
};

// The gate expression of a univariate (Plonk-style) prover on device vectors: a sum of products of
// columns, each factor read at a rotation,
//   out[i] = c0 + sum_j c_j prod_q col_{j,q}[(i + rot_{j,q}) mod n],
// in one call of ark_hip_fr_sum_of_products_device -- the univariate counterpart of ListOfProducts, shaped like it.  The columns
// are the caller's and must outlive the calls; evaluate is asynchronous on the library's stream.
struct SumOfProductsPlan { int blocks, rows_per_lane; };
// the launch geometry of evaluate over n rows; host only
inline SumOfProductsPlan sum_of_products_plan(size_t n) {
  SumOfProductsPlan p{};
  check(ark_hip_fr_sum_of_products_plan(n, &p.blocks, &p.rows_per_lane), "ark_hip_fr_sum_of_products_plan");
  return p;
}
template <int FIELD_ID>
class SumOfProducts {
 public:
  using Vec = DeviceVec<FIELD_ID>;
  struct Factor {
    const Vec* column;
    int64_t rotation;
    Factor(const Vec* c, int64_t r = 0) : column(c), rotation(r) {}
    Factor(const Vec& c, int64_t r = 0) : column(&c), rotation(r) {}
  };
  explicit SumOfProducts(size_t n) : n_(n) {}
  size_t len() const { return n_; }
  size_t num_columns() const { return columns_.size(); }
  size_t num_products() const { return lens_.size(); }
  // adds coefficient * prod factors (coefficient nullptr: one, which costs no product); a vector used in several products, or
  // several times in one, is one shared column (by device pointer)
  void add_product(const std::vector<Factor>& factors, const Fr* coefficient = nullptr) {
    if (factors.empty() || factors.size() > ARK_HIP_SOP_MAX_DEGREE) throw Error(ARK_HIP_ERR_ARG, "a product has 1 to 8 factors");
    if (lens_.size() >= ARK_HIP_SOP_MAX_TERMS) throw Error(ARK_HIP_ERR_ARG, "too many products");
    std::vector<const void*> columns = columns_;
    std::vector<unsigned> idx;
    for (const Factor& f : factors) {
      if (f.column->len() != n_) throw Error(ARK_HIP_ERR_ARG, "the factor's length differs from the expression's");
      size_t i = 0;
      while (i < columns.size() && columns[i] != f.column->device_ptr()) i++;
      if (i == columns.size()) columns.push_back(f.column->device_ptr());
      idx.push_back((unsigned)i);
    }
    if (columns.size() > ARK_HIP_SOP_MAX_COLUMNS) throw Error(ARK_HIP_ERR_ARG, "too many distinct columns");
    Fr c;
    if (coefficient) {
      c = *coefficient;
    } else {
      Fr any{};
      check(ark_hip_fr_pow(FIELD_ID, any.limbs.data(), 0, c.limbs.data()), "ark_hip_fr_pow");
    }
    columns_ = columns;
    lens_.push_back((unsigned)idx.size());
    flat_.insert(flat_.end(), idx.begin(), idx.end());
    for (const Factor& f : factors) rots_.push_back(f.rotation);
    coeffs_.push_back(c);
  }
  void set_constant(const Fr& c0) { c0_ = c0; has_c0_ = true; }
  void clear_constant() { has_c0_ = false; }
  // the expression's n rows
  Vec evaluate() const {
    Vec out = Vec::uninit(n_);
    evaluate(out);
    return out;
  }
  // the same into `out`: one of the columns only if every factor reads that column at a rotation that is 0 mod n
  void evaluate(Vec& out) const {
    if (lens_.empty()) throw Error(ARK_HIP_ERR_ARG, "no products");
    if (out.len() != n_) throw Error(ARK_HIP_ERR_ARG, "the output's length differs from the expression's");
    if (!n_) return;
    check(ark_hip_fr_sum_of_products_device(FIELD_ID, columns_.data(), (unsigned)columns_.size(), n_, lens_.data(), flat_.data(),
                                            rots_.data(), coeffs_[0].limbs.data(), (unsigned)lens_.size(),
                                            has_c0_ ? c0_.limbs.data() : nullptr, out.device_ptr()),
          "ark_hip_fr_sum_of_products_device");
  }

 private:
  size_t n_;
  std::vector<const void*> columns_;
  std::vector<unsigned> lens_, flat_;
  std::vector<int64_t> rots_;
  std::vector<Fr> coeffs_;
  Fr c0_{};
  bool has_c0_ = false;
};

// DenseMultilinearExtension<F> resident on the device (poly/src/evaluations/multivariate/multilinear/dense.rs): 2^num_vars
// evaluations over the boolean hypercube, index bit 0 being the first variable.  Committing to it is an MSM with Montgomery
// scalars on evaluations().device_ptr(); fix_variables and evaluate bind its variables where the table lies.
template <int FIELD_ID>
class DenseMultilinearExtension {
 public:
  using Vec = DeviceVec<FIELD_ID>;
  // from_evaluations_vec (dense.rs:58-70)
  DenseMultilinearExtension(size_t num_vars, Vec&& evaluations) : num_vars_(num_vars), evals_(std::move(evaluations)) {
    if (num_vars >= 64 || evals_.len() != (size_t)1 << num_vars) throw Error(ARK_HIP_ERR_ARG, "The size of evaluations should be 2^num_vars.");
  }
  static DenseMultilinearExtension from_evaluations_vec(size_t num_vars, const std::vector<Fr>& evaluations) {
    return DenseMultilinearExtension(num_vars, Vec::from_vec(evaluations));
  }
  static DenseMultilinearExtension zero() { return DenseMultilinearExtension(0, Vec(1)); }   // dense.rs:422-427
  // num_vars == 0 and a zero evaluation (dense.rs:429-431): one element is downloaded, and only when num_vars == 0
  bool is_zero() const { return num_vars_ == 0 && evals_.to_vec()[0] == Fr{}; }
  size_t num_vars() const { return num_vars_; }
  std::vector<Fr> to_evaluations() const { return evals_.to_vec(); }
  const Vec& evaluations() const { return evals_; }
  Vec& evaluations() { return evals_; }
  DenseMultilinearExtension clone() const { return DenseMultilinearExtension(num_vars_, evals_.clone()); }

  // binds the first partial_point.size() variables (dense.rs:224-257)
  DenseMultilinearExtension fix_variables(const std::vector<Fr>& partial_point) const {
    const size_t dim = partial_point.size();
    if (dim > num_vars_) throw Error(ARK_HIP_ERR_ARG, "invalid size of partial point");
    Vec out = Vec::uninit((size_t)1 << (num_vars_ - dim));
    check(ark_hip_mle_fix_variables_device(FIELD_ID, evals_.device_ptr(), (unsigned)num_vars_, (const uint64_t*)partial_point.data(),
                                           (unsigned)dim, out.device_ptr()), "ark_hip_mle_fix_variables_device");
    return DenseMultilinearExtension(num_vars_ - dim, std::move(out));
  }
  // Polynomial::evaluate (dense.rs:460-465); waits for its result
  Fr evaluate(const std::vector<Fr>& point) const {
    if (point.size() != num_vars_) throw Error(ARK_HIP_ERR_ARG, "point.len() == self.num_vars");
    Fr out;
    check(ark_hip_mle_evaluate_device(FIELD_ID, evals_.device_ptr(), (unsigned)num_vars_, (const uint64_t*)point.data(),
                                      out.limbs.data()), "ark_hip_mle_evaluate_device");
    return out;
  }
  // ---- openings ----
  // the table eq(point, b) = prod_i (b_i ? point_i : 1 - point_i), times *scale (nullptr: one), built on the device
  static DenseMultilinearExtension eq(const std::vector<Fr>& point, const Fr* scale = nullptr) {
    const size_t nv = point.size();
    if (nv >= 64) throw Error(ARK_HIP_ERR_ARG, "num_vars < 64");
    Vec out = Vec::uninit((size_t)1 << nv);
    check(ark_hip_mle_eq_table_device(FIELD_ID, (const uint64_t*)point.data(), (unsigned)nv, scale ? scale->limbs.data() : nullptr,
                                      out.device_ptr()), "ark_hip_mle_eq_table_device");
    return DenseMultilinearExtension(nv, std::move(out));
  }
  // f(point) and the quotients of f(x) - f(point) = sum_i (x_i - point_i) q_i(x_{i+1}, ..): one device vector of
  // 2^num_vars - 1 elements, q_i being the segment_len(i) elements from segment_offset(i) on -- views, no copies
  struct Quotients {
    Fr value;
    size_t num_vars = 0;
    Vec all;
    size_t segment_offset(size_t i) const { return ((size_t)1 << num_vars) - ((size_t)1 << (num_vars - i)); }
    size_t segment_len(size_t i) const { return (size_t)1 << (num_vars - 1 - i); }
    const void* segment_ptr(size_t i) const { return (const char*)all.device_ptr() + 32 * segment_offset(i); }
    std::vector<Fr> segment_to_vec(size_t i) const {
      std::vector<Fr> out(segment_len(i));
      check(ark_hip_memcpy_d2h(out.data(), segment_ptr(i), out.size() * 32), "ark_hip_memcpy_d2h");
      return out;
    }
  };
  Quotients quotients(const std::vector<Fr>& point) const {
    if (point.size() != num_vars_) throw Error(ARK_HIP_ERR_ARG, "point.len() == self.num_vars");
    Quotients q;
    q.num_vars = num_vars_;
    q.all = Vec::uninit(((size_t)1 << num_vars_) - 1);
    check(ark_hip_mle_quotients_device(FIELD_ID, evals_.device_ptr(), (unsigned)num_vars_, (const uint64_t*)point.data(),
                                       q.all.device_ptr(), q.value.limbs.data()), "ark_hip_mle_quotients_device");
    return q;
  }
  // f(point) and a commitment to every q_i: one device MSM per level over the segment where it lies.  d_bases_per_level[i]:
  // device array of 2^(num_vars-1-i) affine points of Curve, whose scalar field is this table's.  No verification, no hashing.
  template <class Curve>
  std::pair<Fr, std::vector<Projective<Curve::WORDS>>> open(const std::vector<Fr>& point,
                                                            const std::vector<const void*>& d_bases_per_level) const {
    static_assert(Curve::SCALAR_FIELD == FIELD_ID, "the curve's scalar field is the table's field");
    if (d_bases_per_level.size() != num_vars_) throw Error(ARK_HIP_ERR_ARG, "one base array per variable");
    Quotients q = quotients(point);
    std::vector<Projective<Curve::WORDS>> pts(num_vars_);
    for (size_t i = 0; i < num_vars_; i++)
      check(ark_hip_msm_sw_device(Curve::ID, d_bases_per_level[i], q.segment_ptr(i), q.segment_len(i), 1,
                                  reinterpret_cast<uint64_t*>(&pts[i])), "ark_hip_msm_sw_device");
    return {q.value, std::move(pts)};
  }
  // ---- grand products ----
  // The binary product tree pairing over the LAST variable: one device vector of 2^num_vars - 1 elements, level j
  // (1 <= j <= num_vars) being the level_len(j) = 2^(num_vars-j) elements from level_offset(j) on, level j's element i the
  // product of elements i and i + level_len(j) of level j - 1 (level 0: the table); the last element is the product.
  struct ProductTree {
    Fr product;
    size_t num_vars = 0;
    Vec all;
    size_t level_offset(size_t j) const { return ((size_t)1 << num_vars) - ((size_t)2 << (num_vars - j)); }
    size_t level_len(size_t j) const { return (size_t)1 << (num_vars - j); }
    Vec level(size_t j) const { return Vec::view(all, level_offset(j), level_len(j)); }
    std::vector<Fr> level_to_vec(size_t j) const { return level(j).to_vec(); }
  };
  ProductTree product_tree() const {
    ProductTree t;
    t.num_vars = num_vars_;
    t.all = Vec::uninit(((size_t)1 << num_vars_) - 1);
    check(ark_hip_mle_product_tree_device(FIELD_ID, evals_.device_ptr(), (unsigned)num_vars_, t.all.device_ptr(), t.product.limbs.data()),
          "ark_hip_mle_product_tree_device");
    return t;
  }
  // the launches of product_tree as ark_hip_mle_product_tree_plan reports them: (levels, log2 chunks per wave) per run
  static std::vector<std::pair<int, int>> product_tree_plan(size_t num_vars) {
    int passes = 0, widths[8], groups[8];
    check(ark_hip_mle_product_tree_plan((unsigned)num_vars, &passes, widths, groups), "ark_hip_mle_product_tree_plan");
    std::vector<std::pair<int, int>> out;
    for (int p = 0; p < passes; p++) out.push_back({widths[p], groups[p]});
    return out;
  }
  // c0 + sum_k coeffs[k] tables[k], entry by entry in one pass (c0 == nullptr: zero): the fingerprints that are the leaves
  // of a grand product; 1 to 8 tables of one size
  static DenseMultilinearExtension linear_combination(const std::vector<const DenseMultilinearExtension*>& tables,
                                                      const std::vector<Fr>& coeffs, const Fr* c0 = nullptr) {
    if (tables.empty() || tables.size() > 8 || coeffs.size() != tables.size()) throw Error(ARK_HIP_ERR_ARG, "1 to 8 tables, one coefficient each");
    std::vector<const void*> ptrs;
    for (auto* t : tables) {
      if (t->num_vars_ != tables[0]->num_vars_) throw Error(ARK_HIP_ERR_ARG, "num_vars differ");
      ptrs.push_back(t->evals_.device_ptr());
    }
    Vec out = Vec::uninit(tables[0]->evals_.len());
    check(ark_hip_fr_lincomb_device(FIELD_ID, ptrs.data(), (unsigned)ptrs.size(), (const uint64_t*)coeffs.data(),
                                    c0 ? c0->limbs.data() : nullptr, out.device_ptr(), out.len()), "ark_hip_fr_lincomb_device");
    return DenseMultilinearExtension(tables[0]->num_vars_, std::move(out));
  }
  // ---- fractional sums ----
  // The tree that adds the fractions num[b] / (*this)[b], pairing over the LAST variable (N = n0 d1 + n1 d0, D = d0 d1): two
  // device vectors of 2^num_vars - 1 elements in product_tree's layout, and the root (P, Q) with P / Q the sum.  Nothing is
  // inverted.
  struct FractionTree {
    Fr root_num, root_den;
    size_t num_vars = 0;
    Vec num, den;
    size_t level_offset(size_t j) const { return ((size_t)1 << num_vars) - ((size_t)2 << (num_vars - j)); }
    size_t level_len(size_t j) const { return (size_t)1 << (num_vars - j); }
    Vec num_level(size_t j) const { return Vec::view(num, level_offset(j), level_len(j)); }
    Vec den_level(size_t j) const { return Vec::view(den, level_offset(j), level_len(j)); }
  };
  // num == nullptr: every numerator is one
  FractionTree fraction_tree(const DenseMultilinearExtension* num) const {
    if (num && num->num_vars_ != num_vars_) throw Error(ARK_HIP_ERR_ARG, "num_vars differ");
    FractionTree t;
    t.num_vars = num_vars_;
    t.num = Vec::uninit(((size_t)1 << num_vars_) - 1);
    t.den = Vec::uninit(((size_t)1 << num_vars_) - 1);
    uint64_t root[8];
    check(ark_hip_mle_fraction_tree_device(FIELD_ID, num ? num->evals_.device_ptr() : nullptr, evals_.device_ptr(), (unsigned)num_vars_,
                                           t.num.device_ptr(), t.den.device_ptr(), root), "ark_hip_mle_fraction_tree_device");
    std::memcpy(t.root_num.limbs.data(), root, 32);
    std::memcpy(t.root_den.limbs.data(), root + 4, 32);
    return t;
  }
  // the launches of fraction_tree as ark_hip_mle_fraction_tree_plan reports them: (levels, 0) per run
  static std::vector<std::pair<int, int>> fraction_tree_plan(size_t num_vars, bool has_num = true) {
    int passes = 0, widths[8], groups[8];
    check(ark_hip_mle_fraction_tree_plan((unsigned)num_vars, has_num ? 1 : 0, &passes, widths, groups), "ark_hip_mle_fraction_tree_plan");
    std::vector<std::pair<int, int>> out;
    for (int p = 0; p < passes; p++) out.push_back({widths[p], groups[p]});
    return out;
  }
  // the multiplicity table of a lookup, m[j] = #{i : indices[i] = j} for j < table_len, counted on the device from n device
  // uint32_t.  An index >= table_len is skipped and not reported: the counts sum to n exactly when none was skipped.
  static Vec count_indices(const uint32_t* d_indices, size_t n, size_t table_len) {
    Vec out = Vec::uninit(table_len);
    check(ark_hip_fr_count_indices_device(FIELD_ID, d_indices, n, out.device_ptr(), table_len), "ark_hip_fr_count_indices_device");
    return out;
  }
  // ---- lookup by value ----
  // The join of a lookup from the values, on the device: mult[j] = #{i : values[i] is found at j} with j the FIRST occurrence of
  // the value in the table (a repeated table value keeps zero in its later cells), the number of cells of `values` that are not
  // in the table, and with want_indices the index of every cell (ARK_HIP_LOOKUP_MISSING where not found), downloaded.
  struct Lookup {
    Vec mult;
    uint64_t missing = 0;
    std::vector<uint32_t> indices;
  };
  static Lookup lookup(const Vec& table, const Vec& values, bool want_indices = false) {
    Lookup r;
    const size_t n = values.len();
    r.mult = Vec::uninit(table.len());
    void* d_idx = nullptr;
    if (want_indices && n) check(ark_hip_malloc(n * 4, &d_idx), "ark_hip_malloc");
    const int rc = ark_hip_fr_lookup_device(FIELD_ID, table.device_ptr(), table.len(), n ? values.device_ptr() : nullptr, n,
                                            static_cast<uint32_t*>(d_idx), r.mult.device_ptr(), &r.missing);
    if (rc == 0 && d_idx) {
      r.indices.resize(n);
      const int rc2 = ark_hip_memcpy_d2h(r.indices.data(), d_idx, n * 4);
      ark_hip_free(d_idx);
      check(rc2, "ark_hip_memcpy_d2h");
    } else if (d_idx) {
      ark_hip_free(d_idx);
    }
    check(rc, "ark_hip_fr_lookup_device");
    return r;
  }
  // (capacity_log, scratch_bytes) of lookup against a table of table_len values, as ark_hip_fr_lookup_plan reports them
  static std::pair<unsigned, size_t> lookup_plan(size_t table_len) {
    unsigned c = 0;
    size_t b = 0;
    check(ark_hip_fr_lookup_plan(table_len, &c, &b), "ark_hip_fr_lookup_plan");
    return {c, b};
  }
  // exchanges the k variables from position a with those from position b (dense.rs:76-92, :195-199)
  DenseMultilinearExtension relabel(size_t a, size_t b, size_t k) const {
    Vec out = Vec::uninit(evals_.len());
    check(ark_hip_mle_relabel_device(FIELD_ID, evals_.device_ptr(), (unsigned)num_vars_, (unsigned)a, (unsigned)b, (unsigned)k,
                                     out.device_ptr()), "ark_hip_mle_relabel_device");
    return DenseMultilinearExtension(num_vars_, std::move(out));
  }
  void relabel_in_place(size_t a, size_t b, size_t k) {
    check(ark_hip_mle_relabel_device(FIELD_ID, evals_.device_ptr(), (unsigned)num_vars_, (unsigned)a, (unsigned)b, (unsigned)k,
                                     evals_.device_ptr()), "ark_hip_mle_relabel_device");
  }
  // the tables one after the other, zero-filled up to the next power of two (dense.rs:133-156)
  static DenseMultilinearExtension concat(const std::vector<const DenseMultilinearExtension*>& polys) {
    size_t total = 0, nv = 0;
    for (auto* q : polys) total += q->evals_.len();
    while (((size_t)1 << nv) < total) nv++;
    Vec out = Vec::uninit((size_t)1 << nv);
    size_t at = 0;
    for (auto* q : polys) {
      check(ark_hip_memcpy_d2d((char*)out.device_ptr() + at * 32, q->evals_.device_ptr(), q->evals_.len() * 32), "ark_hip_memcpy_d2d");
      at += q->evals_.len();
    }
    if (at < out.len()) check(ark_hip_memset_device((char*)out.device_ptr() + at * 32, 0, (out.len() - at) * 32), "ark_hip_memset_device");
    return DenseMultilinearExtension(nv, std::move(out));
  }
  // +, - and neg (dense.rs:278-366): the constant zero on either side of + gives a copy of the other operand
  DenseMultilinearExtension operator+(const DenseMultilinearExtension& o) const {
    if (o.is_zero()) return clone();
    if (is_zero()) return o.clone();
    same(o);
    Vec out = Vec::uninit(evals_.len());
    check(ark_hip_fr_add_device(FIELD_ID, evals_.device_ptr(), o.evals_.device_ptr(), out.device_ptr(), out.len()), "ark_hip_fr_add_device");
    return DenseMultilinearExtension(num_vars_, std::move(out));
  }
  DenseMultilinearExtension operator-() const {
    Vec out = Vec::uninit(evals_.len());
    check(ark_hip_fr_neg_device(FIELD_ID, evals_.device_ptr(), out.device_ptr(), out.len()), "ark_hip_fr_neg_device");
    return DenseMultilinearExtension(num_vars_, std::move(out));
  }
  DenseMultilinearExtension operator-(const DenseMultilinearExtension& o) const {
    if (o.is_zero()) return clone();
    if (is_zero()) return -o;
    same(o);
    Vec out = Vec::uninit(evals_.len());
    check(ark_hip_fr_sub_device(FIELD_ID, evals_.device_ptr(), o.evals_.device_ptr(), out.device_ptr(), out.len()), "ark_hip_fr_sub_device");
    return DenseMultilinearExtension(num_vars_, std::move(out));
  }
  // times one field element; times zero gives zero() (dense.rs:376-392)
  DenseMultilinearExtension operator*(const Fr& k) const {
    if (k == Fr{}) return zero();
    return scaled(k);
  }
  // self += f * other in one pass over the tables (AddAssign<(F, &Self)>, dense.rs:319-327)
  void add_assign_scaled(const Fr& f, const DenseMultilinearExtension& o) {
    if (o.is_zero() || (o.num_vars_ == 0 && f == Fr{})) return;   // f * other is the constant zero
    if (is_zero()) { *this = o.scaled(f); return; }
    same(o);
    check(ark_hip_fr_axpy_device(FIELD_ID, evals_.device_ptr(), f.limbs.data(), o.evals_.device_ptr(), evals_.device_ptr(), evals_.len()),
          "ark_hip_fr_axpy_device");
  }
  DenseMultilinearExtension& operator+=(const DenseMultilinearExtension& o) { *this = *this + o; return *this; }
  DenseMultilinearExtension(DenseMultilinearExtension&&) noexcept = default;
  DenseMultilinearExtension& operator=(DenseMultilinearExtension&&) noexcept = default;

 private:
  size_t num_vars_ = 0;
  Vec evals_;
  void same(const DenseMultilinearExtension& o) const {
    if (o.num_vars_ != num_vars_) throw Error(ARK_HIP_ERR_ARG, "assert_eq!(self.num_vars, rhs.num_vars)");
  }
  DenseMultilinearExtension scaled(const Fr& k) const {
    Vec out = Vec::uninit(evals_.len());
    check(ark_hip_fr_scale_device(FIELD_ID, evals_.device_ptr(), k.limbs.data(), out.device_ptr(), out.len()), "ark_hip_fr_scale_device");
    return DenseMultilinearExtension(num_vars_, std::move(out));
  }
};

// The sumcheck prover over device-resident tables.  ListOfProducts has the shape of ark-linear-sumcheck's
// ListOfProductsOfPolynomials: sum_b sum_j c_j prod_{k in term j} f_k(b), the tables shared by pointer (the same
// DenseMultilinearExtension object added to several products, or twice to one, is one table; the caller keeps the objects
// alive and unmoved).  round() is one call of ark_hip_sumcheck_round_device on the tables where they lie; prove() runs the
// whole prover against the caller's source of challenges.  Nothing is hashed and nothing verified here.
template <int FIELD_ID>
struct SumcheckProof {
  std::vector<std::vector<Fr>> rounds;   // rounds[i]: the D + 1 evaluations g_i(0 .. D)
  std::vector<Fr> point;                 // the nu challenges
  std::vector<Fr> final_evaluations;     // f_k(point), the tables in the order they were first added
  Fr final_value;                        // sum_j c_j prod_k f_k(point): what the verifier's last check compares
};
// The Fiat-Shamir transcript of DESIGN.md section 23: 32 bytes of state the caller initialises; challenge() is one call of
// the host entry ark_hip_transcript_challenge (state | count | elements through SHAKE256; needs no device).
template <int FIELD_ID>
class Transcript {
 public:
  explicit Transcript(const std::array<uint8_t, 32>& seed) : state_(seed) {}
  const std::array<uint8_t, 32>& state() const { return state_; }
  uint8_t* state_ptr() { return state_.data(); }
  Fr challenge(const std::vector<Fr>& elements = {}) {
    Fr out;
    check(ark_hip_transcript_challenge(FIELD_ID, state_.data(), elements.empty() ? nullptr : (const uint64_t*)elements.data(),
                                       (unsigned)elements.size(), out.limbs.data()),
          "ark_hip_transcript_challenge");
    return out;
  }

 private:
  std::array<uint8_t, 32> state_;
};
template <int FIELD_ID>
class ListOfProducts {
 public:
  using Mle = DenseMultilinearExtension<FIELD_ID>;
  using Vec = DeviceVec<FIELD_ID>;
  explicit ListOfProducts(size_t num_vars) : num_vars_(num_vars), left_(num_vars) {}
  size_t num_vars() const { return num_vars_; }
  size_t max_multiplicands() const { return degree_; }
  // adds coefficient * prod mles
  void add_product(const std::vector<const Mle*>& mles, const Fr& coefficient) {
    if (mles.empty() || mles.size() > ARK_HIP_SUMCHECK_MAX_DEGREE) throw Error(ARK_HIP_ERR_ARG, "a product has 1 to 4 factors");
    if (lens_.size() >= ARK_HIP_SUMCHECK_MAX_TERMS) throw Error(ARK_HIP_ERR_ARG, "too many products");
    if (started_) throw Error(ARK_HIP_ERR_ARG, "rounds have been run on this list");
    std::vector<const Mle*> tables = tables_;
    std::vector<unsigned> idx;
    for (const Mle* m : mles) {
      if (m->num_vars() != num_vars_) throw Error(ARK_HIP_ERR_ARG, "the product's num_vars differ from the list's");
      size_t i = 0;
      while (i < tables.size() && tables[i] != m) i++;
      if (i == tables.size()) tables.push_back(m);
      idx.push_back((unsigned)i);
    }
    if (tables.size() > ARK_HIP_SUMCHECK_MAX_TABLES) throw Error(ARK_HIP_ERR_ARG, "too many distinct tables");
    tables_ = tables;
    lens_.push_back((unsigned)idx.size());
    flat_.insert(flat_.end(), idx.begin(), idx.end());
    coeffs_.push_back(coefficient);
    if (idx.size() > degree_) degree_ = idx.size();
  }
  // The D + 1 evaluations of the round polynomial over the tables as bound so far; with r_prev the first remaining variable
  // is bound to it first, in the same launch, into tables of the list's own (the caller's are never written).
  std::vector<Fr> round(const Fr* r_prev = nullptr) {
    if (lens_.empty() || left_ == 0) throw Error(ARK_HIP_ERR_ARG, "no products, or every variable is bound");
    if (!started_) {
      for (const Mle* m : tables_) cur_.push_back(m->evaluations().device_ptr());
      started_ = true;
    }
    if (!r_prev) return call(cur_, left_, nullptr, nullptr);
    if (sets_[0].empty())   // halves and quarters: the output of a bind is never the set it reads
      for (int s = 0; s < 2; s++)
        for (size_t k = 0; k < tables_.size(); k++) sets_[s].push_back(Vec::uninit((size_t)1 << (num_vars_ > (size_t)(1 + s) ? num_vars_ - 1 - s : 0)));
    std::vector<void*> outs;
    for (Vec& v : sets_[next_]) outs.push_back(v.device_ptr());
    std::vector<Fr> evals = call(cur_, left_, r_prev, outs.data());
    cur_.assign(outs.begin(), outs.end());
    left_--;
    next_ ^= 1;
    return evals;
  }
  // Runs the nu + 1 calls: call 0 has no bind, calls 1 .. nu bind the challenge before.  challenge(i, evals) gets round i's
  // evaluations and returns the verifier's element for it.
  template <class Challenge>
  SumcheckProof<FIELD_ID> prove(Challenge&& challenge) {
    if (started_ || num_vars_ == 0) throw Error(ARK_HIP_ERR_ARG, "rounds have been run on this list, or num_vars == 0");
    SumcheckProof<FIELD_ID> out;
    std::vector<Fr> evals = round();
    for (size_t i = 0; i < num_vars_; i++) {
      const Fr r = challenge(i, evals);
      out.rounds.push_back(evals);
      out.point.push_back(r);
      evals = round(&r);
    }
    for (const void* p : cur_) {   // the one-element tables: f_k(point)
      Fr v;
      check(ark_hip_memcpy_d2h(v.limbs.data(), p, 32), "ark_hip_memcpy_d2h");
      out.final_evaluations.push_back(v);
    }
    out.final_value = evals[0];
    return out;
  }
  // The whole proof in one wait: what prove() returns when challenge(i, evals) is transcript.challenge(evals), with the
  // challenges derived on the device (one call of ark_hip_sumcheck_prove_device).  Advances the transcript; allocates and frees
  // its own work vector.  tail_vars: -1 the library's default, 0 no one-workgroup tail, else the variables it starts at.
  SumcheckProof<FIELD_ID> prove_device(Transcript<FIELD_ID>& transcript, int tail_vars = -1) {
    if (started_ || num_vars_ == 0 || lens_.empty()) throw Error(ARK_HIP_ERR_ARG, "rounds have been run on this list, no products, or num_vars == 0");
    size_t work_elems = 0;
    int launches = 0, tail_from = 0;
    check(ark_hip_sumcheck_prove_plan((unsigned)num_vars_, (unsigned)tables_.size(), tail_vars, &work_elems, &launches, &tail_from),
          "ark_hip_sumcheck_prove_plan");
    Vec work = Vec::uninit(work_elems);
    std::vector<const void*> tables;
    for (const Mle* m : tables_) tables.push_back(m->evaluations().device_ptr());
    const size_t d1 = degree_ + 1;
    std::vector<Fr> rounds(num_vars_ * d1);
    SumcheckProof<FIELD_ID> out;
    out.point.resize(num_vars_);
    out.final_evaluations.resize(tables_.size());
    check(ark_hip_sumcheck_prove_device(FIELD_ID, tables.data(), (unsigned)tables.size(), (unsigned)num_vars_, lens_.data(), flat_.data(),
                                        (const uint64_t*)coeffs_.data(), (unsigned)lens_.size(), transcript.state_ptr(), tail_vars,
                                        work.device_ptr(), (uint64_t*)rounds.data(), (uint64_t*)out.point.data(),
                                        (uint64_t*)out.final_evaluations.data(), out.final_value.limbs.data()),
          "ark_hip_sumcheck_prove_device");
    for (size_t i = 0; i < num_vars_; i++) out.rounds.emplace_back(rounds.begin() + i * d1, rounds.begin() + (i + 1) * d1);
    return out;
  }

 private:
  size_t num_vars_, left_, degree_ = 0;
  std::vector<const Mle*> tables_;
  std::vector<unsigned> lens_, flat_;
  std::vector<Fr> coeffs_;
  std::vector<const void*> cur_;
  std::vector<Vec> sets_[2];
  int next_ = 0;
  bool started_ = false;
  std::vector<Fr> call(const std::vector<const void*>& tables, size_t num_vars, const Fr* r_prev, void* const* outs) {
    std::vector<Fr> evals(degree_ + 1);
    check(ark_hip_sumcheck_round_device(FIELD_ID, tables.data(), (unsigned)tables.size(), (unsigned)num_vars, lens_.data(), flat_.data(),
                                        (const uint64_t*)coeffs_.data(), (unsigned)lens_.size(), r_prev ? r_prev->limbs.data() : nullptr,
                                        outs, (uint64_t*)evals.data()),
          "ark_hip_sumcheck_round_device");
    return evals;
  }
};

// The layered proof of a grand product P = prod_b f[b] (Thaler's GKR grand product): the product tree,
// then per layer k = 1 .. nu - 1 one sumcheck of eq(r_k, x) L_{k+1}(x, 0) L_{k+1}(x, 1) over two views of the level, which
// leaves the claim left(rho) + tau (right(rho) - left(rho)) about L_{k+1}(rho, tau); the last claim is f(point), which
// evaluate / open answer.  challenge(layer, round, values) gets round = -1 and the pair (left, right) for a layer's tau.
// Nothing is hashed and nothing verified here; the table and the tree are not written.
template <int FIELD_ID>
struct GrandProductProof {
  Fr product;
  std::vector<std::optional<SumcheckProof<FIELD_ID>>> sumchecks;   // per layer; none for layer 0
  std::vector<std::pair<Fr, Fr>> pairs;                            // per layer: L_1's two elements, then (left(rho), right(rho))
  std::vector<Fr> point;                                           // r_nu: where the verifier's last claim about f lies
};
template <int FIELD_ID>
class GrandProduct {
 public:
  using Mle = DenseMultilinearExtension<FIELD_ID>;
  using Vec = DeviceVec<FIELD_ID>;
  explicit GrandProduct(const Mle& f) : f_(f) {}
  template <class Challenge>
  GrandProductProof<FIELD_ID> prove(Challenge&& challenge) const {
    const size_t nu = f_.num_vars();
    GrandProductProof<FIELD_ID> out;
    typename Mle::ProductTree tree = f_.product_tree();
    out.product = tree.product;
    if (nu == 0) return out;
    const Fr one = Mle::eq({}).to_evaluations()[0];   // the eq table of no variables is its scale, one
    {
      const std::vector<Fr> l1 = nu == 1 ? f_.to_evaluations() : tree.level_to_vec(nu - 1);   // L_1
      out.sumchecks.push_back(std::nullopt);
      out.pairs.push_back({l1[0], l1[1]});
      out.point = {challenge(size_t(0), -1, l1)};
    }
    for (size_t k = 1; k < nu; k++) {
      const size_t h = (size_t)1 << k;
      const bool top = k + 1 == nu;                   // L_(k+1) is the table itself
      const Vec& up_owner = top ? f_.evaluations() : tree.all;
      const size_t at = top ? 0 : tree.level_offset(nu - k - 1);
      const Mle eq = Mle::eq(out.point);
      const Mle left(k, Vec::view(up_owner, at, h)), right(k, Vec::view(up_owner, at + h, h));
      ListOfProducts<FIELD_ID> lp(k);
      lp.add_product({&eq, &left, &right}, one);
      SumcheckProof<FIELD_ID> sc = lp.prove([&](size_t i, const std::vector<Fr>& evals) { return challenge(k, (int)i, evals); });
      const std::pair<Fr, Fr> pair{sc.final_evaluations[1], sc.final_evaluations[2]};
      const Fr tau = challenge(k, -1, std::vector<Fr>{pair.first, pair.second});
      out.point = sc.point;
      out.point.push_back(tau);
      out.sumchecks.push_back(std::move(sc));
      out.pairs.push_back(pair);
    }
    return out;
  }

 private:
  const Mle& f_;
};

// The layered proof of a sum of fractions P / Q = sum_b num[b] / den[b] (the GKR form of logUp): the
// fraction tree, then per layer k = 1 .. nu - 1 one sumcheck of eq(r_k, x) (n0 d1 + n1 d0 + lambda d0 d1)(x) -- three products
// over the eq table and four views of the halves of the levels above -- whose sum is N_k(r_k) + lambda D_k(r_k); it leaves
// the claims n0 + tau (n1 - n0) and d0 + tau (d1 - d0) about N_{k+1}(rho, tau) and D_{k+1}(rho, tau).  The last claims are
// num(point) and den(point), which evaluate / open answer.  With ones for numerators (num == nullptr) the level above the
// last layer is the leaves: its products are eq d1, eq d0 and lambda eq d0 d1, and its values the pair (d0, d1).
// challenge(layer, round, values): round >= 0 carries that round's evaluations; TAU_ROUND = -1 carries the layer's values
// and asks for its tau; LAMBDA_ROUND = -2 carries no values and asks for the layer's batching challenge, before its sumcheck.
// Nothing is hashed and nothing verified here; the tables and the trees are not written.
template <int FIELD_ID>
struct FractionalSumProof {
  Fr root_num, root_den;                                           // (P, Q)
  std::vector<std::optional<SumcheckProof<FIELD_ID>>> sumchecks;   // per layer; none for layer 0
  std::vector<std::vector<Fr>> values;                             // per layer: (n0, n1, d0, d1), or (d0, d1) where the numerators are ones
  std::vector<Fr> point;                                           // r_nu: where the verifier's last claims lie
};
template <int FIELD_ID>
class FractionalSum {
 public:
  using Mle = DenseMultilinearExtension<FIELD_ID>;
  using Vec = DeviceVec<FIELD_ID>;
  static constexpr int TAU_ROUND = -1;
  static constexpr int LAMBDA_ROUND = -2;
  // num == nullptr: every numerator is one
  FractionalSum(const Mle* num, const Mle& den) : num_(num), den_(den) {
    if (num && num->num_vars() != den.num_vars()) throw Error(ARK_HIP_ERR_ARG, "num_vars differ");
  }
  template <class Challenge>
  FractionalSumProof<FIELD_ID> prove(Challenge&& challenge) const {
    const size_t nu = den_.num_vars();
    FractionalSumProof<FIELD_ID> out;
    typename Mle::FractionTree tree = den_.fraction_tree(num_);
    out.root_num = tree.root_num;
    out.root_den = tree.root_den;
    if (nu == 0) return out;
    const Fr one = Mle::eq({}).to_evaluations()[0];   // the eq table of no variables is its scale, one
    {
      std::vector<Fr> v;                              // N_1 (unless it is the implicit ones), then D_1
      if (nu > 1) v = tree.num_level(nu - 1).to_vec();
      else if (num_) v = num_->to_evaluations();
      const std::vector<Fr> d1 = nu == 1 ? den_.to_evaluations() : tree.den_level(nu - 1).to_vec();
      v.insert(v.end(), d1.begin(), d1.end());
      out.sumchecks.push_back(std::nullopt);
      out.point = {challenge(size_t(0), TAU_ROUND, v)};
      out.values.push_back(std::move(v));
    }
    for (size_t k = 1; k < nu; k++) {
      const Fr lambda = challenge(k, LAMBDA_ROUND, std::vector<Fr>{});
      const size_t h = (size_t)1 << k;
      const bool top = k + 1 == nu;                   // the levels above are the tables themselves
      const size_t at = top ? 0 : tree.level_offset(nu - k - 1);
      const Vec& d_owner = top ? den_.evaluations() : tree.den;
      const Mle eq = Mle::eq(out.point);
      const Mle d0(k, Vec::view(d_owner, at, h)), d1(k, Vec::view(d_owner, at + h, h));
      ListOfProducts<FIELD_ID> lp(k);
      std::vector<Fr> v;
      std::optional<SumcheckProof<FIELD_ID>> sc;
      auto ask = [&](size_t i, const std::vector<Fr>& evals) { return challenge(k, (int)i, evals); };
      if (top && !num_) {
        lp.add_product({&eq, &d1}, one);
        lp.add_product({&eq, &d0}, one);
        lp.add_product({&eq, &d0, &d1}, lambda);
        sc = lp.prove(ask);
        v = {sc->final_evaluations[2], sc->final_evaluations[1]};                                  // tables: eq, d1, d0
      } else {
        const Vec& n_owner = top ? num_->evaluations() : tree.num;
        const Mle n0(k, Vec::view(n_owner, at, h)), n1(k, Vec::view(n_owner, at + h, h));
        lp.add_product({&eq, &n0, &d1}, one);
        lp.add_product({&eq, &n1, &d0}, one);
        lp.add_product({&eq, &d0, &d1}, lambda);
        sc = lp.prove(ask);
        v = {sc->final_evaluations[1], sc->final_evaluations[3], sc->final_evaluations[4], sc->final_evaluations[2]};   // eq, n0, d1, n1, d0
      }
      const Fr tau = challenge(k, TAU_ROUND, v);
      out.point = sc->point;
      out.point.push_back(tau);
      out.sumchecks.push_back(std::move(sc));
      out.values.push_back(std::move(v));
    }
    return out;
  }

 private:
  const Mle* num_;
  const Mle& den_;
};

// ---- point vectors kept on the device: elementwise scalar multiplication, elementwise sum, two-scalar fold ----
// The reference maps `Projective *= ScalarField` (ec/src/models/short_weierstrass/group.rs:556-570 -> mul_bigint ->
// SWCurveConfig::mul_projective, short_weierstrass/mod.rs:101-109 -> double_and_add, ec/src/scalar_mul/mod.rs:29-60) and
// `Projective += Projective` (group.rs:450-538) over a vector with rayon.  DevicePoints<Curve> owns ark_hip_malloc memory
// holding Projective points and runs them where the points live (ark_hip_sw_mul_device / ark_hip_sw_add_device /
// ark_hip_sw_fold_device).  Asynchronous on the library's stream; to_vec() waits.  Results are group elements: compare
// after into_affine / normalize.  Mirrors: ark_hip::DevicePoints in rust/ark-hip/src/points.rs, algebra_amd.DevicePoints.
template <class Curve>
class DevicePoints {
 public:
  using AffineT = typename Curve::AffineT;
  using ProjectiveT = typename Curve::ProjectiveT;
  using Scalars = DeviceVec<Curve::SCALAR_FIELD>;
  DevicePoints() = default;
  static DevicePoints from_projective(const std::vector<ProjectiveT>& x) {
    DevicePoints v;
    v.alloc(x.size());
    if (!x.empty()) check(ark_hip_memcpy_h2d(v.p_, x.data(), x.size() * sizeof(ProjectiveT)), "ark_hip_memcpy_h2d");
    return v;
  }
  // Affine points (an SRS as it is stored), converted on the device: [1] P_i with the shared canonical scalar one
  static DevicePoints from_affine(const std::vector<AffineT>& x) {
    DevicePoints v;
    v.alloc(x.size());
    if (x.empty()) return v;
    const size_t bytes = x.size() * sizeof(AffineT);
    void* tmp = nullptr;
    check(ark_hip_malloc(bytes + 32, &tmp), "ark_hip_malloc");
    const uint64_t one[4] = {1, 0, 0, 0};
    void* d_one = static_cast<char*>(tmp) + bytes;
    int rc = ark_hip_memcpy_h2d(tmp, x.data(), bytes);
    if (!rc) rc = ark_hip_memcpy_h2d(d_one, one, 32);
    if (!rc) rc = ark_hip_sw_mul_device(Curve::ID, tmp, ARK_HIP_FORM_AFFINE, d_one, 1, 0, x.size(), v.p_);
    const int rf = ark_hip_free(tmp);   // waits for the stream
    check(rc, "ark_hip_sw_mul_device");
    check(rf, "ark_hip_free");
    return v;
  }
  DevicePoints(DevicePoints&& o) noexcept : p_(o.p_), len_(o.len_) { o.p_ = nullptr; o.len_ = 0; }
  DevicePoints& operator=(DevicePoints&& o) noexcept {
    if (this != &o) { release(); p_ = o.p_; len_ = o.len_; o.p_ = nullptr; o.len_ = 0; }
    return *this;
  }
  DevicePoints(const DevicePoints&) = delete;
  DevicePoints& operator=(const DevicePoints&) = delete;
  ~DevicePoints() { release(); }
  DevicePoints clone() const {
    DevicePoints v;
    v.alloc(len_);
    if (len_) check(ark_hip_memcpy_d2d(v.p_, p_, len_ * sizeof(ProjectiveT)), "ark_hip_memcpy_d2d");
    return v;
  }
  std::vector<ProjectiveT> to_vec() const {
    std::vector<ProjectiveT> out(len_);
    if (len_) check(ark_hip_memcpy_d2h(out.data(), p_, len_ * sizeof(ProjectiveT)), "ark_hip_memcpy_d2h");
    return out;
  }
  size_t len() const { return len_; }
  void* device_ptr() { return p_; }
  const void* device_ptr() const { return p_; }
  // self[i] *= scalars[i], the scalars (Montgomery Fr) already on the device
  DevicePoints& mul_assign(const Scalars& scalars) {
    if (scalars.len() != len_) throw Error(ARK_HIP_ERR_ARG, "one scalar per point");
    check(ark_hip_sw_mul_device(Curve::ID, p_, ARK_HIP_FORM_PROJECTIVE, scalars.device_ptr(), len_, 1, len_, p_), "ark_hip_sw_mul_device");
    return *this;
  }
  // self[i] *= k for one scalar (Montgomery Fr) shared by every point
  DevicePoints& mul_assign(const Fr& k) {
    Scalars s = Scalars::from_slice(&k, 1);
    check(ark_hip_sw_mul_device(Curve::ID, p_, ARK_HIP_FORM_PROJECTIVE, s.device_ptr(), 1, 1, len_, p_), "ark_hip_sw_mul_device");
    return *this;   // s is freed here: ark_hip_free waits for the stream
  }
  DevicePoints& operator+=(const DevicePoints& o) { return add_signed(o, 0); }
  DevicePoints& operator-=(const DevicePoints& o) { return add_signed(o, 1); }
  // [a] self[i] + [b] hi[i] on one joint doubling chain (a, b: Montgomery Fr)
  DevicePoints fold(const DevicePoints& hi, const Fr& a, const Fr& b) const {
    if (hi.len_ != len_) throw Error(ARK_HIP_ERR_ARG, "vectors of unequal length");
    DevicePoints out;
    out.alloc(len_);
    check(ark_hip_sw_fold_device(Curve::ID, p_, hi.p_, ARK_HIP_FORM_PROJECTIVE, a.limbs.data(), b.limbs.data(), 1, len_, out.p_),
          "ark_hip_sw_fold_device");
    return out;
  }
  // CurveGroup::normalize_batch on the device, one download
  std::vector<AffineT> normalize_to_vec() const {
    std::vector<AffineT> out(len_);
    if (!len_) return out;
    void* tmp = nullptr;
    check(ark_hip_malloc(len_ * sizeof(AffineT), &tmp), "ark_hip_malloc");
    int rc = ark_hip_sw_normalize_batch_device(Curve::ID, p_, tmp, len_);
    if (!rc) rc = ark_hip_memcpy_d2h(out.data(), tmp, len_ * sizeof(AffineT));
    const int rf = ark_hip_free(tmp);
    check(rc, "ark_hip_sw_normalize_batch_device");
    check(rf, "ark_hip_free");
    return out;
  }

 private:
  void* p_ = nullptr;
  size_t len_ = 0;
  void alloc(size_t len) {
    len_ = len;
    if (len) check(ark_hip_malloc(len * sizeof(ProjectiveT), &p_), "ark_hip_malloc");
  }
  void release() {
    if (p_) (void)ark_hip_free(p_);
    p_ = nullptr;
    len_ = 0;
  }
  DevicePoints& add_signed(const DevicePoints& o, int negate) {
    if (o.len_ != len_) throw Error(ARK_HIP_ERR_ARG, "vectors of unequal length");
    check(ark_hip_sw_add_device(Curve::ID, p_, o.p_, negate, len_, p_), "ark_hip_sw_add_device");
    return *this;
  }
};
// host slices through the staged entry (ark_hip_sw_mul): out[i] = [k_i] P_i, Montgomery Fr scalars, one per point or one for all
template <class Curve>
inline std::vector<typename Curve::ProjectiveT> sw_mul(const std::vector<typename Curve::AffineT>& points, const std::vector<Fr>& scalars) {
  std::vector<typename Curve::ProjectiveT> out(points.size());
  check(ark_hip_sw_mul(Curve::ID, reinterpret_cast<const uint64_t*>(points.data()), ARK_HIP_FORM_AFFINE,
                       reinterpret_cast<const uint64_t*>(scalars.data()), scalars.size(), 1, points.size(),
                       reinterpret_cast<uint64_t*>(out.data())),
        "ark_hip_sw_mul");
  return out;
}

// ---- one-word prime fields: SmallFp<P> for Goldilocks, BabyBear, KoalaBear (ark_hip_sfp_*) ---------------------------------
// An element is SmallFp::value, the canonical Montgomery residue in the field's own word; single elements are uint64_t.
template <int SFIELD_ID>
struct SmallWord { using type = uint32_t; };
template <>
struct SmallWord<ARK_HIP_SFP_GOLDILOCKS> { using type = uint64_t; };

struct SmallFieldInfo { uint64_t bytes, p, k_bits, r, r2, generator, two_adicity, two_adic_root; };
template <int SFIELD_ID>
inline SmallFieldInfo small_field_info() {
  uint64_t o[8];
  check(ark_hip_sfp_info(SFIELD_ID, o), "ark_hip_sfp_info");
  return SmallFieldInfo{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]};
}
template <int SFIELD_ID>
inline uint64_t small_field_pow(uint64_t base, uint64_t exp) {
  uint64_t out = 0;
  check(ark_hip_sfp_pow(SFIELD_ID, base, exp, &out), "ark_hip_sfp_pow");
  return out;
}
struct SmallFftPlan { int single_log, tile_log, seg_log; std::vector<int> stages; };
template <int SFIELD_ID>
inline SmallFftPlan small_fft_plan(unsigned log_n) {
  int o[8];
  check(ark_hip_sfp_fft_plan(SFIELD_ID, log_n, o), "ark_hip_sfp_fft_plan");
  return SmallFftPlan{o[0], o[1], o[2], std::vector<int>(o + 4, o + 4 + o[3])};
}

template <int SFIELD_ID>
class SmallRadix2EvaluationDomain {
 public:
  using Word = typename SmallWord<SFIELD_ID>::type;
  // Radix2EvaluationDomain::new: nullopt beyond the field's two-adicity
  static std::optional<SmallRadix2EvaluationDomain> create(size_t num_coeffs) {
    SmallRadix2EvaluationDomain d;
    const int rc = ark_hip_sfp_radix2_domain_new(SFIELD_ID, num_coeffs, &d.s_);
    if (rc == ARK_HIP_ERR_SIZE) return std::nullopt;
    check(rc, "ark_hip_sfp_radix2_domain_new");
    return d;
  }
  std::optional<SmallRadix2EvaluationDomain> get_coset(uint64_t offset) const {
    if (offset == 0) return std::nullopt;
    SmallRadix2EvaluationDomain d;
    check(ark_hip_sfp_radix2_domain_get_coset(SFIELD_ID, &s_, offset, &d.s_), "ark_hip_sfp_radix2_domain_get_coset");
    return d;
  }
  size_t size() const { return (size_t)s_.size; }
  uint32_t log_size_of_group() const { return s_.log_size_of_group; }
  uint64_t size_inv() const { return s_.size_inv; }
  uint64_t group_gen() const { return s_.group_gen; }
  uint64_t group_gen_inv() const { return s_.group_gen_inv; }
  uint64_t coset_offset() const { return s_.offset; }
  uint64_t coset_offset_inv() const { return s_.offset_inv; }
  uint64_t coset_offset_pow_size() const { return s_.offset_pow_size; }
  const ark_hip_sfp_radix2_domain& raw() const { return s_; }
  // host slices: zero-extended to the domain, one upload and one download
  void fft_in_place(std::vector<Word>& x) const { host(x, 0); }
  void ifft_in_place(std::vector<Word>& x) const { host(x, 1); }
  // count columns on the device, `stride` elements apart; num_coeffs = 0: the whole column
  void fft_batch_in_place(void* d_data, size_t count, size_t stride, size_t num_coeffs = 0, bool inverse = false) const {
    check(ark_hip_sfp_fft_batch_device(SFIELD_ID, &s_, d_data, count, stride, num_coeffs ? num_coeffs : size(), inverse ? 1 : 0),
          "ark_hip_sfp_fft_batch_device");
  }

 private:
  void host(std::vector<Word>& x, int inverse) const {
    if (x.size() > size()) throw Error(ARK_HIP_ERR_ARG, "more elements than the domain holds");
    x.resize(size(), 0);
    check(ark_hip_sfp_fft_in_place(SFIELD_ID, &s_, x.data(), inverse), "ark_hip_sfp_fft_in_place");
  }
  ark_hip_sfp_radix2_domain s_{};
};

template <int SFIELD_ID>
class SmallDeviceVec {
 public:
  using Word = typename SmallWord<SFIELD_ID>::type;
  using Domain = SmallRadix2EvaluationDomain<SFIELD_ID>;
  SmallDeviceVec() = default;
  explicit SmallDeviceVec(size_t len) {   // vec![F::zero(); len]
    alloc(len);
    if (len) check(ark_hip_memset_device(p_, 0, len * sizeof(Word)), "ark_hip_memset_device");
  }
  static SmallDeviceVec from_vec(const std::vector<Word>& x) {
    SmallDeviceVec v;
    v.alloc(x.size());
    if (!x.empty()) check(ark_hip_memcpy_h2d(v.p_, x.data(), x.size() * sizeof(Word)), "ark_hip_memcpy_h2d");
    return v;
  }
  SmallDeviceVec(SmallDeviceVec&& o) noexcept : p_(o.p_), len_(o.len_) { o.p_ = nullptr; o.len_ = 0; }
  SmallDeviceVec& operator=(SmallDeviceVec&& o) noexcept {
    if (this != &o) { release(); p_ = o.p_; len_ = o.len_; o.p_ = nullptr; o.len_ = 0; }
    return *this;
  }
  SmallDeviceVec(const SmallDeviceVec&) = delete;
  SmallDeviceVec& operator=(const SmallDeviceVec&) = delete;
  ~SmallDeviceVec() { release(); }
  SmallDeviceVec clone() const {
    SmallDeviceVec v;
    v.alloc(len_);
    if (len_) check(ark_hip_memcpy_d2d(v.p_, p_, len_ * sizeof(Word)), "ark_hip_memcpy_d2d");
    return v;
  }
  std::vector<Word> to_vec() const {
    std::vector<Word> out(len_);
    if (len_) check(ark_hip_memcpy_d2h(out.data(), p_, len_ * sizeof(Word)), "ark_hip_memcpy_d2h");
    return out;
  }
  size_t len() const { return len_; }
  void* device_ptr() { return p_; }
  const void* device_ptr() const { return p_; }
  SmallDeviceVec& operator+=(const SmallDeviceVec& o) { same(o); check(ark_hip_sfp_add_device(SFIELD_ID, p_, o.p_, p_, len_), "ark_hip_sfp_add_device"); return *this; }
  SmallDeviceVec& operator-=(const SmallDeviceVec& o) { same(o); check(ark_hip_sfp_sub_device(SFIELD_ID, p_, o.p_, p_, len_), "ark_hip_sfp_sub_device"); return *this; }
  SmallDeviceVec& operator*=(const SmallDeviceVec& o) { same(o); check(ark_hip_sfp_mul_device(SFIELD_ID, p_, o.p_, p_, len_), "ark_hip_sfp_mul_device"); return *this; }
  SmallDeviceVec& scale(uint64_t k) { check(ark_hip_sfp_scale_device(SFIELD_ID, p_, k, p_, len_), "ark_hip_sfp_scale_device"); return *this; }
  SmallDeviceVec& negate() { check(ark_hip_sfp_neg_device(SFIELD_ID, p_, p_, len_), "ark_hip_sfp_neg_device"); return *this; }
  SmallDeviceVec& batch_inverse() { check(ark_hip_sfp_inverse_device(SFIELD_ID, p_, p_, len_), "ark_hip_sfp_inverse_device"); return *this; }
  SmallDeviceVec& from_canonical() { check(ark_hip_sfp_from_canonical_device(SFIELD_ID, p_, p_, len_), "ark_hip_sfp_from_canonical_device"); return *this; }
  SmallDeviceVec& into_canonical() { check(ark_hip_sfp_into_canonical_device(SFIELD_ID, p_, p_, len_), "ark_hip_sfp_into_canonical_device"); return *this; }
  // DensePolynomial::evaluate_over_domain: domain.size() evaluations of these 1 .. size coefficients
  SmallDeviceVec evaluate_over_domain(const Domain& d) const {
    if (len_ == 0 || len_ > d.size()) throw Error(ARK_HIP_ERR_ARG, "1 .. domain.size() coefficients");
    SmallDeviceVec out;
    out.alloc(d.size());
    check(ark_hip_memcpy_d2d(out.p_, p_, len_ * sizeof(Word)), "ark_hip_memcpy_d2d");
    d.fft_batch_in_place(out.p_, 1, d.size(), len_, false);
    return out;
  }
  // Evaluations::interpolate
  SmallDeviceVec interpolate(const Domain& d) const {
    if (len_ != d.size()) throw Error(ARK_HIP_ERR_ARG, "one evaluation per element of the domain");
    SmallDeviceVec out = clone();
    d.fft_batch_in_place(out.p_, 1, d.size(), 0, true);
    return out;
  }

 private:
  void alloc(size_t len) {
    check(ark_hip_malloc((len ? len : 1) * sizeof(Word), &p_), "ark_hip_malloc");
    len_ = len;
  }
  void release() {
    if (p_) (void)ark_hip_free(p_);
    p_ = nullptr;
    len_ = 0;
  }
  void same(const SmallDeviceVec& o) const {
    if (o.len_ != len_) throw Error(ARK_HIP_ERR_ARG, "vectors of one length are combined");
  }
  void* p_ = nullptr;
  size_t len_ = 0;
};

// ---- Merkle commitments: SHA3-256 trees over column batches (ark_hip_merkle_*) ------------------------------------------------
// An extension (the reference has no Merkle tree); a leaf hashes the bytes serialize_compressed writes for the row's elements.
using Digest = std::array<uint8_t, ARK_HIP_MERKLE_DIGEST_BYTES>;
struct MerklePlan { uint64_t tree_bytes, leaf_permutations, launches, tail_level, leaf_blocks, node_blocks, levels_per_launch, permutation; };
inline MerklePlan merkle_plan(size_t n, size_t count, unsigned elem_bytes) {
  uint64_t o[8];
  check(ark_hip_merkle_plan(n, count, elem_bytes, o), "ark_hip_merkle_plan");
  return MerklePlan{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]};
}
inline Digest merkle_node(const Digest& left, const Digest& right) {
  Digest d;
  check(ark_hip_merkle_node(left.data(), right.data(), d.data()), "ark_hip_merkle_node");
  return d;
}
template <int SFIELD_ID>
inline Digest merkle_leaf_small(const std::vector<typename SmallWord<SFIELD_ID>::type>& row) {
  Digest d;
  check(ark_hip_merkle_leaf_sfp(SFIELD_ID, row.data(), row.size(), d.data()), "ark_hip_merkle_leaf_sfp");
  return d;
}
template <int FIELD_ID>
inline Digest merkle_leaf_fr(const std::vector<Fr>& row) {
  Digest d;
  check(ark_hip_merkle_leaf_fr(FIELD_ID, (const uint64_t*)row.data(), row.size(), d.data()), "ark_hip_merkle_leaf_fr");
  return d;
}

// The tree of a committed matrix, in device memory.  The matrix stays the caller's: it must outlive every open() that asks for rows.
class MerkleTree {
 public:
  MerkleTree() = default;
  // count columns of n = 2^k one-word elements, column j at element offset j * stride of `data`
  template <int SFIELD_ID>
  static MerkleTree commit_small(const SmallDeviceVec<SFIELD_ID>& data, size_t count, size_t stride, size_t n, bool wait = true) {
    if (count == 0 || stride < n || (count - 1) * stride + n > data.len()) throw Error(ARK_HIP_ERR_ARG, "the matrix lies inside the vector");
    MerkleTree t(data.device_ptr(), sizeof(typename SmallWord<SFIELD_ID>::type), count, stride, n);
    check(ark_hip_merkle_commit_sfp_device(SFIELD_ID, t.data_, count, stride, n, t.tree_, wait ? t.root_.data() : nullptr),
          "ark_hip_merkle_commit_sfp_device");
    t.have_root_ = wait;
    return t;
  }
  // count columns of data.len() / count Fr elements each, one after the other
  template <int FIELD_ID>
  static MerkleTree commit_fr(const DeviceVec<FIELD_ID>& data, size_t count = 1, bool wait = true) {
    if (count == 0 || data.len() == 0 || data.len() % count) throw Error(ARK_HIP_ERR_ARG, "count columns of one length");
    const size_t n = data.len() / count;
    MerkleTree t(data.device_ptr(), 32, count, n, n);
    check(ark_hip_merkle_commit_fr_device(FIELD_ID, t.data_, count, n, n, t.tree_, wait ? t.root_.data() : nullptr),
          "ark_hip_merkle_commit_fr_device");
    t.have_root_ = wait;
    return t;
  }
  MerkleTree(MerkleTree&& o) noexcept { *this = std::move(o); }
  MerkleTree& operator=(MerkleTree&& o) noexcept {
    if (this != &o) {
      release();
      tree_ = o.tree_; data_ = o.data_; elem_bytes_ = o.elem_bytes_; count_ = o.count_; stride_ = o.stride_; n_ = o.n_;
      root_ = o.root_; have_root_ = o.have_root_;
      o.tree_ = nullptr;
    }
    return *this;
  }
  MerkleTree(const MerkleTree&) = delete;
  MerkleTree& operator=(const MerkleTree&) = delete;
  ~MerkleTree() { release(); }
  size_t size() const { return n_; }
  size_t log_size() const { size_t k = 0; while (((size_t)1 << k) < n_) k++; return k; }
  const void* device_ptr() const { return tree_; }
  // after an asynchronous commit: a waiting 32-byte download
  const Digest& root() {
    if (!have_root_) check(ark_hip_memcpy_d2h(root_.data(), tree_, root_.size()), "ark_hip_memcpy_d2h");
    have_root_ = true;
    return root_;
  }
  // rows: q * count elements in memory form, as bytes; paths: q * log n digests, siblings from the leaf level upwards
  struct Opening { std::vector<uint8_t> rows, paths; };
  Opening open(const std::vector<uint64_t>& indices, bool rows = true) const {
    Opening o;
    o.paths.resize(indices.size() * log_size() * ARK_HIP_MERKLE_DIGEST_BYTES);
    if (rows) o.rows.resize(indices.size() * count_ * elem_bytes_);
    check(ark_hip_merkle_open_device(tree_, n_, rows ? data_ : nullptr, elem_bytes_, count_, stride_, indices.data(), indices.size(),
                                     rows ? o.rows.data() : nullptr, o.paths.data()), "ark_hip_merkle_open_device");
    return o;
  }
  // one opening against a root, on the host; row: the count elements in memory form
  template <int SFIELD_ID>
  static bool verify_small(const Digest& root, size_t n, uint64_t index, const void* row, size_t count, const uint8_t* path) {
    int ok = 0;
    check(ark_hip_merkle_verify_sfp(SFIELD_ID, root.data(), n, index, row, count, path, &ok), "ark_hip_merkle_verify_sfp");
    return ok != 0;
  }
  template <int FIELD_ID>
  static bool verify_fr(const Digest& root, size_t n, uint64_t index, const void* row, size_t count, const uint8_t* path) {
    int ok = 0;
    check(ark_hip_merkle_verify_fr(FIELD_ID, root.data(), n, index, (const uint64_t*)row, count, path, &ok), "ark_hip_merkle_verify_fr");
    return ok != 0;
  }

 private:
  MerkleTree(const void* data, unsigned elem_bytes, size_t count, size_t stride, size_t n)
      : data_(data), elem_bytes_(elem_bytes), count_(count), stride_(stride), n_(n) {
    if (n == 0 || (n & (n - 1))) throw Error(ARK_HIP_ERR_ARG, "a column holds 2^k elements");
    check(ark_hip_malloc((2 * n - 1) * ARK_HIP_MERKLE_DIGEST_BYTES, &tree_), "ark_hip_malloc");
  }
  void release() {
    if (tree_) (void)ark_hip_free(tree_);
    tree_ = nullptr;
  }
  void* tree_ = nullptr;
  const void* data_ = nullptr;
  unsigned elem_bytes_ = 0;
  size_t count_ = 0, stride_ = 0, n_ = 0;
  Digest root_{};
  bool have_root_ = false;
};

// ---- extension fields over the one-word fields, and FRI over them (ark_hip_xfp_*, ark_hip_fri_*) ----------------------------------
// Fp2 = Fp[u] / (u^2 - 7) over Goldilocks; Fp4 = Fp2[v] / (v^2 - u) over Fp2 = Fp[u] / (u^2 - W) for BabyBear (W = 11) and KoalaBear
// (W = 3): the reference's tower models over SmallFp<P>.  An element is its d components in the order CanonicalSerialize writes
// them, each a stored word, zero-extended to four.
using ExtElement = std::array<uint64_t, 4>;
template <int SFIELD_ID>
constexpr unsigned small_ext_degree() { return SFIELD_ID == ARK_HIP_SFP_GOLDILOCKS ? 2 : 4; }
struct SmallExtInfo { unsigned degree; uint64_t w, w_stored; std::array<unsigned, 4> exponents; };
template <int SFIELD_ID>
inline SmallExtInfo small_ext_info() {
  uint64_t o[8];
  check(ark_hip_xfp_info(SFIELD_ID, o), "ark_hip_xfp_info");
  return SmallExtInfo{(unsigned)o[0], o[1], o[2], {(unsigned)o[3], (unsigned)o[4], (unsigned)o[5], (unsigned)o[6]}};
}
template <int SFIELD_ID>
inline ExtElement ext_mul(const ExtElement& a, const ExtElement& b) {
  ExtElement r;
  check(ark_hip_xfp_mul(SFIELD_ID, a.data(), b.data(), r.data()), "ark_hip_xfp_mul");
  return r;
}
template <int SFIELD_ID>
inline ExtElement ext_inverse(const ExtElement& a) {
  ExtElement r;
  check(ark_hip_xfp_inverse(SFIELD_ID, a.data(), r.data()), "ark_hip_xfp_inverse");
  return r;
}
template <int SFIELD_ID>
inline ExtElement ext_pow(const ExtElement& a, uint64_t e) {
  ExtElement r;
  check(ark_hip_xfp_pow(SFIELD_ID, a.data(), e, r.data()), "ark_hip_xfp_pow");
  return r;
}

// n extension elements on the device: d columns of `stride` words in one SmallDeviceVec, component k at element offset k * stride.
// The base-field transform with count = d, += / -= / negate / scale of data() and MerkleTree::commit_small with count = d are the
// extension's.
template <int SFIELD_ID>
class SmallExtVec {
 public:
  using Word = typename SmallWord<SFIELD_ID>::type;
  static constexpr unsigned D = small_ext_degree<SFIELD_ID>();
  SmallExtVec() = default;
  explicit SmallExtVec(size_t n, size_t stride = 0) : data_(D * (stride ? stride : n)), n_(n), stride_(stride ? stride : n) {
    if (stride_ < n_) throw Error(ARK_HIP_ERR_ARG, "stride >= n");
  }
  // components: d vectors of n stored words
  static SmallExtVec from_components(const std::vector<std::vector<Word>>& c) {
    if (c.size() != D) throw Error(ARK_HIP_ERR_ARG, "d components");
    std::vector<Word> flat;
    for (const auto& col : c) {
      if (col.size() != c[0].size()) throw Error(ARK_HIP_ERR_ARG, "components of one length");
      flat.insert(flat.end(), col.begin(), col.end());
    }
    SmallExtVec v;
    v.n_ = v.stride_ = c[0].size();
    v.data_ = SmallDeviceVec<SFIELD_ID>::from_vec(flat);
    return v;
  }
  size_t len() const { return n_; }
  size_t stride() const { return stride_; }
  SmallDeviceVec<SFIELD_ID>& data() { return data_; }
  const SmallDeviceVec<SFIELD_ID>& data() const { return data_; }
  void* device_ptr() { return data_.device_ptr(); }
  const void* device_ptr() const { return data_.device_ptr(); }
  SmallExtVec& operator*=(const SmallExtVec& o) {
    if (o.n_ != n_) throw Error(ARK_HIP_ERR_ARG, "vectors of one length are combined");
    check(ark_hip_xfp_vec_mul(SFIELD_ID, device_ptr(), stride_, o.device_ptr(), o.stride_, device_ptr(), stride_, n_), "ark_hip_xfp_vec_mul");
    return *this;
  }
  SmallExtVec& batch_inverse() {
    check(ark_hip_xfp_vec_inverse(SFIELD_ID, device_ptr(), stride_, device_ptr(), stride_, n_), "ark_hip_xfp_vec_inverse");
    return *this;
  }
  SmallExtVec& mul_const(const ExtElement& k) {
    check(ark_hip_xfp_vec_mul_const(SFIELD_ID, device_ptr(), stride_, k.data(), device_ptr(), stride_, n_), "ark_hip_xfp_vec_mul_const");
    return *this;
  }
  SmallExtVec& mul_base(const SmallDeviceVec<SFIELD_ID>& b) {
    if (b.len() != n_) throw Error(ARK_HIP_ERR_ARG, "one base-field word per element");
    check(ark_hip_xfp_vec_mul_base(SFIELD_ID, device_ptr(), stride_, b.device_ptr(), device_ptr(), stride_, n_), "ark_hip_xfp_vec_mul_base");
    return *this;
  }

 private:
  SmallDeviceVec<SFIELD_ID> data_;
  size_t n_ = 0, stride_ = 0;
};

// out[i] (+)= alpha^first_power * sum_j alpha^j col_j[i] over `count` columns of `rows` words, `stride` apart, inside `cols`
template <int SFIELD_ID>
inline void combine_columns(const SmallDeviceVec<SFIELD_ID>& cols, size_t count, size_t stride, size_t rows, const ExtElement& alpha,
                            SmallExtVec<SFIELD_ID>& out, uint64_t first_power = 0, bool accumulate = false) {
  if (count == 0 || stride < rows || (count - 1) * stride + rows > cols.len() || out.len() != rows)
    throw Error(ARK_HIP_ERR_ARG, "the matrix lies inside the vector, one element per row");
  check(ark_hip_xfp_combine_columns(SFIELD_ID, cols.device_ptr(), count, stride, rows, alpha.data(), first_power, out.device_ptr(), out.stride(),
                                    accumulate ? 1 : 0), "ark_hip_xfp_combine_columns");
}

struct FriLayer { unsigned log_size, log_arity; uint64_t layer_offset, tree_offset; unsigned lo_bits; };
struct FriPlan { unsigned degree; uint64_t layer_words, tree_bytes, launches_per_fold, final_size, final_copy_offset; std::vector<FriLayer> layers; };
template <int SFIELD_ID>
inline FriPlan fri_plan(unsigned log_n, unsigned log_arity, unsigned num_folds) {
  std::vector<uint64_t> o(8 + 5 * ((size_t)num_folds + 1));
  check(ark_hip_fri_plan(SFIELD_ID, log_n, log_arity, num_folds, o.data()), "ark_hip_fri_plan");
  FriPlan p{(unsigned)o[0], o[2], o[3], o[4], o[5], o[6], {}};
  for (size_t l = 0; l < o[1]; l++)
    p.layers.push_back(FriLayer{(unsigned)o[8 + 5 * l], (unsigned)o[9 + 5 * l], o[10 + 5 * l], o[11 + 5 * l], (unsigned)o[12 + 5 * l]});
  return p;
}
template <int SFIELD_ID>
inline ark_hip_sfp_radix2_domain fri_folded_domain(const ark_hip_sfp_radix2_domain& dom, unsigned log_arity) {
  ark_hip_sfp_radix2_domain out;
  check(ark_hip_fri_folded_domain(SFIELD_ID, &dom, log_arity, &out), "ark_hip_fri_folded_domain");
  return out;
}
// the fold of one opened row: row[k * 2^a + j] = component k of f[index + j n / 2^a]
template <int SFIELD_ID>
inline ExtElement fri_fold_row(const ark_hip_sfp_radix2_domain& dom, unsigned log_arity, uint64_t index, const std::vector<uint64_t>& row,
                               const ExtElement& beta) {
  if (row.size() != ((size_t)small_ext_degree<SFIELD_ID>() << log_arity)) throw Error(ARK_HIP_ERR_ARG, "a row holds d * 2^log_arity words");
  ExtElement r;
  check(ark_hip_fri_fold_row(SFIELD_ID, &dom, log_arity, index, row.data(), beta.data(), r.data()), "ark_hip_fri_fold_row");
  return r;
}
template <int SFIELD_ID>
inline SmallExtVec<SFIELD_ID> fri_fold(const SmallExtVec<SFIELD_ID>& f, const SmallRadix2EvaluationDomain<SFIELD_ID>& dom, unsigned log_arity,
                                       const ExtElement& beta) {
  if (f.len() != dom.size()) throw Error(ARK_HIP_ERR_ARG, "one evaluation per element of the domain");
  SmallExtVec<SFIELD_ID> out(f.len() >> log_arity);
  check(ark_hip_fri_fold(SFIELD_ID, &dom.raw(), log_arity, beta.data(), f.device_ptr(), f.stride(), out.device_ptr(), out.stride()),
        "ark_hip_fri_fold");
  return out;
}

// The commit phase over a compact SmallExtVec of dom.size() evaluations (layer 0, never written; it must outlive the prover).
template <int SFIELD_ID>
class FriProver {
 public:
  using Word = typename SmallWord<SFIELD_ID>::type;
  static constexpr unsigned D = small_ext_degree<SFIELD_ID>();
  // the challenge of a layer from its root
  struct Challenger {
    virtual ExtElement next_beta(const Digest& root) = 0;
    virtual ~Challenger() = default;
  };
  FriProver(const SmallExtVec<SFIELD_ID>& layer0, const SmallRadix2EvaluationDomain<SFIELD_ID>& dom, unsigned log_arity, unsigned num_folds)
      : layer0_(&layer0), dom_(dom.raw()), log_arity_(log_arity), num_folds_(num_folds),
        plan_(fri_plan<SFIELD_ID>(dom.log_size_of_group(), log_arity, num_folds)) {
    if (layer0.len() != dom.size() || layer0.stride() != layer0.len()) throw Error(ARK_HIP_ERR_ARG, "layer 0 is compact and fills the domain");
    check(ark_hip_malloc(plan_.layer_words * sizeof(Word), &layers_), "ark_hip_malloc");
    check(ark_hip_malloc(plan_.tree_bytes ? plan_.tree_bytes : 16, &trees_), "ark_hip_malloc");
  }
  FriProver(const FriProver&) = delete;
  FriProver& operator=(const FriProver&) = delete;
  ~FriProver() {
    if (layers_) (void)ark_hip_free(layers_);
    if (trees_) (void)ark_hip_free(trees_);
  }
  const FriPlan& plan() const { return plan_; }
  // fills roots(), betas() and final_poly() (d * size stored coefficient words of the last layer, component by component)
  void commit_phase(Challenger& ch) {
    State st{&ch, &betas_};
    betas_.clear();
    roots_.assign(num_folds_, Digest{});
    final_.assign((size_t)D * plan_.final_size, 0);
    check(ark_hip_fri_commit_phase(SFIELD_ID, &dom_, log_arity_, num_folds_, layer0_->device_ptr(), layers_, trees_, &FriProver::trampoline, &st,
                                   num_folds_ ? roots_[0].data() : nullptr, final_.data()), "ark_hip_fri_commit_phase");
  }
  const std::vector<Digest>& roots() const { return roots_; }
  const std::vector<ExtElement>& betas() const { return betas_; }
  const std::vector<Word>& final_poly() const { return final_; }
  const void* layer_ptr(unsigned l) const {
    return l == 0 ? layer0_->device_ptr() : (const void*)((const char*)layers_ + plan_.layers[l].layer_offset * sizeof(Word));
  }
  // per layer l < num_folds: the rows (d * 2^a words each) and paths of index mod rows, one opening per index
  std::vector<MerkleTree::Opening> query(std::vector<uint64_t> indices) const {
    std::vector<MerkleTree::Opening> out;
    for (unsigned l = 0; l < num_folds_; l++) {
      const FriLayer& lay = plan_.layers[l];
      const size_t rows = (size_t)1 << (lay.log_size - lay.log_arity), count = (size_t)D << lay.log_arity;
      for (auto& i : indices) i %= rows;
      MerkleTree::Opening o;
      o.paths.resize(indices.size() * (lay.log_size - lay.log_arity) * ARK_HIP_MERKLE_DIGEST_BYTES);
      o.rows.resize(indices.size() * count * sizeof(Word));
      check(ark_hip_merkle_open_device((const char*)trees_ + lay.tree_offset, rows, layer_ptr(l), sizeof(Word), count, rows, indices.data(),
                                       indices.size(), o.rows.data(), o.paths.data()), "ark_hip_merkle_open_device");
      out.push_back(std::move(o));
    }
    return out;
  }

 private:
  struct State { Challenger* ch; std::vector<ExtElement>* betas; };
  static int trampoline(void* user, const uint8_t root[32], uint64_t beta_out[4]) {
    State* st = (State*)user;
    Digest d;
    std::memcpy(d.data(), root, d.size());
    const ExtElement b = st->ch->next_beta(d);
    st->betas->push_back(b);
    std::memcpy(beta_out, b.data(), sizeof(uint64_t) * 4);
    return 0;
  }
  const SmallExtVec<SFIELD_ID>* layer0_;
  ark_hip_sfp_radix2_domain dom_;
  unsigned log_arity_, num_folds_;
  FriPlan plan_;
  void* layers_ = nullptr;
  void* trees_ = nullptr;
  std::vector<Digest> roots_;
  std::vector<ExtElement> betas_;
  std::vector<Word> final_;
};

// One query of a commit phase, on the host: rows[l] / paths[l] open row (position mod rows) of layer l.  Every row must open
// against its root and carry the value the previous fold produced; the last fold must equal the final polynomial at its point.
template <int SFIELD_ID>
inline bool fri_verify_query(const ark_hip_sfp_radix2_domain& dom, unsigned log_arity, const std::vector<Digest>& roots,
                             const std::vector<ExtElement>& betas, const std::vector<typename SmallWord<SFIELD_ID>::type>& final_poly,
                             uint64_t index, const std::vector<std::vector<typename SmallWord<SFIELD_ID>::type>>& rows,
                             const std::vector<std::vector<uint8_t>>& paths) {
  constexpr unsigned D = small_ext_degree<SFIELD_ID>();
  const unsigned num_folds = (unsigned)roots.size();
  const FriPlan plan = fri_plan<SFIELD_ID>(dom.log_size_of_group, log_arity, num_folds);
  const uint64_t p = small_field_info<SFIELD_ID>().p;
  if (betas.size() != num_folds || rows.size() != num_folds || paths.size() != num_folds || final_poly.size() != D * plan.final_size) return false;
  ark_hip_sfp_radix2_domain cur = dom;
  uint64_t pos = index % dom.size;
  ExtElement value{};
  bool have = false;
  for (unsigned l = 0; l < num_folds; l++) {
    const unsigned a = plan.layers[l].log_arity;
    const uint64_t m = (uint64_t)1 << (plan.layers[l].log_size - a), r = pos % m, j = pos / m;
    if (rows[l].size() != ((size_t)D << a) || paths[l].size() != (size_t)(plan.layers[l].log_size - a) * ARK_HIP_MERKLE_DIGEST_BYTES) return false;
    if (!MerkleTree::verify_small<SFIELD_ID>(roots[l], m, r, rows[l].data(), rows[l].size(), paths[l].data())) return false;
    std::vector<uint64_t> row(rows[l].begin(), rows[l].end());
    for (uint64_t w : row)
      if (w >= p) return false;
    if (have)
      for (unsigned k = 0; k < D; k++)
        if (row[((size_t)k << a) + j] != value[k]) return false;
    value = fri_fold_row<SFIELD_ID>(cur, a, r, row, betas[l]);
    have = true;
    cur = fri_folded_domain<SFIELD_ID>(cur, a);
    pos = r;
  }
  if (!have) return true;
  const ExtElement x = ext_mul<SFIELD_ID>(ExtElement{cur.offset, 0, 0, 0}, ExtElement{small_field_pow<SFIELD_ID>(cur.group_gen, pos), 0, 0, 0});
  ExtElement acc{};
  for (size_t i = plan.final_size; i-- > 0;) {   // Horner on every component: x lies in the base field
    acc = ext_mul<SFIELD_ID>(acc, x);
    for (unsigned k = 0; k < D; k++) {
      const unsigned __int128 s = (unsigned __int128)acc[k] + final_poly[k * plan.final_size + i];
      acc[k] = (uint64_t)(s % p);
    }
  }
  return acc == value;
}

}  // namespace ark_hip
