/*
 * ark_hip.h -- C ABI of libark_hip.so: MI355X (gfx950) implementation of the one data-parallel hot
 * path of arkworks-rs/algebra:
 *     ark_ec::VariableBaseMSM::msm over short-Weierstrass G1/G2   (Pippenger bucket method)
 *     ark_poly::Radix2EvaluationDomain::{fft,ifft}_in_place over Fr (Cooley-Tukey radix-2)
 * Every entry point below is what the reference's Rust side would bind through FFI; the
 * reference item each one replaces is cited (paths relative to the arkworks-rs/algebra tree).
 * INTEGRATION.md shows the Rust `extern "C"` block and the trait impls that call them.
 *
 * Data layout == the reference's in-memory layout, no conversion on either side:
 *   Fp           N little-endian u64 limbs, Montgomery form, value < p   (ff/src/biginteger/mod.rs:34,
 *                                                                          ff/src/fields/models/fp/mod.rs:109-115)
 *   Fp2          c0 | c1                                                  (quadratic_extension.rs:100-106)
 *   Affine       x | y, identity = all-zero (ZeroFlag = ())               (short_weierstrass/affine.rs:30-37,91-104)
 *   Projective   x | y | z Jacobian, identity = (R, R, 0)                 (short_weierstrass/group.rs:34-41,145-151)
 *   scalar       4 u64 limbs: BigInt<4> canonical, or Fr Montgomery
 * All functions return 0 on success and a negative code on error; none throws or aborts.
 * Devices and threads: the library keeps one context (streams, workspaces) per GPU.  A call runs on the
 * calling thread's current device (ark_hip_set_device; default: the first device initialised in the process)
 * and holds that context's lock for its whole body, so any number of host threads (rayon workers) may call
 * concurrently: calls on one GPU serialise, calls on different GPUs overlap.  One process per GPU
 * (torch.distributed / RCCL) and one process driving all GPUs (ark_hip_msm_sw_multi) are both supported.
 * Limits: MSM n < 2^31 and n * windows < 2^32 (n <= 2^28 for 255-bit scalars; 2^28 is tested); FFT log2(size) <= 30.
 * Environment: ARK_HIP_WAIT=block makes an MSM wait for the GPU with a blocking hipEventSynchronize; by default the
 * calling thread polls the completion event (the MSM is on its caller's critical path; a sleeping thread was measured
 * to add up to 1 ms per call on some hosts).  ARK_HIP_MSM_C / ARK_HIP_MSM_C_PREPARED force the window size (tuning).
 * ARK_HIP_HOST_TAIL_THREADS=k (default 7; 0: none): size of the ONE process-wide pool of parked helper threads that shares
 * the short host-side tails with the calling thread -- the windows' own sums of a short MSM's tail, the verified cache's hashing
 * pass.  Created on first use, never per call; see ark_hip_host_threads.
 * ARK_HIP_COPY_THREADS=n (default 0 = the HIP runtime's own pageable path): n worker threads stage uploads from ordinary
 * host memory through page-locked buffers.  ARK_HIP_STREAM_PIECES: pieces a host-scalar MSM is cut into (default
 * n / 2^18, at most 8).  ARK_HIP_BASE_CACHE_MB / ARK_HIP_AUTO_PREPARE: see ark_hip_msm_cache_config.
 */
#ifndef ARK_HIP_H
#define ARK_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared between this push and the pop below are its
 * dynamic symbols. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* field ids */
enum { ARK_HIP_BN254_FQ = 0, ARK_HIP_BN254_FR = 1, ARK_HIP_BLS12_381_FQ = 2, ARK_HIP_BLS12_381_FR = 3,
       ARK_HIP_BLS12_377_FQ = 4, ARK_HIP_BLS12_377_FR = 5 };
/* curve ids (SWCurveConfig instances) */
enum { ARK_HIP_BN254_G1 = 0, ARK_HIP_BLS12_381_G1 = 1, ARK_HIP_BLS12_377_G1 = 2, ARK_HIP_BLS12_377_G2 = 3,
       ARK_HIP_BLS12_381_G2 = 4 };
/* error codes */
enum { ARK_HIP_OK = 0, ARK_HIP_ERR_ARG = -1, ARK_HIP_ERR_SIZE = -2, ARK_HIP_ERR_NOMEM = -3,
       ARK_HIP_ERR_SCALAR_RANGE = -4, ARK_HIP_ERR_NO_DEVICE = -5, ARK_HIP_ERR_BUSY = -6,
       ARK_HIP_ERR_COMM = -7 /* RCCL missing or failed */ /* HIP runtime errors: <= -1000 */ };

/* ---- runtime ---- */
int ark_hip_device_count(void);
/* Make GPU `device` the calling thread's current device and create its context (streams, workspaces) if needed.
 * The first device initialised becomes the default of threads that never choose one.  Idempotent.
 * (ARK_HIP_OVERSUBSCRIBE=1 in the environment lets ids beyond the physical count wrap around -- separate contexts
 * on a shared GPU -- so that multi-device code can be exercised on a one-GPU box.) */
int ark_hip_init(int device);
int ark_hip_set_device(int device);   /* same as ark_hip_init */
int ark_hip_get_device(void);
/* Destroys every context (waits for calls in flight). */
void ark_hip_shutdown(void);
/* Waits for everything enqueued on the current device's streams. */
int ark_hip_synchronize(void);
const char* ark_hip_version(void);
/* Host threads the library keeps: out[0] = helper threads of the process-wide pool that shares the short host-side tails
 * (the windows' sums of an MSM's tail, the verified cache's hashing pass) with the calling thread -- created once, on first
 * use, parked while idle; ARK_HIP_HOST_TAIL_THREADS (default 7, 0: none) and the cores the process may use bound it;
 * out[1] = threads that pool has created since the process started (stays at out[0]: no thread is created per call).
 * Callable without a GPU. */
int ark_hip_host_threads(int out[2]);
/* u64 words per base-field element (4, 6 or 12), scalar field id, base field id, extension degree */
int ark_hip_curve_info(int curve, int* fe_words, int* scalar_field, int* base_field, int* ext_degree);

/* Device memory for hosts that have no HIP binding of their own: upload a fixed base set (an SRS) once with
 * ark_hip_malloc + ark_hip_memcpy_h2d and pass the device pointer to ark_hip_msm_sw_device for every proof. */
int ark_hip_malloc(size_t bytes, void** out_dptr);
int ark_hip_free(void* dptr);
int ark_hip_memcpy_h2d(void* dst_dptr, const void* src_host, size_t bytes);
int ark_hip_memcpy_d2h(void* dst_host, const void* src_dptr, size_t bytes);
/* device-to-device copy and byte fill, asynchronous on the context stream (ordered with every *_device entry) */
int ark_hip_memcpy_d2d(void* dst_dptr, const void* src_dptr, size_t bytes);
int ark_hip_memset_device(void* dptr, int value, size_t bytes);
/* Page-locked host memory: scalar vectors produced into it upload at full PCIe rate and truly asynchronously
 * (ark_hip_msm_prepared_async). */
int ark_hip_host_alloc(size_t bytes, void** out_ptr);
int ark_hip_host_free(void* ptr);

/* SWCurveConfig::GENERATOR (e.g. curves/bls12_381/src/curves/g1.rs:199-205) as Affine limbs */
int ark_hip_curve_generator(int curve, uint64_t* out_xy);

/* ---- MSM ----
 * Replaces SWCurveConfig::msm (ec/src/models/short_weierstrass/mod.rs:112-119) -> 
 * VariableBaseMSM::msm_unchecked / msm_bigint (ec/src/scalar_mul/variable_base/mod.rs:59-85).
 * bases: n Affine points; scalars: n x 4 limbs; scalars_are_montgomery != 0 for the `msm(&[Fr])`
 * entry (the into_bigint pass of mod.rs:60-62 then runs on the device), 0 for `msm_bigint`.
 * The length check (Err(min_len), mod.rs:73-77) stays on the caller's side: one n here.
 * out_xyz: Projective.  Bases must lie in the prime-order subgroup (as Affine deserialisation guarantees; the
 * reference's own msm_signed relies on r*P = O as well, mod.rs:251-285).  Scalars: any BigInt<4> below
 * 2^MODULUS_BIT_SIZE is accepted and gives the reference's result (values in [r, 2^bits) are reduced once);
 * a scalar with higher bits set returns ARK_HIP_ERR_SCALAR_RANGE -- the reference's make_digits (mod.rs:754-794)
 * silently drops bits above ceil(bits/c)*c there, i.e. its result depends on the window size it happened to pick. */
int ark_hip_msm_sw(int curve, const uint64_t* bases, const uint64_t* scalars, size_t n, int scalars_are_montgomery,
                   uint64_t* out_xyz);
/* ark_hip_msm_sw is a FUNCTION OF ITS TWO SLICES, like the reference (`bases: &[Affine]` is borrowed for the call,
 * variable_base/mod.rs:59-85): whatever the library keeps between calls never changes a result.  Provers hand the SAME
 * base slice -- an SRS -- to call after call (bench-templates/src/macros/ec.rs:223-240 does exactly that), so device
 * copies of base slices are kept in two ways:
 *
 * Verified cache (on by default).  Device copies keyed by (curve, host address, length), validated on EVERY call by a
 * keyed 128-bit hash of the slice's FULL content: host threads (ARK_HIP_HASH_THREADS, default 8) hash the slice while the device already
 * works from the cached copy, and the result is returned only if the hash equals that of the content the copy was filled
 * from -- otherwise the copy is refreshed and the MSM rerun.  An in-place edit of the slice, of a single limb, is therefore
 * honoured on the next call; a hit costs one pass over the host slice instead of its PCIe transfer (2^24 BLS12-381 G1:
 * 40 ms per call against 48 ms streamed).  A slice that does not fit the budget streams over PCIe with its scalars, piece
 * k+1 under piece k's kernels.  Least-recently-used sets (with their tables) are dropped beyond the budget.
 *   ark_hip_msm_cache_config(budget_bytes, auto_prepare_after): budget -1 keeps the current value, -2 restores the
 *     default (16 GiB, at most a quarter of the device memory; ARK_HIP_BASE_CACHE_MB raises or lowers it), 0 disables and empties the cache (every call
 *     then streams bases and scalars and nothing is retained); auto_prepare_after = K > 0 builds the per-window table of a
 *     resident set -- pinned or cached -- once the WHOLE set has been the operand K times (default 0 = never, or
 *     ARK_HIP_AUTO_PREPARE; a cached set's table counts against the budget), < 0 keeps the current value.
 *   ark_hip_msm_cache_clear: drops the cached sets (pinned sets stay).
 *   ark_hip_msm_cache_stats: [cached sets, their device bytes, hits, misses, refreshed (content changed), evicted,
 *     pinned sets, pinned hits].
 *
 * Pinned base sets (no host pass at all).  ark_hip_msm_bases_pin(curve, bases, n) uploads the set now and declares
 * bases[0 .. n) IMMUTABLE until the matching ark_hip_msm_bases_unpin(curve, bases, n).  Every ark_hip_msm_sw /
 * ark_hip_msm_sw_small call on this device whose base slice lies inside a pinned range (at a point boundary: the whole set,
 * msm_unchecked's truncation, the steps of msm_chunks / ChunkedPippenger) runs against the resident copy and uploads only
 * its scalars -- no validation, the declaration is the contract (the Rust guard ark_hip::msm::ResidentBases holds the
 * shared borrow for the pin's lifetime, so the compiler enforces it).  Pins of the same (curve, address, n) nest; pinned
 * sets are outside the cache's budget.  ARK_HIP_ERR_NOMEM if the copy does not fit, ARK_HIP_ERR_ARG for an unpin without
 * a pin. */
int ark_hip_msm_bases_pin(int curve, const uint64_t* bases, size_t n);
int ark_hip_msm_bases_unpin(int curve, const uint64_t* bases, size_t n);
int ark_hip_msm_cache_config(long long budget_bytes, int auto_prepare_after);
int ark_hip_msm_cache_clear(void);
int ark_hip_msm_cache_stats(uint64_t out[8]);
/* The validation pass of the verified cache (round 5): a keyed 128-bit universal hash (NH with 64-bit words under a key
 * drawn from the OS once per process -- two different slices of one length collide with probability <= 2^-63 over the key,
 * and nothing in the source predicts it).  The pass is timed on every call; while its predicted duration exceeds what
 * streaming the slice over PCIe took when the copy was filled (a host whose cores are saturated by the caller's own thread
 * pool), calls stream instead and every eighth call hashes again.  out: [0] calls streamed for that reason, [1] the
 * latest pass in microseconds, [2] its smoothed rate in MB/s, [3] host threads per pass (ARK_HIP_HASH_THREADS). */
int ark_hip_msm_cache_hash_stats(uint64_t out[4]);
/* VariableBaseMSM::msm_u1 / msm_u8 / msm_u16 / msm_u32 / msm_u64 (variable_base/mod.rs:87-117; CPU bodies msm_binary /
 * msm_u8.. :373-434): scalars are n unsigned integers of scalar_bytes (1, 2, 4 or 8) bytes -- exactly the reference's
 * &[bool] (one byte each, max_bits = 1), &[u8], &[u16], &[u32], &[u64] -- whose low max_bits bits may be set (0 = all
 * 8 * scalar_bytes).  Only the ceil((max_bits + 1) / c) windows such scalars reach are built: nothing is widened to 32
 * bytes (a u8 vector uploads 1/32 of what msm_bigint would) and no empty window is sorted.  The host-pointer form shares
 * ark_hip_msm_sw's
 * pinned sets and verified cache (on by default). */
int ark_hip_msm_sw_small(int curve, const uint64_t* bases, const void* scalars, size_t n, int scalar_bytes, int max_bits,
                         uint64_t* out_xyz);
int ark_hip_msm_sw_small_device(int curve, const void* d_bases, const void* d_scalars, size_t n, int scalar_bytes,
                                int max_bits, uint64_t* out_xyz);
/* Same with bases/scalars already in this GPU's memory (device pointers); out_xyz is a host pointer.
 * Scalar widths: msm_signed (variable_base/mod.rs:242-347) sorts the scalars into width classes (+-u1, +-u8, +-u16,
 * +-u32, +-u64, the rest) and runs one MSM per class.  This entry runs ONE pipeline and plans it from the same classes:
 * from 2^19 pairs, with nothing else of the context in flight, a probe measures the bit length of min(s, r - s) over a
 * sample of 4096 scalars and -- unless they look uniform -- over all of them (one 40-byte read-back), and the window size and
 * the number of windows follow the digits the scalars really have.  The result is the same group element either way;
 * ARK_HIP_MSM_PROBE=0 plans every call for n uniform full-width scalars.  A prepared base set whose scalars turn out no wider
 * than 48 bits runs this plain pipeline on row 0 of its table (the bases themselves).  The host-pointer entry above estimates the
 * classes from about 1024 of the host scalars and takes only the window size from them. */
int ark_hip_msm_sw_device(int curve, const void* d_bases, const void* d_scalars, size_t n, int scalars_are_montgomery,
                          uint64_t* out_xyz);
/* Asynchronous form: the device work is enqueued and the call returns; ark_hip_msm_wait blocks until the result is
 * there, finishes it (window combine, a few hundred point operations on the host) and frees the job.  Up to 4 jobs
 * may be in flight per device: an *_async entry reports ARK_HIP_ERR_BUSY beyond that, while the SYNCHRONOUS entries
 * (ark_hip_msm_sw, _sw_device, _sw_small(_device), _prepared(_device), _prepared_small_device, _sw_chunks) wait for a slot
 * -- they may be called from any number of host threads at once (the reference's callers are rayon pools) and never
 * return BUSY.  Inputs must stay valid until the wait returns.
 * With a job already in flight the next one runs on the device's second MSM lane (own stream and workspace): its
 * digits / sort / reduction overlap the first job's accumulate kernel (two jobs in flight: +20 % MSMs/s at 2^20, +5 % at
 * 2^24).  Synchronous calls from one thread never use (or allocate) the second lane.
 * The *_async entries never wait for device work already queued (a transform producing the scalars, an earlier job): the
 * width probe of the synchronous entries (one 40-byte read-back that plans narrow / skewed scalar vectors) is skipped
 * here, and the plan is the one for n uniform full-width scalars -- correct for any input, optimal for those. */
typedef struct ark_hip_msm_job ark_hip_msm_job;
int ark_hip_msm_sw_device_async(int curve, const void* d_bases, const void* d_scalars, size_t n,
                                int scalars_are_montgomery, ark_hip_msm_job** out_job);
int ark_hip_msm_wait(ark_hip_msm_job* job, uint64_t* out_xyz);

/* ---- prepared base sets ----
 * Provers run many MSMs against ONE fixed base set (an SRS).  ark_hip_msm_bases_prepare uploads it once and
 * precomputes, for every window w of the digit decomposition, the multiples 2^(offset_w) * P_i (288 GB of HBM pay for
 * the W-fold table: 18 GiB for 2^24 BLS12-381 G1 points).  All windows then share one bucket set, which allows wider
 * windows -- fewer mixed additions per scalar -- and shrinks the bucket reduction W-fold.  Role in the reference: the
 * `bases: &[Affine]` argument of VariableBaseMSM::msm (variable_base/mod.rs:59-85) held by the caller across calls;
 * the precomputation itself is the fixed-base idea of BatchMulPreprocessing (scalar_mul/mod.rs:156-245) applied per base.
 * ark_hip_msm_prepared* compute sum_i s_i * P_i over the first n <= n_bases pairs (msm_unchecked's truncation). */
typedef struct ark_hip_msm_bases ark_hip_msm_bases;
int ark_hip_msm_bases_prepare(int curve, const uint64_t* bases, size_t n, ark_hip_msm_bases** out);
int ark_hip_msm_bases_prepare_device(int curve, const void* d_bases, size_t n, ark_hip_msm_bases** out);
int ark_hip_msm_bases_free(ark_hip_msm_bases* bases);
int ark_hip_msm_bases_info(const ark_hip_msm_bases* bases, size_t* n, int* window_bits, int* windows, size_t* table_bytes);
int ark_hip_msm_prepared(const ark_hip_msm_bases* bases, const uint64_t* scalars, size_t n, int scalars_are_montgomery,
                         uint64_t* out_xyz);
int ark_hip_msm_prepared_device(const ark_hip_msm_bases* bases, const void* d_scalars, size_t n,
                                int scalars_are_montgomery, uint64_t* out_xyz);
/* Narrow scalars (ark_hip_msm_sw_small's scalar_bytes / max_bits) against a prepared base set: runs as a plain MSM over
 * the base set itself (row 0 of the table) with a window plan for the narrow scalars. */
int ark_hip_msm_prepared_small_device(const ark_hip_msm_bases* bases, const void* d_scalars, size_t n, int scalar_bytes,
                                      int max_bits, uint64_t* out_xyz);
/* Asynchronous forms.  The host-scalar one uploads through a two-slot ring on a copy stream: the upload of MSM k+1's
 * scalars overlaps MSM k's kernels. */
int ark_hip_msm_prepared_async(const ark_hip_msm_bases* bases, const uint64_t* scalars, size_t n,
                               int scalars_are_montgomery, ark_hip_msm_job** out_job);
int ark_hip_msm_prepared_device_async(const ark_hip_msm_bases* bases, const void* d_scalars, size_t n,
                                      int scalars_are_montgomery, ark_hip_msm_job** out_job);

/* VariableBaseMSM::msm_chunks (variable_base/mod.rs:119-150): Fr (Montgomery) scalars; the streams are aligned at
 * their end (the first n_bases - n_scalars bases are skipped); steps of `step` pairs (0 = the reference's 2^20), each
 * one msm_bigint, results added.  Step k+1 uploads while step k computes. */
int ark_hip_msm_sw_chunks(int curve, const uint64_t* bases, size_t n_bases, const uint64_t* scalars, size_t n_scalars,
                          size_t step, uint64_t* out_xyz);

/* One MSM across n_gpus GPUs driven from this process: base-range shards (the reference's own split,
 * variable_base/mod.rs:521-557), one host thread + context per device, partial results summed on the host.
 * _multi: host inputs, split evenly; _multi_device: shard g already resident on GPU g (n_per_gpu[g] pairs). */
int ark_hip_msm_sw_multi(int curve, int n_gpus, const uint64_t* bases, const uint64_t* scalars, size_t n,
                         int scalars_are_montgomery, uint64_t* out_xyz);
int ark_hip_msm_sw_multi_device(int curve, int n_gpus, const void* const* d_bases, const void* const* d_scalars,
                                const size_t* n_per_gpu, int scalars_are_montgomery, uint64_t* out_xyz);
/* The same over PREPARED shards: shards[g] was prepared on GPU g (ark_hip_set_device(g); ark_hip_msm_bases_prepare over
 * the g-th base range); the scalars are host memory, cut at the shards' sizes in order, uploaded and run on all devices
 * concurrently (the asynchronous prepared entry per device), partial results summed on the host. */
int ark_hip_msm_prepared_multi(int n_gpus, const ark_hip_msm_bases* const* shards, const uint64_t* scalars, size_t n,
                               int scalars_are_montgomery, uint64_t* out_xyz);

/* The window plan (widest window in bits, number of windows) the library picks for an MSM of n pairs on `curve`, plain
 * (prepared = 0) or over a prepared base set; pure host arithmetic. */
int ark_hip_msm_plan(int curve, size_t n, int prepared, int* window_bits, int* windows);
/* The plan of a plain msm_bigint whose n scalars fall into the given width classes of b = bits(min(s, r - s)) -- counts[k]
 * scalars with TOP[k-1] < b <= TOP[k], TOP = {0, 1, 8, 16, 32, 64, 128, 192, 256} (msm_signed's partition, mod.rs:251-285,
 * with two classes above u64) -- and whose widest has max_bits: what ark_hip_msm_sw_device does after its probe.  Host
 * arithmetic only. */
int ark_hip_msm_plan_widths(int curve, size_t n, uint32_t max_bits, const uint32_t counts[9], int* window_bits, int* windows);
/* Per-phase device times of the last MSM finished on this device with timing enabled (ms):
 * [digits, partition histogram + scan, partition scatter + finish + bucket order, accumulate (incl. heavy
 *  buckets), reduce, total, window_bits, windows] */
int ark_hip_msm_set_timing(int enable);
int ark_hip_msm_last_timing(double out[8]);

/* ---- fixed-base batch multiplication ----
 * ScalarMul::batch_mul / BatchMulPreprocessing (ec/src/scalar_mul/mod.rs:104-251): out[i] = v[i] * g for ONE group element
 * g, results affine (the reference's Vec<MulBase>).  table_new = BatchMulPreprocessing::new(base, num_scalars): builds the
 * table of multiples on the device (base_xyz: Projective; num_scalars sizes the table as in the reference, :222-228, by
 * the device's own cost rule: 12-bit rows, 16-bit rows from 2^24 scalars -- the window never changes a result);
 * batch_mul = BatchMulPreprocessing::batch_mul.  Scalars: n x 4 limbs, Fr (Montgomery) when
 * scalars_are_montgomery != 0 as in the reference, or canonical BigInt<4> (any 256-bit value is multiplied exactly). */
typedef struct ark_hip_batch_mul_table ark_hip_batch_mul_table;
int ark_hip_batch_mul_table_new(int curve, const uint64_t* base_xyz, size_t num_scalars, ark_hip_batch_mul_table** out);
int ark_hip_batch_mul_table_free(ark_hip_batch_mul_table* table);
int ark_hip_batch_mul(const ark_hip_batch_mul_table* table, const uint64_t* scalars, size_t n, int scalars_are_montgomery,
                      uint64_t* out_xy);
int ark_hip_batch_mul_device(const ark_hip_batch_mul_table* table, const void* d_scalars, size_t n,
                             int scalars_are_montgomery, void* d_out_xy);

/* ---- host-side group helpers (run on the CPU; tiny) ----
 * Sum of n Projective points: the multi-GPU combine of per-rank partial MSMs (the reference's
 * chunk sum, ec/src/scalar_mul/variable_base/mod.rs:542-557).  The reduction operator is
 * elliptic-curve addition, so it cannot be an RCCL sum: ranks all-gather 3 field elements each. */
int ark_hip_sw_sum(int curve, const uint64_t* jac_points, size_t n, uint64_t* out_xyz);
/* From<Projective> for Affine (ec/src/models/short_weierstrass/affine.rs:374-396): the unique
 * representative the reference's assert_eq! compares; identity -> (0, 0). */
int ark_hip_sw_into_affine(int curve, const uint64_t* jac_points, size_t n, uint64_t* out_xy);

/* out[i] = in[i] + delta for n affine points in device memory (affine result, one inversion per
 * point; d_in may equal d_out).  Used to grow synthetic base sets P_i = (a + i*b)G on the device
 * (bench.py / tests); mathematically Affine + Affine -> into_affine (group.rs:332-413, affine.rs:374-396). */
int ark_hip_sw_add_affine_device(int curve, const void* d_in, void* d_out, size_t n, const uint64_t* delta_xy);

/* CurveGroup::normalize_batch (ec/src/models/short_weierstrass/group.rs:302-319) for n Projective points in
 * device memory -> n Affine points in device memory; identity -> (0, 0). */
int ark_hip_sw_normalize_batch_device(int curve, const void* d_jac, void* d_out_xy, size_t n);
/* the same from host memory: n Projective in, n Affine out (the Rust hook behind CurveGroup::normalize_batch) */
int ark_hip_sw_normalize_batch(int curve, const uint64_t* jac_points, size_t n, uint64_t* out_xy);

/* ---- base-set validation: what establishes the MSM entries' precondition on the device ----
 * The reference runs two predicates when it deserialises a point: Affine::is_on_curve (ec/src/models/short_weierstrass/
 * affine.rs:146-157) and SWCurveConfig::is_in_correct_subgroup_assuming_on_curve (short_weierstrass/mod.rs:82-90; overrides:
 * curves/bn254/src/curves/g1.rs:59, bls12_381 g1.rs:69-85, g2.rs:75).  These entries run them over n Affine points (x | y,
 * Montgomery form, identity = (0, 0)) where the points live.  Per point a status, the first stage that fails:
 *   0  passed every requested stage
 *   1  a coordinate is not a field element (an Fp component, read as an integer, is >= p).  Nothing can be computed for such
 *      a point, so this stage runs under every mask.
 *   2  not on the curve (y^2 != x^3 + b); the identity passes
 *   3  on the curve (or assumed to be) but [r]P != O
 * checks: bit 0 (1) = the curve equation, bit 1 (2) = the subgroup test; with both, the subgroup test runs only for points that
 *   passed the equation; with bit 1 alone it is "assuming on curve", as in the reference.  BN254 G1 has cofactor one: its
 *   subgroup test is the constant true.
 * method: 1 = double-and-add over the bits of r on the exact mixed addition (the reference's default; every curve);
 *   2 = phi(P) == -[x^2]P with phi(x, y) = (beta x, y) (Scott, eprint 2021/1130 section 6; bls12_381 g1.rs:69-85): BLS12-381 G1
 *   only, ARK_HIP_ERR_ARG elsewhere; 0 = auto: method 2 on BLS12-381 G1 (the faster one there), method 1 elsewhere.  The
 *   status does not depend on the method.
 * d_status / status: n bytes, or NULL.  out[0] = smallest index with a non-zero status (n if none), out[1..3] = number of points
 * with status 1, 2, 3.  n = 0 gives out = {0, 0, 0, 0}.  The input is not modified.  ARK_HIP_ERR_ARG for a bad curve / checks /
 * method or a null pointer, before any device is touched.  Both entries synchronise before they return. */
int ark_hip_sw_check_device(int curve, const void* d_bases_xy, size_t n, int checks, int method, void* d_status, uint64_t out[4]);
/* the same for a host slice: staged upload in chunks, one launch per chunk */
int ark_hip_sw_check(int curve, const uint64_t* bases_xy, size_t n, int checks, int method, uint8_t* status, uint64_t out[4]);

/* ---- compressed points: decompress (+ validate) and compress where the points live ----
 * The reference reads a point with Compress::Yes by taking one square root in the base field per point
 * (Affine::get_ys_from_x_unchecked, ec/src/models/short_weierstrass/affine.rs:129-143) and, with Validate::Yes, the subgroup test
 * above.  These entries do both over n encodings of E = ark_hip_sw_compressed_size(curve) bytes each:
 *   BN254 G1 32, BLS12-377 G1 48, BLS12-377 G2 96: the arkworks form (short_weierstrass/mod.rs:125-193): x little-endian (Fp2:
 *     c0 then c1), bit 7 of the last byte = "take the larger y", bit 6 = infinity.  Both bits: refused.  Every Fp component must be
 *     < p once the two bits are cleared, also with the infinity bit; with it the result is the identity whatever x is.
 *   BLS12-381 G1 48, G2 96: the zcash form (curves/bls12_381/src/curves/util.rs, g1.rs:97-147, g2.rs:124-140): x big-endian (Fp2:
 *     c1 then c0), byte 0: bit 7 = compressed (required), bit 6 = infinity (then every other bit must be zero), bit 5 = larger y.
 *   "Larger": y > -y on canonical residues; over Fp2 c1 decides, c0 if c1 = 0 (quadratic_extension.rs:443-453).
 * Per point a status, the first stage that fails; 0 iff the reference returns Ok, and then the point is the reference's:
 *   1  flags refused or malformed   2  a component is not a field element   3  x^3 + b has no square root
 *   4  [r]P != O (only with validate = 1)
 * A point with a non-zero status is written as the identity (0, 0).  Which SerializationError the reference picks is not mirrored.
 * validate: 0 = Validate::No, 1 = Validate::Yes.  method: as for ark_hip_sw_check (0 auto, 1 ladder over r, 2 endomorphism test,
 *   BLS12-381 G1 only); checked even when validate = 0.
 * d_points_xy / points_xy: n Affine points out (x | y, Montgomery form).  d_status / status: n bytes, or NULL.
 * out[0] = smallest index with a non-zero status (n if none), out[1..4] = number of points with status 1..4; n = 0 gives zeros.
 * ARK_HIP_ERR_ARG before any device is touched: bad curve / validate / method, a null pointer with n > 0, a device pointer that is
 * not 4-byte aligned, d_bytes and d_points_xy overlapping.  Device point arrays are 16-byte aligned, as everywhere in this library.
 * Both decompress entries and ark_hip_sw_compress synchronise before they return; ark_hip_sw_compress_device is asynchronous on
 * the context stream.  The host-slice entries, ark_hip_sw_decompress AND ark_hip_sw_compress, stage in chunks of 64 MiB of points
 * (ARK_HIP_DECOMPRESS_CHUNK_POINTS overrides the chunk length of both, in points).
 * Compress writes the canonical encoding; its precondition is reduced coordinates (what ark_hip_sw_check establishes).
 * The uncompressed form (Compress::No) needs no square root and is not served. */
int ark_hip_sw_compressed_size(int curve);                         /* 32 / 48 / 96; host only, ARK_HIP_ERR_ARG for a bad curve */
int ark_hip_sw_decompress_device(int curve, const void* d_bytes, size_t n, int validate, int method, void* d_points_xy, void* d_status, uint64_t out[5]);
int ark_hip_sw_decompress(int curve, const uint8_t* bytes, size_t n, int validate, int method, uint64_t* points_xy, uint8_t* status, uint64_t out[5]);
int ark_hip_sw_compress_device(int curve, const void* d_points_xy, size_t n, void* d_bytes);
int ark_hip_sw_compress(int curve, const uint64_t* points_xy, size_t n, uint8_t* bytes);

/* ---- point vectors: elementwise scalar multiplication, elementwise sum, two-scalar fold, where the points live ----
 * The reference has no batch form of these: `Projective *= ScalarField` (ec/src/models/short_weierstrass/group.rs:556-570) goes
 * through mul_bigint to SWCurveConfig::mul_projective / mul_affine (short_weierstrass/mod.rs:101-109) and double_and_add(_affine)
 * (ec/src/scalar_mul/mod.rs:29-60), `Projective += / -= Projective` is group.rs:450-538, and callers map them over a vector with
 * rayon.  These entries do that over n points where they live -- one lane per point:
 *   mul   out[i] = [k_i] P_i, with n scalars or ONE scalar shared by every point (n_scalars = 1)
 *   add   out[i] = A_i + B_i, or A_i - B_i with negate_b = 1: the full addition (either side the identity, A = B, A = -B)
 *   fold  out[i] = [a] Lo_i + [b] Hi_i with two shared scalars on ONE joint doubling chain (a round of an inner-product
 *         argument: G' = [u^-1] G_lo + [u] G_hi)
 * form: of the INPUT points.  ARK_HIP_FORM_AFFINE: x | y, identity (0, 0); ARK_HIP_FORM_PROJECTIVE: Jacobian x | y | z, identity
 *   z = 0.  add takes Projective only.  Coordinates are Montgomery residues below p.  The OUTPUT is always Projective; as a group
 *   element it is the reference's, its representative is not (compare after into_affine / normalize_batch).
 * scalars: 4 x u64 each; Montgomery Fr (scalars_are_montgomery = 1) or canonical BigInt<4> (0), and then EVERY 256-bit value is
 *   multiplied exactly, as in ark_hip_batch_mul (mul_bigint semantics: nothing is reduced mod r, so a point outside the
 *   prime-order subgroup gets the multiple asked for).
 * The three G1 curves run on the carry-free limbs of the MSM's accumulate kernels (ARK_HIP_MSM_LAZY=0: on saturated limbs, as
 * the G2 curves always do).  A vector is walked in slabs of at most 2^17 lanes per launch (a launch keeps 8 multiples of each
 * point in context scratch; ARK_HIP_POINTVEC_SLAB_LOG = 6..17 lowers the slab).
 * ARK_HIP_ERR_ARG before any device is looked for: a bad curve / form / flag; n_scalars not 1 or n; a null pointer with n > 0; a
 *   device pointer that is not 16-byte aligned; out overlapping an input.  EXACT aliasing (out == the input pointer) is allowed
 *   where the input is Projective -- a lane reads its element before it writes it; with Affine input the strides differ and any
 *   overlap is refused; out never overlaps the scalars.  n = 0 succeeds and touches nothing.
 * The three _device entries are ASYNCHRONOUS on the context stream (ark_hip_synchronize, or any synchronising entry such as
 * ark_hip_memcpy_d2h, waits for them); a and b of the fold are read before the call returns.  ark_hip_sw_mul (host slices)
 * stages points and scalars in chunks of 64 MiB of points (ARK_HIP_POINTVEC_CHUNK_POINTS overrides the chunk length, in
 * points) and synchronises before it returns. */
enum { ARK_HIP_FORM_AFFINE = 0, ARK_HIP_FORM_PROJECTIVE = 1 };
int ark_hip_sw_mul_device(int curve, const void* d_points, int form, const void* d_scalars, size_t n_scalars /* 1 or n */,
                          int scalars_are_montgomery, size_t n, void* d_out_xyz);
int ark_hip_sw_mul(int curve, const uint64_t* points, int form, const uint64_t* scalars, size_t n_scalars, int scalars_are_montgomery,
                   size_t n, uint64_t* out_xyz);
int ark_hip_sw_add_device(int curve, const void* d_a_xyz, const void* d_b_xyz, int negate_b, size_t n, void* d_out_xyz);
int ark_hip_sw_fold_device(int curve, const void* d_lo, const void* d_hi, int form, const uint64_t a[4], const uint64_t b[4],
                           int scalars_are_montgomery, size_t n, void* d_out_xyz);

/* ---- Radix-2 evaluation domain ----
 * Mirror of Radix2EvaluationDomain<F>'s public fields (poly/src/domain/radix2/mod.rs:22-42). */
typedef struct {
  uint64_t size;
  uint32_t log_size_of_group;
  uint32_t _pad;
  uint64_t size_as_field_element[4];
  uint64_t size_inv[4];
  uint64_t group_gen[4];
  uint64_t group_gen_inv[4];
  uint64_t offset[4];
  uint64_t offset_inv[4];
  uint64_t offset_pow_size[4];
} ark_hip_radix2_domain;

/* Radix2EvaluationDomain::new (radix2/mod.rs:55-83): size = num_coeffs.next_power_of_two();
 * returns ARK_HIP_ERR_SIZE where the reference returns None (log size > TWO_ADICITY). */
int ark_hip_radix2_domain_new(int field, size_t num_coeffs, ark_hip_radix2_domain* out);
/* get_coset (radix2/mod.rs:85-92); ARK_HIP_ERR_ARG if offset == 0 (reference: None) */
int ark_hip_radix2_domain_get_coset(int field, const ark_hip_radix2_domain* dom, const uint64_t* offset,
                                    ark_hip_radix2_domain* out);
/* fft_in_place / ifft_in_place (radix2/mod.rs:140-153) on exactly dom->size elements (the caller
 * has already done the reference's resize(size, zero)); natural order in and out. */
int ark_hip_fft_in_place(int field, const ark_hip_radix2_domain* dom, uint64_t* data);
int ark_hip_ifft_in_place(int field, const ark_hip_radix2_domain* dom, uint64_t* data);
/* Same on device memory; asynchronous on the context stream (ark_hip_synchronize() to wait). */
int ark_hip_fft_in_place_device(int field, const ark_hip_radix2_domain* dom, void* d_data);
int ark_hip_ifft_in_place_device(int field, const ark_hip_radix2_domain* dom, void* d_data);
/* fft_in_place on a coefficient vector of num_coeffs <= size elements (radix2/mod.rs:140-147): the buffer holds
 * dom->size elements, only the first num_coeffs are read (the rest is treated as zero, as the reference's resize
 * does).  With num_coeffs * 4 <= size this is the degree-aware path (fft.rs:29-71): the first
 * log2(size / next_pow2(num_coeffs)) butterfly stages are skipped and only the coefficients are uploaded. */
int ark_hip_fft_in_place_degree_aware(int field, const ark_hip_radix2_domain* dom, uint64_t* data, size_t num_coeffs);
int ark_hip_fft_in_place_degree_aware_device(int field, const ark_hip_radix2_domain* dom, void* d_data, size_t num_coeffs);
/* `count` independent transforms over one domain (forward, or inverse != 0), each in place on its own device buffer of
 * dom->size elements -- the several polynomials a prover transforms at once.  Up to three run concurrently on the GPU,
 * which fills the vector-ALU slots a single transform leaves idle around its pass boundaries: per transform 2^22
 * 0.53 -> 0.48 ms, 2^20 0.157 -> 0.108 ms, 2^16 44 -> 18 us.  Asynchronous on the context stream like the single call.
 * No counterpart in the reference (its callers loop over fft_in_place, poly/src/domain/mod.rs:92-112). */
int ark_hip_fft_batch_in_place_device(int field, const ark_hip_radix2_domain* dom, void* const* d_data, size_t count,
                                      int inverse);
/* r[i] = a[i] * b[i] over n Fr elements in device memory: `Evaluations *= &Evaluations`
 * (poly/src/evaluations/univariate/mod.rs), the pointwise step between the two FFTs and the IFFT of
 * DensePolynomial multiplication (poly/src/polynomial/univariate/dense.rs:641-656).  Asynchronous. */
int ark_hip_fr_mul_device(int field, const void* d_a, const void* d_b, void* d_r, size_t n);
/* The transform over GROUP elements (round 5): EvaluationDomain::fft_in_place / ifft_in_place for T = Projective<P>
 * (poly/src/domain/mod.rs:332-362, radix2/fft.rs:74-119; the reference's own use: poly/src/test.rs:57 with G1Projective).
 * jac_points: dom->size Jacobian points (x | y | z, the reference's Projective) of `curve`, whose scalar field must be the
 * field the domain was made for; the caller pads with identities (z = 0) to the domain size, as the reference's resize does.
 * Forward: X_j = sum_i [(h g^j)^i] P_i; inverse: P_i = [n^-1 h^-i] sum_j [g^-ij] X_j.  Results are group elements: the
 * Projective representatives differ from the reference's, into_affine() agrees.  The device form is asynchronous. */
int ark_hip_fft_group_in_place(int curve, const ark_hip_radix2_domain* dom, uint64_t* jac_points, int inverse);
int ark_hip_fft_group_in_place_device(int curve, const ark_hip_radix2_domain* dom, void* d_jac_points, int inverse);
/* The rest of the pointwise algebra of device-resident Fr vectors (round 5): Evaluations += / -= / negation
 * (poly/src/evaluations/univariate/mod.rs:104-180) and a vector times ONE field element (dense.rs:604-622; k is a host
 * pointer to one Montgomery element, read before the call returns).  With the transforms above, a chain
 * evaluate_over_domain -> pointwise -> interpolate (polynomial/univariate/mod.rs:305-360, evaluations/univariate/
 * mod.rs:40-50) runs between ONE upload and ONE download.  Asynchronous on the context stream; r may alias a or b. */
int ark_hip_fr_add_device(int field, const void* d_a, const void* d_b, void* d_r, size_t n);
int ark_hip_fr_sub_device(int field, const void* d_a, const void* d_b, void* d_r, size_t n);
int ark_hip_fr_neg_device(int field, const void* d_a, void* d_r, size_t n);
int ark_hip_fr_scale_device(int field, const void* d_a, const uint64_t* k, void* d_r, size_t n);
/* r[i] = a[i] / b[i] (Evaluations /= Evaluations, mod.rs:142-163) and r[i] = 1 / a[i] (ark_ff::batch_inversion,
 * ff/src/fields/mod.rs:358-385): a zero divisor gives zero, as the reference's batch inversion leaves zeros in place. */
int ark_hip_fr_div_device(int field, const void* d_a, const void* d_b, void* d_r, size_t n);
int ark_hip_fr_inverse_device(int field, const void* d_a, void* d_r, size_t n);
/* `&DensePolynomial * &DensePolynomial` (poly/src/polynomial/univariate/dense.rs:641-656: evaluate both factors over the
 * radix-2 domain of size >= na + nb - 1, multiply pointwise, interpolate) from HOST coefficient vectors: ONE upload of a and
 * b, both forward transforms in flight together (short factors on the degree-aware path), the pointwise product and the
 * inverse transform on the device, ONE download.  out: room for na + nb - 1 elements; *out_len: coefficients of the product
 * with leading zeros dropped as DensePolynomial::from_coefficients_vec leaves them (0: a factor was the zero polynomial).
 * ARK_HIP_ERR_ARG when the field's two-adicity cannot hold the domain (the reference panics there). */
int ark_hip_poly_mul(int field, const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out, size_t* out_len);
/* base^exp in Fr on the host (domain elements / twiddles for hosts without field code of their own) */
int ark_hip_fr_pow(int field, const uint64_t* base, uint64_t exp, uint64_t* out);
/* the G-point transform along the slow axis of a [G][cols] device array (G = 2, 4, 8 or 16), in place:
 * out[j][c] = sum_i root^(i j) in[i][c] */
int ark_hip_fft_axis_device(int field, void* d_data, unsigned G, size_t cols, const uint64_t* root);

/* ---- polynomial operations on device-resident vectors ------------------------------------------------------------
 * The O(n) steps that sit between the transforms and the MSM in a prover -- a KZG opening (p(z), the witness polynomial
 * (p(x) - p(z)) / (x - z)), the quotient by a vanishing polynomial, evaluation-form protocols -- on vectors that stay in
 * device memory.  `field` as for ark_hip_fr_*_device; elements are 4 x u64 Montgomery residues; d_* are device pointers
 * and the work runs on the context stream.  The single elements handed over by host pointer (point, z, tau) must be
 * canonical residues (< p), like every element of the vectors; they are not checked.  ARK_HIP_ERR_ARG for an unknown field or
 * a null pointer, checked before any device is touched; ARK_HIP_ERR_NO_DEVICE without a GPU. */
/* DensePolynomial::evaluate (poly/src/polynomial/univariate/dense.rs:42-92): *out = sum_i coeffs[i] point^i.  point and
 * out are HOST pointers to one element; the call waits for its result.  n = 0 gives 0; trailing zero coefficients are
 * allowed (a device vector is not truncated). */
int ark_hip_poly_evaluate_device(int field, const void* d_coeffs, size_t n, const uint64_t* point, uint64_t* out);
/* Division by x - z: what DenseOrSparsePolynomial::divide_with_q_and_r computes for a degree-1 divisor
 * (polynomial/univariate/mod.rs:145-159, the naive division).  Writes exactly max(n, 1) - 1 quotient elements
 * q[i] = sum_{j > i} p[j] z^(j-i-1) to d_quot and the remainder p(z) to the HOST element out_rem, waiting for it.
 * out_rem may be NULL: the call is then asynchronous like ark_hip_fr_*_device.  d_quot == d_coeffs (the same pointer) is
 * allowed, element n - 1 of the buffer is then left as it was; any other overlap of the two is undefined. */
int ark_hip_poly_divide_linear_device(int field, const void* d_coeffs, size_t n, const uint64_t* z, void* d_quot,
                                      uint64_t* out_rem);
/* DensePolynomial::divide_by_vanishing_poly (dense.rs:168-211).  As in the reference only the SIZE m of the domain enters:
 * the divisor is x^m - 1, also when the domain is a coset.  n >= m: d_quot receives n - m elements
 * q[j] = sum_{i >= 1, j + i m < n} p[j + i m], d_rem receives m elements r[j] = p[j] + q[j] (j < n - m), p[j] otherwise.
 * n < m: the quotient is empty and d_rem receives the n coefficients.  Asynchronous; no aliasing.  The work is O(n) on m
 * parallel lanes of n / m serial steps each: made for n a few times m with m large. */
int ark_hip_poly_divide_by_vanishing_device(int field, size_t domain_size, const void* d_coeffs, size_t n, void* d_quot,
                                            void* d_rem);
/* EvaluationDomain::evaluate_all_lagrange_coefficients (poly/src/domain/mod.rs:157-222): d_out[i] = L_i(tau) for the
 * dom->size points h g^i of the (coset) domain; when tau is one of them, that coefficient is one and the others are zero.
 * tau: HOST pointer to one element.  Asynchronous. */
int ark_hip_domain_lagrange_coefficients_device(int field, const ark_hip_radix2_domain* dom, const uint64_t* tau, void* d_out);
/* *out = sum_i a[i] b[i] (HOST element; the call waits).  With the Lagrange coefficients above: P(tau) from the
 * evaluations of P over the domain (the use domain/mod.rs:150-156 describes). */
int ark_hip_fr_inner_product_device(int field, const void* d_a, const void* d_b, size_t n, uint64_t* out);
/* Host only, no device needed: the tile length and the number of scan levels ark_hip_poly_evaluate_device and
 * ark_hip_poly_divide_linear_device use for n coefficients (one level while a tile holds them all, one more per factor
 * `tile`), as ark_hip_msm_plan exposes the MSM's plan. */
int ark_hip_poly_scan_plan(size_t n, int* tile, int* levels);
/* Prefix scans along a vector -- the accumulator column of a univariate prover (the grand product z of a permutation or
 * lookup argument, the running sum of a univariate logUp).  exclusive = 0: out[i] = prod_{j <= i} a[j]; exclusive = 1:
 * out[i] = prod_{j < i} a[j], so out[0] = 1.  Exactly n elements are written.  *out_total = prod_{j < n} a[j] is a HOST
 * element and the call waits for it (n = 0 gives one); out_total = NULL makes the call asynchronous like
 * ark_hip_fr_*_device.  d_out == d_a (the same pointer) is allowed, any other overlap is ARK_HIP_ERR_ARG.  Zeros are just
 * values: everything past a zero is zero. */
int ark_hip_fr_prefix_product_device(int field, const void* d_a, size_t n, int exclusive, void* d_out, uint64_t* out_total);
/* The same over addition: out[i] = sum_{j <= i} a[j] (exclusive: j < i, out[0] = 0), *out_total = sum_{j < n} a[j]. */
int ark_hip_fr_prefix_sum_device(int field, const void* d_a, size_t n, int exclusive, void* d_out, uint64_t* out_total);
/* The ratio accumulator z[0] = 1, z[i+1] = z[i] num[i] / den[i]: out[i] = prod_{j < i} num[j] / den[j] for i < n and
 * *out_last = prod_{j < n} num[j] / den[j] -- the value that must be one for a valid permutation (HOST element, the call waits
 * for it; NULL: asynchronous; n = 0 gives one).  One inversion per tile of ark_hip_prefix_scan_plan, not one per element.
 * d_out may be the same pointer as d_num or as d_den; any other overlap is ARK_HIP_ERR_ARG.  A zero denominator behaves as the
 * composition of the entries above would: out[i] = PN_i inv0(PD_i) with PN, PD the exclusive prefix products of num and den
 * and inv0(0) = 0 as ark_hip_fr_div_device defines it -- every output up to and including the index of the first zero
 * denominator is exact, every output after it is zero, and out_last follows the same rule. */
int ark_hip_fr_prefix_ratio_device(int field, const void* d_num, const void* d_den, size_t n, void* d_out, uint64_t* out_last);
/* Host only, no device needed: the tile length and the number of scan levels of the three entries above for n elements;
 * op 0 / 1 / 2 = product / sum / ratio (anything else: ARK_HIP_ERR_ARG).  One level while a tile holds the vector, one more per
 * factor `tile`. */
int ark_hip_prefix_scan_plan(int op, size_t n, int* tile, int* levels);

/* ---- gate expressions on device vectors: sums of products with rotations ----------------------
 * The row-by-row constraint expression of a univariate (Plonk-style) prover over a domain or an extended coset: for ncolumns
 * device vectors of n elements each and nterms terms,
 *   out[i] = c0 + sum_{j < nterms} c_j prod_{q < term_len[j]} col[ tc_{j,q} ][ (i + rot_{j,q}) mod n ],    0 <= i < n.
 * n is any size.  A rotation is any int64_t (negative, |rot| >= n, INT64_MIN): it is reduced to [0, n) on the host with the
 * mathematical mod; on a coset of blow-up k "the next row" is rotation k.  A column may appear in several terms and several
 * times in one term, and the same pointer may be passed as two columns.  The univariate counterpart of the list of products
 * of ark_hip_sumcheck_round_device: one pass instead of a composition of ark_hip_fr_mul_device, ark_hip_fr_axpy_device,
 * ark_hip_fr_lincomb_device and copies. */
#define ARK_HIP_SOP_MAX_COLUMNS 16
#define ARK_HIP_SOP_MAX_TERMS   16
#define ARK_HIP_SOP_MAX_DEGREE   8
/* term_len, term_columns and coeffs are laid out as ark_hip_sumcheck_round_device lays out term_len, term_tables and coeffs:
 * term j has term_len[j] factors (1 .. ARK_HIP_SOP_MAX_DEGREE), term_columns holds their column indices term after term,
 * coeffs holds nterms elements.  term_rotations runs parallel to term_columns; NULL: every rotation is zero.  c0: a HOST
 * element, NULL for zero.  A coefficient equal to one costs no product; one unit term of one factor without c0 is a rotated
 * copy.  Host pointers are read before the call returns; the call is asynchronous on the context stream; exactly n elements
 * are written, canonical residues.  n = 0 validates its arguments, launches nothing and succeeds (column pointers may be NULL).
 * d_out may be the SAME pointer as a column only if every factor that reads that column has rotation 0 after reduction (with
 * a rotation one workgroup would write what another still reads); any other overlap of d_out with a column is
 * ARK_HIP_ERR_ARG.  ARK_HIP_ERR_ARG, before any device is looked for: an unknown or unserved field; a null d_columns,
 * term_len, term_columns, coeffs or d_out; a null column pointer when n > 0; ncolumns, nterms or a term_len that is 0 or above
 * its limit; a column index >= ncolumns; n > 2^58; the aliasing violations above. */
int ark_hip_fr_sum_of_products_device(int field, const void* const* d_columns, unsigned ncolumns, size_t n,
                                      const unsigned* term_len, const unsigned* term_columns,
                                      const int64_t* term_rotations, const uint64_t* coeffs, unsigned nterms,
                                      const uint64_t* c0, void* d_out);
/* Host only, no device needed: the launch geometry of that call for n rows.  *blocks: workgroups of 256 lanes (0 for n = 0);
 * *rows_per_lane: rows one lane walks -- 1 until the grid's cap is reached (0 for n = 0; saturates at INT_MAX). */
int ark_hip_fr_sum_of_products_plan(size_t n, int* blocks, int* rows_per_lane);

/* ---- dense multilinear extensions on device-resident evaluation tables ---------------------------------------------
 * DenseMultilinearExtension (poly/src/evaluations/multivariate/multilinear/dense.rs): a table of 2^num_vars evaluations over
 * the boolean hypercube, index bit 0 being the FIRST variable (index 0b1011 is P(1,1,0,1)).  Committing to such a table is
 * an MSM with scalars_are_montgomery = 1 on the same device vector; these entries bind its variables without the table
 * leaving the device.  Conventions as for the section above: canonical Montgomery residues, points by HOST pointer read
 * before the call returns, ARK_HIP_ERR_ARG (also for num_vars >= 64, and for a device table of more than 2^58 elements,
 * whose bytes a size_t cannot count) before any device is touched. */
/* MultilinearExtension::fix_variables (dense.rs:224-257): binds the first `dim` variables to partial_point[0 .. dim-1] and
 * writes the 2^(num_vars - dim) evaluations of what is left to d_out; binding variable 0 maps
 * out[b] = t[2b] + r (t[2b+1] - t[2b]).  Several variables are bound per kernel launch (ark_hip_mle_fold_plan).  dim = 0
 * copies; dim > num_vars is ARK_HIP_ERR_ARG.  The input is left untouched.  There is NO in-place form: one workgroup writes
 * where another still reads, so d_out must not overlap d_evals (ARK_HIP_ERR_ARG).  Asynchronous. */
int ark_hip_mle_fix_variables_device(int field, const void* d_evals, unsigned num_vars, const uint64_t* partial_point,
                                     unsigned dim, void* d_out);
/* Polynomial::evaluate (dense.rs:460-465): binds all num_vars variables to point[0 .. num_vars-1] -- the launches of
 * fix_variables, the last one writing a result slot.  out is a HOST element; the call waits for it. */
int ark_hip_mle_evaluate_device(int field, const void* d_evals, unsigned num_vars, const uint64_t* point, uint64_t* out);
/* relabel / relabel_in_place (dense.rs:76-92, :195-199): d_out[i] = d_evals[swap_bits(i, a, b, k)], exchanging the k
 * variables from position a with the k from position b.  d_out == d_evals (the same pointer) works in place; any other
 * overlap is ARK_HIP_ERR_ARG.  After ordering a <= b: a == b or k == 0 copies (in place: nothing happens); otherwise
 * b + k <= num_vars and a + k <= b must hold (the reference's two assertions), else ARK_HIP_ERR_ARG.  Asynchronous. */
int ark_hip_mle_relabel_device(int field, const void* d_evals, unsigned num_vars, unsigned a, unsigned b, unsigned k,
                               void* d_out);
/* r[i] = a[i] + k x[i] in one pass (AddAssign<(F, &Self)>, dense.rs:319-327); k: HOST pointer to one element; r may alias a
 * or x.  Asynchronous. */
int ark_hip_fr_axpy_device(int field, const void* d_a, const uint64_t* k, const void* d_x, void* d_r, size_t n);
/* Host only, no device needed: the launches that bind `dim` variables of a 2^num_vars table.  *tile_log: the most variables
 * one launch binds; *passes: the number of launches; widths[0 .. *passes-1]: the variables each binds, in order (the rest of
 * the 8 entries are set to 0). */
int ark_hip_mle_fold_plan(unsigned num_vars, unsigned dim, int* tile_log, int* passes, int* widths);
/* Host only: tiles_log[p] = log2 of the tiles of 2^tile_log elements one wave takes in launch p of that plan (8 entries,
 * 0 past the last launch).  The fold kernel is compiled once per (variables bound, tiles per wave); more tiles per wave mean
 * fewer multiplies per element, and large tables get more of them.  Tests read from it which kernel variant a size runs. */
int ark_hip_mle_fold_tiles(unsigned num_vars, unsigned dim, int* tiles_log);
/* The table of eq(point, .): d_out[b] = scale * prod_{i < num_vars} (bit i of b ? point[i] :
 * 1 - point[i]) for all b < 2^num_vars -- the weights with <f, eq(r)> = f(r), the first factor of a zero-check's sum.
 * point: HOST, num_vars elements; scale: a HOST element, or NULL for one.  num_vars = 0 writes the one element `scale`.
 * The products are taken in Montgomery form, so the output is Montgomery residues like every table here.  A write-only
 * pass: ceil(num_vars / 9) launches (ark_hip_mle_eq_plan), each reading 1/512 of what it writes.  Asynchronous. */
int ark_hip_mle_eq_table_device(int field, const uint64_t* point, unsigned num_vars, const uint64_t* scale, void* d_out);
/* The quotients of a multilinear opening at `point`:
 *   f(x) - f(point) = sum_i (x_i - point_i) q_i(x_{i+1}, .., x_{num_vars-1}),   q_i[b] = f_i[2b+1] - f_i[2b],
 * f_0 = f and f_{i+1} = f_i with its first variable bound to point[i]: the differences fix_variables forms and drops.
 * d_quot receives 2^num_vars - 1 elements: segment i (0 <= i < num_vars) lies at element offset
 * 2^num_vars - 2^(num_vars-i) and holds the 2^(num_vars-1-i) elements of q_i, each a device vector an MSM with
 * scalars_are_montgomery = 1 commits to.  out_value: a HOST element that receives f(point) -- bit for bit what
 * ark_hip_mle_evaluate_device returns -- and the call waits for it; NULL makes the call asynchronous.  num_vars = 0 writes
 * no quotient (d_quot may be NULL) and the value is d_evals[0].  The input is left untouched.  There is NO in-place form,
 * as for fix_variables: d_quot must not overlap d_evals (ARK_HIP_ERR_ARG). */
int ark_hip_mle_quotients_device(int field, const void* d_evals, unsigned num_vars, const uint64_t* point, void* d_quot,
                                 uint64_t* out_value);
/* Host only, no device needed: the launches of the two calls above for a 2^num_vars table, as ark_hip_mle_fold_plan and
 * ark_hip_mle_fold_tiles report the fold's.  *tile_log: the most variables one launch takes; *passes: the number of
 * launches; widths[p]: the variables launch p takes; tiles_log[p]: log2 of the tiles of 2^tile_log elements one wave takes
 * in it (8 entries each, 0 past the last launch).  The eq table's launch p writes the table of the TOP widths[0] + .. +
 * widths[p] variables (num_vars = 0: one launch of no variables); the quotients' launch p binds the next widths[p]
 * variables from the first on, its kernel compiled once per width.  Tests read from them which sizes reach which variant. */
int ark_hip_mle_eq_plan(unsigned num_vars, int* tile_log, int* passes, int* widths, int* tiles_log);
int ark_hip_mle_quotients_plan(unsigned num_vars, int* tile_log, int* passes, int* widths, int* tiles_log);

/* ---- grand products on device tables -----------------------------------------------------------
 * The binary product tree over a table, pairing over the LAST variable: L_nu = the table, L_k[i] = L_{k+1}[i] *
 * L_{k+1}[i + 2^k] for i < 2^k, L_0 = [the product of all entries].  The two factors of a level are the two contiguous
 * halves of the level above, so L_k(r) = sum_x eq(r, x) L_{k+1}(x, 0) L_{k+1}(x, 1) is a sumcheck over two views
 * (ark_hip_sumcheck_round_device), and the layered proof of the product ends in one evaluation of the table.
 * d_tree: 2^num_vars - 1 elements in the layout of ark_hip_mle_quotients_device: level j (1 <= j <= num_vars) is
 * L_{num_vars-j}, 2^(num_vars-j) elements at element offset 2^num_vars - 2^(num_vars-j+1); the product is the last element.
 * out_product: a HOST element, the call waits for it; NULL makes the call asynchronous.  num_vars = 0: no tree (d_tree may
 * be NULL), the product is d_evals[0].  The input is left untouched; d_tree must not overlap d_evals (ARK_HIP_ERR_ARG).
 * ARK_HIP_ERR_ARG comes before any device is touched for an unknown field, a null pointer, num_vars >= 64 or a table
 * whose bytes a size_t cannot count, as for ark_hip_mle_quotients_device.  No scratch: later launches read the levels the
 * earlier ones wrote in d_tree. */
#define ARK_HIP_PRODUCT_TREE_LEVELS 3
int ark_hip_mle_product_tree_device(int field, const void* d_evals, unsigned num_vars, void* d_tree, uint64_t* out_product);
/* Host only, no device needed: the launches of that call.  A launch forms up to ARK_HIP_PRODUCT_TREE_LEVELS consecutive
 * levels from the level above them; a table of 58 variables takes 20 launches, so entry p (8 entries each, 0 past the last)
 * is a RUN of consecutive launches of one kernel instantiation: first the full launches, widths[0] levels in all,
 * ARK_HIP_PRODUCT_TREE_LEVELS per launch; then the one remainder launch of 1 or 2 levels.  At most two entries; the widths
 * sum to num_vars.  group_log[p] = log2 of the chunks of 64 output indices one wave takes: always 0 (several chunks per
 * wave were measured no faster and are not built).  Levels of fewer than 64 elements are left to the same kernel in launches
 * of one partly filled wave; there is no separate tail kernel. */
int ark_hip_mle_product_tree_plan(unsigned num_vars, int* passes, int* widths, int* group_log);
/* d_out[i] = c0 + sum_k coeffs[k] * d_tables[k][i] for i < n, in one pass: the fingerprints gamma + sum_k c_k T_k[i] that
 * are the leaves of a grand product.  d_tables: HOST array of ntables device pointers; coeffs: HOST, ntables elements; c0:
 * a HOST element or NULL for zero; 1 <= ntables <= 8.  d_out may be the same pointer as one of the tables; any other
 * overlap of d_out with a table is ARK_HIP_ERR_ARG.  Asynchronous. */
int ark_hip_fr_lincomb_device(int field, const void* const* d_tables, unsigned ntables, const uint64_t* coeffs,
                              const uint64_t* c0, void* d_out, size_t n);

/* ---- fractional sums on device tables -----------------------------------------------------------
 * A lookup argument in logUp form reduces to a sum of fractions, sum_i 1 / (gamma + w_i) = sum_j m_j / (gamma + t_j).  The
 * fraction tree carries pairs (N, D) and adds fractions level by level, pairing over the LAST variable as the product tree
 * does: N_nu = d_num, D_nu = d_den (2^num_vars elements each), and for i < 2^k
 *   N_k[i] = N_{k+1}[i] * D_{k+1}[i + 2^k] + N_{k+1}[i + 2^k] * D_{k+1}[i],     D_k[i] = D_{k+1}[i] * D_{k+1}[i + 2^k];
 * (N_0[0], D_0[0]) is the root (P, Q) with P / Q = sum_b N_nu[b] / D_nu[b].  Nothing is inverted and a zero denominator is
 * just a value.  d_num_tree, d_den_tree: 2^num_vars - 1 elements each in the layout of ark_hip_mle_product_tree_device --
 * level j (1 <= j <= num_vars) is L_{num_vars-j}, 2^(num_vars-j) elements at element offset 2^num_vars - 2^(num_vars-j+1),
 * the root last.  d_num == NULL: every numerator is one (the witness side of a lookup); no numerator leaf is read, the first
 * level is N = D[i] + D[i + h], D = D[i] * D[i + h], and d_num_tree still receives levels 1 .. num_vars.
 * out_root: a HOST pointer to two elements (P, Q), the call waits for it; NULL makes the call asynchronous.  num_vars = 0:
 * no trees (both tree pointers may be NULL), the root is (d_num[0] or one, d_den[0]).  The inputs are left untouched; the
 * two trees must not overlap each other or an input (ARK_HIP_ERR_ARG).  ARK_HIP_ERR_ARG comes before any device is touched
 * for an unknown field, a null d_den, a null tree with num_vars > 0, num_vars >= 64 or tables of more than 2^58 elements,
 * and any such overlap.  No scratch: later launches read the levels the earlier ones wrote in the trees. */
#define ARK_HIP_FRACTION_TREE_LEVELS 2
int ark_hip_mle_fraction_tree_device(int field, const void* d_num, const void* d_den, unsigned num_vars, void* d_num_tree,
                                     void* d_den_tree, uint64_t* out_root);
/* Host only, no device needed: the launches of that call, reported as ark_hip_mle_product_tree_plan reports the product
 * tree's.  Entry p (8 entries each, 0 past the last) is a RUN of consecutive launches of one kernel instantiation: first the
 * full launches, widths[0] levels in all, ARK_HIP_FRACTION_TREE_LEVELS per launch; then the one remainder launch.  At most
 * two entries; the widths sum to num_vars; group_log[p] is always 0.  has_num = 0 (ones for numerators) changes the kernel
 * variant of the first launch, not the launches. */
int ark_hip_mle_fraction_tree_plan(unsigned num_vars, int has_num, int* passes, int* widths, int* group_log);
/* The multiplicity table of a lookup: d_out[j] = #{i < n : d_indices[i] = j} for j < table_len, as Montgomery elements.
 * d_indices: n device uint32_t (may be NULL when n = 0); table_len need not be a power of two.  An index >= table_len is
 * SKIPPED and not reported: sum_j d_out[j] = n holds exactly when none was skipped.  n = 0 writes zeros.  No scratch: the
 * output is its own workspace (cleared, counted into with atomic adds on each cell's first word, converted in place).
 * ARK_HIP_ERR_ARG comes before any device is touched for an unknown field, a null pointer, table_len = 0, n >= 2^32,
 * table_len > 2^58, or d_out overlapping the indices.  Asynchronous. */
int ark_hip_fr_count_indices_device(int field, const uint32_t* d_indices, size_t n, void* d_out, size_t table_len);

/* ---- lookup by value on device vectors ----------------------------------------------------------
 * The join of a lookup argument, from the VALUES: for a table t of table_len elements and a witness w of n elements, both
 * device-resident (a column, or tuples that ark_hip_fr_lincomb_device has compressed with theta), the index of every witness
 * cell in the table and the multiplicities m_j = #{i : w_i = t_j}, without an index array from the host.  Elements are
 * 4 x u64 canonical Montgomery residues as in the rest of the ark_hip_fr_*_device block; they are not checked, and two
 * elements are equal exactly when their eight 32-bit words are equal.
 *   d_indices (n uint32_t, or NULL): d_indices[i] = the SMALLEST j with d_table[j] == d_values[i], or
 *     ARK_HIP_LOOKUP_MISSING when there is none.
 *   d_mult (table_len elements, or NULL): d_mult[j] = #{i : d_indices[i] = j} as a Montgomery element.  When a table value is
 *     repeated, its FIRST occurrence receives all the counts and the later ones receive zero: sum_j m_j / (gamma + t_j) is then
 *     still sum over the found cells of 1 / (gamma + w_i), which is what the fractional sum of a lookup needs.  d_mult may hold
 *     anything beforehand; n = 0 writes zeros.
 *   out_missing (HOST, or NULL): the number of witness cells that were not found; the call waits for it.  NULL makes the
 *     call asynchronous on the context stream.
 * At least one of the three outputs must be non-NULL; out_missing alone is a membership check.  The two inputs may overlap or be
 * the same pointer: looking a table up in itself yields each entry's first occurrence.  The inputs are left untouched.
 * The table is hashed per call into 2^capacity_log four-byte slots (open addressing, load factor at most 1/2) in the
 * context's scratch, see ark_hip_fr_lookup_plan; nothing is kept between calls.  The result does not depend on scheduling.
 * ARK_HIP_ERR_ARG comes before any device is touched for an unknown field, table_len = 0, table_len > 2^28, n >= 2^32, a
 * null input with a non-zero length, all three outputs NULL, or an output that overlaps an input or the other output. */
#define ARK_HIP_LOOKUP_MISSING 0xFFFFFFFFu
int ark_hip_fr_lookup_device(int field, const void* d_table, size_t table_len, const void* d_values, size_t n,
                             uint32_t* d_indices, void* d_mult, uint64_t* out_missing);
/* Host only, no device needed: capacity_log = the smallest c >= 1 with 2^c >= 2 * table_len, and scratch_bytes = what that
 * call asks of the context's scratch buffer (a result slot, the miss counter and the slots).  ARK_HIP_ERR_ARG for a null
 * pointer, table_len = 0 or table_len > 2^28. */
int ark_hip_fr_lookup_plan(size_t table_len, unsigned* capacity_log, size_t* scratch_bytes);

/* ---- sparse constraint matrices on the device ---------------------------------------------------
 * The matrices of an R1CS / CCS instance in CSR form, resident on the device, and their products with device vectors:
 * A z, B z, C z in front of a quotient or a sumcheck, M^T eq(rx) for the second sumcheck of a Spartan-style prover, and with
 * an inner product the value of the sparse multilinear extension, eq(rx)^T M eq(ry).  Elements follow the conventions of the
 * ark_hip_fr_*_device block: 4 x u64 canonical Montgomery residues, not checked; ARK_HIP_ERR_ARG comes before any device is
 * looked for; work runs on the context stream.
 *
 * ark_hip_fr_csr_create takes HOST arrays (a circuit's matrices come from a host compiler once per circuit): row_ptr
 * (rows + 1 entries), col_idx (nnz), vals (nnz elements).  Everything a kernel will index with is validated here, on the host:
 * row_ptr[0] = 0, row_ptr non-decreasing, row_ptr[rows] = nnz, every col_idx < cols, rows, cols and nnz < 2^32, non-null
 * pointers wherever a count is non-zero (row_ptr may be NULL only when rows = 0 and nnz = 0), a scalar field this build
 * serves, no flag bit other than ARK_HIP_CSR_WITH_TRANSPOSE, a non-null out.  Any violation is ARK_HIP_ERR_ARG with nothing
 * allocated and *out untouched.  Duplicate column indices inside a row are legal and add; rows = 0, cols = 0 and nnz = 0 are
 * legal; zero values are values.  With ARK_HIP_CSR_WITH_TRANSPOSE the handle also holds M^T in the same form, built on the host
 * by a STABLE counting sort over the columns: inside a row of M^T the entries keep ascending original row order.  The call
 * returns when the handle is complete; the host arrays are not referenced afterwards.  The handle belongs to the caller,
 * like a prepared base set, and to the device that was current when it was created.
 *
 * ark_hip_fr_csr_free waits for work that may still read the handle; NULL is fine.
 *
 * ark_hip_fr_csr_mul_device: transpose = 0 computes y = M x with x_len = cols, y_len = rows; transpose = 1 computes
 * y = M^T x with x_len = rows, y_len = cols and needs a handle created with ARK_HIP_CSR_WITH_TRANSPOSE.  Exactly y_len
 * elements are written; empty rows give zero.  ARK_HIP_ERR_ARG: a null handle, transpose not 0 or 1 or 1 without the flag, a
 * wrong length, a null vector with a non-zero length, any overlap of d_x and d_y.  Asynchronous.  No atomics on field elements:
 * the result is canonical and bit-exact.  Scratch: one partial per chunk of a long row, all written by the same call.
 *
 * ark_hip_csr_plan is host only and needs no device: how create cuts `rows` rows with these row_ptr (the same validation:
 * row_ptr[0] = 0, non-decreasing, else ARK_HIP_ERR_ARG; NULL only with rows = 0) into work.  *tile (at most 2^16): nonzeros per
 * workgroup; *max_rows: rows per stream block; *blocks: stream blocks -- runs of consecutive rows with at most `tile`
 * nonzeros and `max_rows` rows, empty rows counting; *long_rows: rows with more than `tile` nonzeros, each alone;
 * *long_chunks: the sum of ceil(nnz / tile) over the long rows.  Every output pointer may be NULL. */
typedef struct ark_hip_fr_csr ark_hip_fr_csr;
#define ARK_HIP_CSR_WITH_TRANSPOSE 1u
int ark_hip_fr_csr_create(int field, size_t rows, size_t cols, const uint32_t* row_ptr, const uint32_t* col_idx,
                          const uint64_t* vals, size_t nnz, unsigned flags, ark_hip_fr_csr** out);
int ark_hip_fr_csr_free(ark_hip_fr_csr* m);
int ark_hip_fr_csr_mul_device(const ark_hip_fr_csr* m, int transpose, const void* d_x, size_t x_len, void* d_y, size_t y_len);
int ark_hip_csr_plan(size_t rows, const uint32_t* row_ptr, int* tile, int* max_rows, size_t* blocks, size_t* long_rows,
                     size_t* long_chunks);

/* ---- the sumcheck prover's round on device tables --------------------------------------------
 * The sum is a list of products of multilinear tables, each with a coefficient (ListOfProductsOfPolynomials of
 * ark-linear-sumcheck): sum_j c_j prod_{k in term j} f_k.  Tables follow the conventions above: 2^num_vars Montgomery
 * elements on the device, index bit 0 the first variable. */
#define ARK_HIP_SUMCHECK_MAX_TABLES 8
#define ARK_HIP_SUMCHECK_MAX_TERMS 8
#define ARK_HIP_SUMCHECK_MAX_DEGREE 4
/* One round.  d_tables: ntables device tables of 2^num_vars elements (the same table may appear twice).  Term j has
 * term_len[j] factors (1 .. ARK_HIP_SUMCHECK_MAX_DEGREE); term_tables holds their table indices, term after term
 * (term_len[0] + ... + term_len[nterms-1] entries, repeats allowed); coeffs holds nterms elements.  D = the longest term.
 * Without r_prev, for m = num_vars >= 1 and T = the tables:
 *   out_evals[t] = sum_{b < 2^(m-1)} sum_j c_j prod_{k in term j} ( T_k[2b] + t (T_k[2b+1] - T_k[2b]) ),  t = 0 .. D.
 * With r_prev (a HOST element) the call first binds the first variable to it: it writes
 *   T'_k[i] = T_k[2i] + r_prev (T_k[2i+1] - T_k[2i])
 * to d_out_tables[k] (ntables tables of 2^(num_vars-1) elements) and computes the sums above over T' with m = num_vars - 1,
 * reading every table once.  When m = 0 nothing is left to sum: the one-element tables are the values f_k(r_1 .. r_nu),
 * out_evals[0] = sum_j c_j prod_k T'_k[0] -- what the verifier's last check compares -- and out_evals[1 .. D] are zero.
 * out_evals: HOST, D + 1 elements; the call waits for them.  Host pointers are read before the call returns.
 * ARK_HIP_ERR_ARG, before any device is touched: an unknown field; a null pointer; ntables, nterms or a term_len that is 0 or
 * above its limit; a table index >= ntables; num_vars >= 64 or a table whose bytes a size_t cannot count; num_vars == 0
 * (with or without r_prev); an output table that overlaps an input table or another output table -- there is NO in-place
 * form, one workgroup writes where another still reads.  d_out_tables is not read without r_prev. */
int ark_hip_sumcheck_round_device(int field, const void* const* d_tables, unsigned ntables, unsigned num_vars,
                                  const unsigned* term_len, const unsigned* term_tables, const uint64_t* coeffs, unsigned nterms,
                                  const uint64_t* r_prev, void* const* d_out_tables, uint64_t* out_evals);
/* Host only, no device needed: the launch geometry of that round for 2^num_vars-element tables (fused: with r_prev).
 * *blocks: workgroups of 256 lanes; *pairs_per_lane: pairs of rows one lane walks (> 1 once the grid is capped; saturates at INT_MAX); *stages: 1
 * when one workgroup holds the whole sum, 2 when a second launch adds the workgroups' partial sums.  Tests read from it
 * which variant a size runs.  ntables and degree select the kernel (tables held per lane), not the geometry. */
int ark_hip_sumcheck_plan(unsigned num_vars, unsigned ntables, unsigned degree, int fused, int* blocks, int* pairs_per_lane,
                          int* stages);

/* ---- the Fiat-Shamir transcript and the whole sumcheck proof in one wait ----------------------
 * The transcript's state is 32 bytes, initialised by the caller (a label, a statement hash).  Its one operation absorbs
 * count >= 0 elements and returns a challenge:
 *   msg   = state | u32_le(count) | le32(e_0) | ... | le32(e_{count-1})    (le32: the canonical value, 32 bytes little-endian)
 *   out   = SHAKE256(msg, 96 bytes);   state = out[0:32];   challenge = int_le(out[32:96]) mod r, in Montgomery form.
 * Host only, no device needed; state is updated in place.  elements: count Montgomery elements, canonical residues like
 * every other entry's -- this is NOT checked.  ARK_HIP_ERR_ARG: an unknown field, a null state or out_challenge, null
 * elements with count > 0, count > 2^24 (the message is built in host memory: 512 MiB at that count). */
int ark_hip_transcript_challenge(int field, uint8_t* state, const uint64_t* elements, unsigned count, uint64_t* out_challenge);
/* The largest number of variables the one-workgroup tail of ark_hip_sumcheck_prove_device takes. */
#define ARK_HIP_SUMCHECK_TAIL_MAX_VARS 14
/* The whole proof of the sum of ark_hip_sumcheck_round_device's list of products over 2^num_vars-element tables, the
 * challenges derived on the device: exactly what num_vars + 1 calls of the round entry give when the challenge after round
 * i is ark_hip_transcript_challenge(state, evals_i, D + 1).  out_rounds: num_vars x (D + 1) elements; out_point: the
 * num_vars challenges; out_finals: f_k(point) per table; out_value: sum_j c_j prod_k f_k(point); state (HOST, in/out): the
 * state after the last challenge -- the final values are not absorbed.  All outputs are HOST; the call queues everything
 * and waits once.  The caller's tables are never written.  d_work: work_elems elements (ark_hip_sumcheck_prove_plan) for
 * two alternating sets of bound tables.  tail_vars: once at most that many variables are left one workgroup runs every
 * remaining round in one launch; 0 disables that, -1 takes the library's measured default.
 * ARK_HIP_ERR_ARG, before any device is touched: every argument error of the round entry; a null state, output or d_work;
 * tail_vars outside -1 .. ARK_HIP_SUMCHECK_TAIL_MAX_VARS; d_work overlapping an input table. */
int ark_hip_sumcheck_prove_device(int field, const void* const* d_tables, unsigned ntables, unsigned num_vars,
                                  const unsigned* term_len, const unsigned* term_tables, const uint64_t* coeffs, unsigned nterms,
                                  uint8_t* state, int tail_vars, void* d_work, uint64_t* out_rounds, uint64_t* out_point,
                                  uint64_t* out_finals, uint64_t* out_value);
/* Host only: *work_elems = ntables (2^(num_vars-1) + 2^max(num_vars-2, 0)); *launches: kernels the proof queues;
 * *tail_from: the variables left when the tail takes over (tail_vars resolved and clamped to num_vars; 0: no tail). */
int ark_hip_sumcheck_prove_plan(unsigned num_vars, unsigned ntables, int tail_vars, size_t* work_elems, int* launches,
                                int* tail_from);

/* ---- one process per GPU: RCCL inside the library ---------------------------------------------------------------
 * The reference chunks an MSM by base range and sums the chunk results (variable_base/mod.rs:521-557); an FFT shards by
 * coefficient range with ONE transpose between two rounds of local butterflies (the four-step form of the radix-2
 * recursion, radix2/fft.rs:190-349).  Across the GPUs of a node both need exactly one exchange, and the library runs it
 * itself on RCCL (loaded at run time: librccl.so.1, the copy the process already has if any -- e.g. PyTorch's):
 *   id:    rank 0 calls ark_hip_comm_unique_id and ships the ARK_HIP_COMM_ID_BYTES to the other ranks by any means the
 *          host has (MPI, a TCP socket, torch.distributed's store);
 *   init:  every rank calls ark_hip_comm_init(id, rank, world) on its device (collective: ncclCommInitRank);
 *   then the *_sharded entries below are collective calls: every rank makes the same sequence of them.
 * Without a communicator (or with world = 1) they run the single-GPU path. */
#define ARK_HIP_COMM_ID_BYTES 128
int ark_hip_comm_unique_id(void* out_id);
int ark_hip_comm_init(const void* id, int rank, int world);
int ark_hip_comm_info(int* rank, int* world);   /* (0, 1) when this device has no communicator */
int ark_hip_comm_destroy(void);
/* One MSM over the union of all ranks' (base, scalar) shards, device-resident; every rank receives the same sum.  The
 * exchange is an all-gather of one Projective per rank (3 field elements: elliptic-curve addition is not an RCCL reduce
 * op) followed by world - 1 point additions in rank order.  _prepared_: this rank's shard as a prepared base set. */
int ark_hip_msm_sw_device_sharded(int curve, const void* d_bases, const void* d_scalars, size_t n_local,
                                  int scalars_are_montgomery, uint64_t* out_xyz);
int ark_hip_msm_prepared_device_sharded(const ark_hip_msm_bases* bases, const void* d_scalars, size_t n_local,
                                        int scalars_are_montgomery, uint64_t* out_xyz);
/* Radix-2 FFT / IFFT of dom->size = G m elements over G = world ranks (G a power of two <= 16, G^2 | size), m per rank,
 * in place on d_local, ONE all-to-all.  With i = i1 + G i2 and j = j1 m + j2 (i1, j1 < G; i2, j2 < m; sub = m / G):
 *     X[j1 m + j2] = sum_i1 w_G^(i1 j1) * w_n^(i1 j2) * ( sum_i2 w_m^(i2 j2) x[i1 + G i2] )
 *   forward  in:  d_local[i2] = x[rank + G i2]                       (cyclic by coefficient index)
 *            out: d_local[j1 sub + t] = X[j1 m + rank sub + t]       (G rows of the rank's j2 range)
 *            = size-m transform with the twiddle w_n^rank fused into its last pass, all-to-all, G-point transform
 *   inverse  takes the forward's output layout back to the forward's input layout (G-point transform, all-to-all,
 *            twiddle fused into the first pass of the size-m inverse transform, 1/n into its last).
 * A coset domain (dom->offset != 1) is honoured as in the single-GPU transform.  The exchange is cut into slices that
 * travel on a second stream while the G-point kernel works on the previous slice.  Asynchronous on the context stream. */
int ark_hip_fft_sharded_device(int field, const ark_hip_radix2_domain* dom, void* d_local, int inverse);
/* The two local halves of that transform for a host that brings its own exchange (MPI, gloo, ...), and for testing the
 * decomposition on one GPU:  _local: the size-m transform with the per-rank twiddle (forward: first step; inverse: last
 * step);  _cross: the G-point transform of a [G][sub] array, d_src -> d_dst (may alias).  Forward = local, all-to-all
 * (block q of every rank to rank q), cross;  inverse = cross, all-to-all, local. */
int ark_hip_fft_shard_local_device(int field, const ark_hip_radix2_domain* dom, int rank, int world, void* d_local,
                                   int inverse);
int ark_hip_fft_shard_cross_device(int field, const ark_hip_radix2_domain* dom, int world, const void* d_src, void* d_dst,
                                   int inverse);
/* Which pass kernel the transforms of the current device use: 0 = saturated 32-bit limbs (default), 1 = carry-free 9 x 29-bit
 * limbs (same results bit for bit; measured no faster: DESIGN.md section 5), -1 = the environment's choice (ARK_HIP_FFT_LAZY). */
int ark_hip_fft_set_kernel(int variant);
int ark_hip_fft_set_timing(int enable);
/* [total_ms, npass, pass0_ms, pass1_ms, ...] of the last timed device transform */
int ark_hip_fft_last_timing(double out[10]);

/* ---- one-word prime fields: the reference's SmallFp<P> (ff/src/fields/models/small_fp/) for Goldilocks, BabyBear and
 * KoalaBear.  A family of its own: these ids are NOT field ids, and every `field` argument above keeps answering
 * ARK_HIP_ERR_ARG to anything but the three four-limb scalar fields.
 * An element in memory is SmallFp::value, the canonical Montgomery residue x * R mod p in the field's own word: uint64_t with
 * R = 2^64 for Goldilocks, uint32_t with R = 2^32 (not 2^31) for the two 31-bit fields.  Vectors are arrays of that word; single
 * elements cross this interface as uint64_t, zero-extended.  Every output is canonical (< p) and equals the reference's bit for
 * bit.  Argument errors (an unknown sfield, a null pointer -- of a vector only with n > 0 --, stride < size, num_coeffs out of range, a domain whose size is not
 * 2^log_size_of_group, an element >= p) are ARK_HIP_ERR_ARG before any device is touched; ARK_HIP_ERR_NO_DEVICE without a GPU. */
enum { ARK_HIP_SFP_GOLDILOCKS = 0, ARK_HIP_SFP_BABYBEAR = 1, ARK_HIP_SFP_KOALABEAR = 2 };
typedef struct {
  uint64_t size;
  uint32_t log_size_of_group, _pad;
  uint64_t size_as_field_element, size_inv, group_gen, group_gen_inv, offset, offset_inv, offset_pow_size;
} ark_hip_sfp_radix2_domain;
/* out = { element bytes, p, k_bits, R mod p, R^2 mod p, generator, two-adicity, two-adic root of unity }, the last three
 * element values as stored.  Host only. */
int ark_hip_sfp_info(int sfield, uint64_t out[8]);
/* base^exp; host only */
int ark_hip_sfp_pow(int sfield, uint64_t base, uint64_t exp, uint64_t* out);
/* Radix2EvaluationDomain::new / get_coset (poly/src/domain/radix2/mod.rs:55-92): ARK_HIP_ERR_SIZE beyond the two-adicity,
 * ARK_HIP_ERR_ARG for a zero offset or one >= p.  Host only. */
int ark_hip_sfp_radix2_domain_new(int sfield, size_t num_coeffs, ark_hip_sfp_radix2_domain* out);
int ark_hip_sfp_radix2_domain_get_coset(int sfield, const ark_hip_sfp_radix2_domain* dom, uint64_t offset,
                                        ark_hip_sfp_radix2_domain* out);
/* fft_in_place / ifft_in_place of dom->size elements in HOST memory: one upload, the transform, one download */
int ark_hip_sfp_fft_in_place(int sfield, const ark_hip_sfp_radix2_domain* dom, void* host_data, int inverse);
/* count transforms, the j-th in place at element offset j * stride of d_data (stride >= dom->size); asynchronous on the context
 * stream.  Forward: only the first num_coeffs (1 .. size) elements of a column are read, the rest counts as zero (the reference's
 * resize).  Inverse: num_coeffs must equal size.  count = 0 does nothing.  Exactly size elements per column are written; the gaps
 * between columns are untouched. */
int ark_hip_sfp_fft_batch_device(int sfield, const ark_hip_sfp_radix2_domain* dom, void* d_data, size_t count, size_t stride,
                                 size_t num_coeffs, int inverse);
/* The pass plan of a transform of 2^log_n elements, host only: out = { largest log n one workgroup transforms alone, tile log,
 * segment log (elements per 128 bytes), passes, stages of pass 0, 1, 2, 3 }.  ARK_HIP_ERR_SIZE beyond the two-adicity. */
int ark_hip_sfp_fft_plan(int sfield, unsigned log_n, int out[8]);
/* Pointwise on device vectors of n elements (any n, 0 included); d_r may be d_a or d_b.  Asynchronous.  inverse: a zero stays
 * zero.  from_canonical takes integers of the word's whole range and reduces values >= p first (SmallFpConfig::new);
 * into_canonical gives the integer < p. */
int ark_hip_sfp_add_device(int sfield, const void* d_a, const void* d_b, void* d_r, size_t n);
int ark_hip_sfp_sub_device(int sfield, const void* d_a, const void* d_b, void* d_r, size_t n);
int ark_hip_sfp_mul_device(int sfield, const void* d_a, const void* d_b, void* d_r, size_t n);
int ark_hip_sfp_neg_device(int sfield, const void* d_a, void* d_r, size_t n);
int ark_hip_sfp_inverse_device(int sfield, const void* d_a, void* d_r, size_t n);
int ark_hip_sfp_scale_device(int sfield, const void* d_a, uint64_t k, void* d_r, size_t n);
int ark_hip_sfp_from_canonical_device(int sfield, const void* d_a, void* d_r, size_t n);
int ark_hip_sfp_into_canonical_device(int sfield, const void* d_a, void* d_r, size_t n);

/* ---- Merkle commitments: SHA3-256 trees over the rows of a column batch.  An extension: the reference has no Merkle tree; the
 * leaf encoding is pinned on it (a leaf hashes the bytes CanonicalSerialize::serialize_compressed writes for the row's elements).
 * H = SHA3-256 (FIPS 202: rate 136 bytes, suffix 0x06); a digest is 32 bytes.
 *   matrix  count >= 1 columns of n = 2^k elements (k >= 0); column j starts at element offset j * stride of d_data, stride >= n:
 *           the layout of ark_hip_sfp_fft_batch_device.  count <= 2^32 - 2.
 *   leaf(i) = H( u32_le(count) | u32_le(elem_bytes) | ser(col_0[i]) | .. | ser(col_{count-1}[i]) )
 *           one-word fields: ser = the stored word, little-endian, 4 or 8 bytes (small_fp/serialize.rs:23-31);
 *           Fr fields: ser = the canonical value out of Montgomery form, 32 bytes little-endian (fp/mod.rs:551-628).
 *   node    = H( u32_le(0xFFFFFFFF) | u32_le(0) | left | right ): 72 bytes, one permutation; no leaf header equals the node's.
 *           The 8-byte headers keep every message a whole number of 32-bit words and 8- and 32-byte elements on 64-bit lanes.
 *   tree    2n - 1 digests in d_tree: node t at byte 32 t, the root t = 0, children 2t + 1 and 2t + 2, leaf i at t = n - 1 + i;
 *           n = 1: the root is the leaf.
 *   path    of index i: the k siblings from the leaf level upwards, 32 bytes each.
 * Elements are in memory form (Montgomery) everywhere; elements >= p are not checked.
 * ARK_HIP_ERR_ARG, before any device is touched: an unknown sfield / field; n zero or not a power of two; count = 0 or
 * > 2^32 - 2; stride < n; elem_bytes not 4, 8 or 32; a null pointer where one is needed; d_data not aligned to its element
 * (32-byte elements: 16 bytes) or d_tree not aligned to 16 bytes; d_tree overlapping the matrix's extent
 * ((count - 1) * stride + n elements from d_data); an index >= n; out_rows without d_data or d_data without out_rows.
 * ARK_HIP_ERR_SIZE: n > 2^40, or an extent beyond size_t.  ARK_HIP_ERR_NO_DEVICE from the device entries without a GPU. */
#define ARK_HIP_MERKLE_DIGEST_BYTES 32
/* The tree of a matrix of one-word (sfield: ARK_HIP_SFP_*) or Fr (field: a scalar-field id) elements.  out_root NULL: asynchronous
 * on the context stream, the root is then the first 32 bytes of d_tree; out_root (HOST, 32 bytes) set: one wait.  d_data is
 * never written; exactly (2n - 1) * 32 bytes of d_tree are written. */
int ark_hip_merkle_commit_sfp_device(int sfield, const void* d_data, size_t count, size_t stride, size_t n, void* d_tree,
                                     uint8_t* out_root);
int ark_hip_merkle_commit_fr_device(int field, const void* d_data, size_t count, size_t stride, size_t n, void* d_tree,
                                    uint8_t* out_root);
/* Openings of q >= 0 indices (HOST, any order, repeats allowed) of a committed tree: out_paths (HOST) receives q * log2 n * 32
 * bytes, query by query (may be NULL when n = 1 or q = 0); out_rows (HOST) receives q * count elements of elem_bytes bytes in
 * memory form, query by query, read from d_data (the matrix the tree was built from: count, stride as then).  d_data and out_rows
 * may both be NULL for paths only (count and stride are then ignored).  One gather launch into staged device memory, one copy,
 * one wait. */
int ark_hip_merkle_open_device(const void* d_tree, size_t n, const void* d_data, unsigned elem_bytes, size_t count, size_t stride,
                               const uint64_t* indices, size_t q, void* out_rows, uint8_t* out_paths);
/* Host only, no GPU needed.  row: the count elements of one row, contiguous, in memory form (one-word fields: the field's own
 * word; Fr: 4 x uint64_t each).  verify: path holds log2 n digests (may be NULL when n = 1); *ok = 1 when the row at `index`
 * with this path hashes to root, else 0 -- ARK_HIP_OK either way. */
int ark_hip_merkle_leaf_sfp(int sfield, const void* row, size_t count, uint8_t out[32]);
int ark_hip_merkle_leaf_fr(int field, const uint64_t* row, size_t count, uint8_t out[32]);
int ark_hip_merkle_node(const uint8_t left[32], const uint8_t right[32], uint8_t out[32]);
int ark_hip_merkle_verify_sfp(int sfield, const uint8_t root[32], size_t n, uint64_t index, const void* row, size_t count,
                              const uint8_t* path, int* ok);
int ark_hip_merkle_verify_fr(int field, const uint8_t root[32], size_t n, uint64_t index, const uint64_t* row, size_t count,
                             const uint8_t* path, int* ok);
/* How a commit of (n, count, elem_bytes) runs, host only: out = { tree bytes, permutations per leaf, launches of a commit,
 * the level T from which one workgroup finishes the tree (it computes levels min(T, log2 n - 1) .. 0; level l holds 2^l nodes),
 * workgroups of the leaf launch, workgroups of the first multi-level node launch (0 without one), node levels per multi-level
 * launch, the permutation variant in force (0: the transcript's, 1: the one shaped for these kernels) }. */
int ark_hip_merkle_plan(size_t n, size_t count, unsigned elem_bytes, uint64_t out[8]);

/* ---- extension fields over the one-word fields, and FRI over them.  The extension fields are the reference's tower models over
 * SmallFp<P> (ff/src/fields/models/fp2.rs, fp4.rs, quadratic_extension.rs), so every output is a function of the field alone
 * and bit-exact:
 *   Goldilocks             Fp2 = Fp[u] / (u^2 - 7),                                  degree d = 2
 *   BabyBear / KoalaBear   Fp4 = Fp2[v] / (v^2 - u) over Fp2 = Fp[u] / (u^2 - W),    d = 4, W = 11 / 3
 *   With X = v the quartic field is Fp[X] / (X^4 - W), and (c0 = (a0, a1), c1 = (b0, b1)) is a0 + b0 X + a1 X^2 + b1 X^3.
 *   7, 11 and 3 are non-squares (Euler's criterion); all three primes are 1 mod 4, so X^4 - W is irreducible.
 *   Components, in memory and in every hash, in the order CanonicalSerialize writes them (quadratic_extension.rs:685-695):
 *   c0, c1 for Fp2 and c0.c0, c0.c1, c1.c0, c1.c1 for Fp4, each a stored Montgomery word of the base field.
 *   A single element crosses this interface as uint64_t[4], the upper two words zero for d = 2.
 * Extension vector: a d-column matrix in the layout of ark_hip_sfp_fft_batch_device and ark_hip_merkle_commit_sfp_device:
 *   component k of element i at element offset k * stride + i, stride >= n.  So the base-field transform with count = d is the
 *   extension's transform over a base-field domain; ark_hip_sfp_add / sub / neg / scale_device over the whole allocation are the
 *   extension's; the Merkle commit with count = d hashes header | serialize_compressed(element).  None needs a kernel of its own.
 * Fold: f holds n = 2^k evaluations in natural order over the coset D = { h w^i } (dom: group_gen w, offset h).  For
 *   log_arity a in 1 .. 3 and beta in the extension write f(X) = sum_{r < 2^a} X^r f_r(X^(2^a)); the fold is
 *   g = sum_r beta^r f_r as n / 2^a evaluations in natural order over D' = { h^(2^a) w^(2^a i) } (ark_hip_fri_folded_domain).
 *   a = 1, i < n / 2:   g[i] = (f[i] + f[i + n/2]) / 2 + beta (f[i] - f[i + n/2]) / (2 h w^i)
 *   arity 2^a equals a successive 2-folds with beta, beta^2, beta^4.
 *   Row i of a layer of size n at arity 2^a is the tuple f[i + j n / 2^a], j < 2^a.  A compact layer (stride = n) is also a
 *   matrix of d 2^a columns of n / 2^a rows with stride n / 2^a, column k 2^a + j holding component k of f[. + j n / 2^a];
 *   committing that view puts a whole row in one leaf, so one opening per layer answers a query.
 * EVERY vector argument of this family (d_*) is DEVICE memory and every call that takes one is ASYNCHRONOUS on the context
 * stream, as ark_hip_memcpy_d2d is -- except ark_hip_fri_commit_phase, which returns host results.  Challenges and constants are
 * read before the call returns.
 * ARK_HIP_ERR_ARG before any device is touched: an unknown sfield; a null pointer; log_arity outside 1 .. 3 or beyond the
 * domain's log size; a fold left without a level to take ((num_folds - 1) * log_arity >= log n: only the LAST fold may be
 * shorter); stride < n; a domain domain_check refuses (size != 2^log, an element >= p); a component >= p (or a non-zero upper
 * word at d = 2) in a constant; in and out of a fold or of combine_columns overlapping; the workspaces of the commit phase
 * overlapping layer 0 or each other, or not 16-byte aligned; a device pointer that is no multiple of the field's word.
 * ARK_HIP_ERR_NO_DEVICE from the device entries without a GPU. */
/* out = { d, W, W as stored, e_0, e_1, e_2, e_3, 0 }: component k is the coefficient of X^(e_k) in Fp[X] / (X^d - W).  Host only. */
int ark_hip_xfp_info(int sfield, uint64_t out[8]);
/* a * b, a^-1 (by the norm down the tower: one base-field inversion; 0 -> 0), a^exp.  Host only. */
int ark_hip_xfp_mul(int sfield, const uint64_t a[4], const uint64_t b[4], uint64_t out[4]);
int ark_hip_xfp_inverse(int sfield, const uint64_t a[4], uint64_t out[4]);
int ark_hip_xfp_pow(int sfield, const uint64_t a[4], uint64_t exp, uint64_t out[4]);
/* Pointwise on extension vectors of n elements (any n, 0 included); d_r may be d_a or d_b itself (the same pointer and stride).
 * inverse: a zero stays zero.  mul_const: by one extension element.  mul_base: by a base-field vector of n words. */
int ark_hip_xfp_vec_mul(int sfield, const void* d_a, size_t stride_a, const void* d_b, size_t stride_b, void* d_r, size_t stride_r,
                        size_t n);
int ark_hip_xfp_vec_inverse(int sfield, const void* d_a, size_t stride_a, void* d_r, size_t stride_r, size_t n);
int ark_hip_xfp_vec_mul_const(int sfield, const void* d_a, size_t stride_a, const uint64_t k[4], void* d_r, size_t stride_r, size_t n);
int ark_hip_xfp_vec_mul_base(int sfield, const void* d_a, size_t stride_a, const void* d_b, void* d_r, size_t stride_r, size_t n);
/* d_out[i] = alpha^first_power * sum_{j < count} alpha^j col_j[i], i < rows, over a base-field matrix (count >= 1 columns,
 * `stride` apart); d_out an extension vector.  accumulate != 0: added to what d_out holds, so several matrices chain with
 * first_power = the columns before them. */
int ark_hip_xfp_combine_columns(int sfield, const void* d_cols, size_t count, size_t stride, size_t rows, const uint64_t alpha[4],
                                uint64_t first_power, void* d_out, size_t stride_out, int accumulate);
/* The fold of one row through the function the kernel runs, host only: row[k * 2^a + j] = component k of f[index + j n / 2^a]
 * (the order of an opened row of the row view), index < n / 2^a. */
int ark_hip_fri_fold_row(int sfield, const ark_hip_sfp_radix2_domain* dom, unsigned log_arity, uint64_t index, const uint64_t* row,
                         const uint64_t beta[4], uint64_t out[4]);
/* D' of the fold: Radix2EvaluationDomain::new(n / 2^a).get_coset(h^(2^a)).  Host only. */
int ark_hip_fri_folded_domain(int sfield, const ark_hip_sfp_radix2_domain* dom, unsigned log_arity, ark_hip_sfp_radix2_domain* out);
/* The commit phase of 2^log_n elements with num_folds folds of log_arity levels (the last takes min(log_arity, what is left)),
 * host only.  out holds 8 + 5 (num_folds + 1) words:
 *   { d, layers = num_folds + 1, words of d_layers, bytes of d_trees, launches per fold, size of the last layer,
 *     word offset in d_layers of the last layer's interpolated copy, 0 },
 *   then per layer l = 0 .. num_folds: { log size, log arity of its fold (0: the last layer), word offset in d_layers (layer 0 is
 *   the caller's: 0), byte offset of its tree in d_trees, lo_bits of its fold's power table (i -> hi[i >> lo_bits] lo[i & mask]) }.
 * ARK_HIP_ERR_SIZE beyond the two-adicity. */
int ark_hip_fri_plan(int sfield, unsigned log_n, unsigned log_arity, unsigned num_folds, uint64_t* out);
/* d_out = the fold of d_in (dom->size elements over dom) by beta: dom->size >> log_arity elements.  One launch; the twiddles
 * (2 h w^i)^-1 come from the cached two-level power table of (size, group_gen_inv, (2 h)^-1), built by one more launch on first
 * use.  d_in is not written. */
int ark_hip_fri_fold(int sfield, const ark_hip_sfp_radix2_domain* dom, unsigned log_arity, const uint64_t beta[4], const void* d_in,
                     size_t stride_in, void* d_out, size_t stride_out);
/* The challenge of a layer from its root, on the calling thread: beta_out[4] as every element here; non-zero ends the phase. */
typedef int (*ark_hip_fri_next_beta)(void* user, const uint8_t root[32], uint64_t beta_out[4]);
/* The commit phase.  Layer 0 (d_layer0: compact, stride = dom->size, never written) is the caller's; layers 1 .. num_folds, the
 * interpolated copy of the last one and trees 0 .. num_folds - 1 go into d_layers and d_trees at the plan's offsets.  For each
 * l < num_folds: commit the row view of layer l (one wait, for the root), next_beta(user, root, beta), fold into layer l + 1.
 * The last layer is interpolated (the inverse coset transform with count = d, on a copy) and its d * size coefficient words, in
 * memory form, are written to out_final (HOST); the num_folds roots to out_roots (HOST).  A non-zero return of next_beta, or a
 * challenge that is no element, ends the phase with that code after a stream wait.  d_trees, next_beta and out_roots may be NULL
 * when num_folds = 0. */
int ark_hip_fri_commit_phase(int sfield, const ark_hip_sfp_radix2_domain* dom, unsigned log_arity, unsigned num_folds,
                             const void* d_layer0, void* d_layers, void* d_trees, ark_hip_fri_next_beta next_beta, void* user,
                             uint8_t* out_roots, void* out_final);

#ifdef ARK_HIP_TEST_HOOKS
/* ---- device-arithmetic test hooks (used by tests/ to check the kernels' field and point
 * arithmetic against the oracle; host pointers) ----
 * Exported by libark_hip_test.so ONLY (the same objects as libark_hip.so + csrc/capi_test.hip; `make` builds both): the shipped
 * library has no ark_hip_test_* symbol.  Declared when ARK_HIP_TEST_HOOKS is defined.
 * op: 0 add, 1 sub, 2 mul, 3 sqr, 4 neg, 5 dbl, 7 into_bigint, 8 from_bigint; 20 / 21 / 22: x y, x^2, 2 x y computed through
 * the carry-free 28-bit-limb form of the accumulate kernels (device product, square, sum of two products) */
int ark_hip_test_field_op(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* r, size_t n);
int ark_hip_test_basefield_op(int curve, int op, const uint64_t* a, const uint64_t* b, uint64_t* r, size_t n);
/* the same ops (0 add, 1 sub, 2 mul, 3 sqr, 4 neg, 5 dbl) through the HOST builds of the field arithmetic -- what the MSM's serial
 * tail runs on (64-bit limbs) -- on the calling thread: no GPU involved */
int ark_hip_test_host_basefield_op(int curve, int op, const uint64_t* a, const uint64_t* b, uint64_t* r, size_t n);
/* sw_check_point (csrc/pointcheck.cuh: the per-point function of ark_hip_sw_check_device) through its HOST build, on the calling
 * thread: no GPU involved.  status: n bytes. */
int ark_hip_test_host_sw_check(int curve, const uint64_t* bases_xy, size_t n, int checks, int method, uint8_t* status);
/* sw_decompress_point / sw_compress_point (csrc/pointcodec.cuh: the per-point functions of the codec kernels) through their HOST
 * builds, on the calling thread: no GPU involved.  status may be NULL. */
int ark_hip_test_host_sw_decompress(int curve, const uint8_t* bytes, size_t n, int validate, int method, uint64_t* points_xy, uint8_t* status);
int ark_hip_test_host_sw_compress(int curve, const uint64_t* points_xy, size_t n, uint8_t* bytes);
/* pv_chain_point / pv_add_point (csrc/pointvec.cuh: the per-lane functions of ark_hip_sw_mul_device / _fold_device / _add_device)
 * through their HOST builds, on the calling thread: no GPU involved.  Arguments as for the device entries, host pointers.
 * impl: 0 = the form the device entry runs by default (carry-free limbs for the G1 curves, saturated for G2), 1 = saturated. */
int ark_hip_test_host_sw_mul(int curve, const uint64_t* points, int form, const uint64_t* scalars, size_t n_scalars,
                             int scalars_are_montgomery, int impl, size_t n, uint64_t* out_xyz);
int ark_hip_test_host_sw_add(int curve, const uint64_t* a_xyz, const uint64_t* b_xyz, int negate_b, size_t n, uint64_t* out_xyz);
int ark_hip_test_host_sw_fold(int curve, const uint64_t* lo, const uint64_t* hi, int form, const uint64_t a[4], const uint64_t b[4],
                              int scalars_are_montgomery, int impl, size_t n, uint64_t* out_xyz);
/* the square root in the curve's coordinate field (Fp or Fp2, Montgomery form) on the device / through its host build:
 * out = the root r with r <= -r, or zero with ok = 0 */
int ark_hip_test_coord_sqrt(int curve, const uint64_t* in, uint64_t* out, uint8_t* ok, size_t n);
int ark_hip_test_host_coord_sqrt(int curve, const uint64_t* in, uint64_t* out, uint8_t* ok, size_t n);
/* kind: 2 bucket += affine, 3 bucket -= affine, 4 bucket += bucket, 5 bucket double, 6 bucket -> jacobian,
 * 7 affine double_to_bucket.  acc/other/out are arrays of n elements. */
int ark_hip_test_point_op(int curve, int kind, const uint64_t* acc, const uint64_t* other, uint64_t* out, size_t n);
/* test hook: msm_sharded's exchange with the ranks emulated in one process on one GPU (everything but the RCCL call): world
 * local MSMs, their part sums added on the device, one host tail -- or the fallback when the shards' plans differ.
 * *path: 1 = device-side sum of the part sums, 2 = fallback (finished partials summed on the host). */
int ark_hip_test_msm_sharded_emulated(int curve, int world, const void* const* d_bases, const void* const* d_scalars,
                                      const size_t* n_local, int scalars_are_montgomery, uint64_t* out_xyz, int* path);
/* HOST-ONLY test hook (no device needed): the serial tail of an MSM (ec/src/scalar_mul/variable_base/mod.rs:489-502, the
 * window combine) as msm_finish runs it.  parts: windows x (nbits + 1) bucket-form points (x | y | zz | zzz), row w =
 * U_(w,0) .. U_(w,nbits-1), A_w; widths: the windows' bit widths.  out = sum_w 2^(off_w) (A_w + 2^log2_l0 sum_b 2^b U_(w,b))
 * as a Projective (x | y | z). */
/* Host only: the verified cache's 128-bit tag of a buffer (keyed per process: equal only within one process). */
int ark_hip_test_base_hash(const uint64_t* p, size_t words, uint64_t out[2]);
int ark_hip_test_msm_host_fold(int curve, const uint64_t* parts, int windows, int nbits, int log2_l0, const int* widths,
                               uint64_t* out_xyz);
/* The same tail with the level-0 chunk length l0 itself (1 .. 65536, any integer):
 * out = sum_w 2^(off_w) (A_w + l0 sum_b 2^b U_(w,b)). */
int ark_hip_test_msm_host_fold_l0(int curve, const uint64_t* parts, int windows, int nbits, int l0, const int* widths,
                                  uint64_t* out_xyz);
/* HOST-ONLY test hook: the geometry of the bucket reduction (csrc/msm_plan.hpp, msm_reduce_geometry, every knob at its default)
 * for the plan (c window bits, W windows, the top `narrow` one bit narrower, shared: a prepared set) on `curve`;
 * resident_lanes: chunks the level-0 kernel keeps resident on the chip (0: unknown).
 * out = L0, m, mn, nbits, Q, two_digit, d2, rows2, nsum2, chunk, nchunks, npairs. */
int ark_hip_test_msm_reduce_geometry(int curve, int c, int W, int narrow, int shared, size_t resident_lanes, uint32_t out[12]);
/* HOST-ONLY test hook: the geometry of the MSM's partition sort, bucket order pass and heavy-run arrays (csrc/msm_plan.hpp,
 * msm_sort_geometry and msm_heavy_geometry) for n carried scalars under the plan (c, W, narrow, shared); W = 0: the window layout
 * of the curve's full-width scalars.  knobs[8] = c, hb, tile, heavy, groups, big_slices, compact, probe (MsmKnobs fields; the rest
 * at their defaults; no environment variable is read).
 * out = HB, LB, nsuper, tile, ntiles, nthist, lds_a, lds_b, stage_cap, big_on, big_region, noblk, nohist, nsums, mean_load,
 * forced_thresh, max_heavy, max_items, W, narrow, accepted (the call passes msm_enqueue's size checks), PART_LDS_WORDS,
 * PART_SCATTER_LDS_MAX, PART_BIG, SCAN_SMALL_MAX, HEAVY_CHUNK, SCAN_TILE, ORDER_TILE, ORDER_BINS, window groups, 0, 0. */
int ark_hip_test_msm_sort_geometry(int curve, size_t n, int c, int W, int narrow, int shared, const int32_t knobs[8], uint64_t out[32]);
/* The integer stages of one plain MSM call -- width probe, plan, zero-scalar compaction, digit recoding, the partition sort and
 * order pass of every window group, the heavy-run list -- run through the stage functions msm_enqueue runs, synchronised and
 * copied out.  No bases, no accumulation; no job slot stays busy.  scalars: 32-byte field elements (sbytes = 0, sbits = 0) or
 * sbytes-byte unsigned integers with sbits significant bits (0: all), in device (on_device) or host memory.  knobs: as above.
 * header[32] = c, W, narrow, n_carried, compacted, ngroups, HB, LB, tile, ntiles, nthist, stage_cap, big_on, shift, HEAVY_CHUNK,
 * PART_BIG, max_heavy, max_items, noblk, nsums, lds_a, lds_b, SCAN_SMALL_MAX, n; from word 24, per window group: w0, Wg, nslots,
 * nbk_g.  out = NULL: the header only.  Otherwise nine arrays of u32 words with their capacities in words (cap_words): keys
 * [W][n_carried]; cidx [n_carried] and the compacted scalars [n_carried][8] (when compacted; else may be NULL); sorted
 * [W][n_carried] (group g from word w0 n_carried; 0xffffffff where the sort wrote nothing); offsets (group g: nslots + 1 words
 * from word (w0 << (c - 1)) + g); order (group g from word w0 << (c - 1)); hctr [16]; hlist (3 words per heavy run: bucket,
 * first_item, items; group 0's, then group 1's); hitems (2 words per chunk item, likewise).  ARK_HIP_ERR_SIZE when a capacity is
 * too small: nothing is ever written short. */
int ark_hip_test_msm_sort_stages(int curve, const void* scalars, int on_device, size_t n, int mont, int sbytes, int sbits,
                                 const int32_t knobs[8], uint64_t header[32], void* const* out, const size_t* cap_words);
/* One MSM run as explicit pieces that share one plan and one bucket array (csrc/msm_piece_dump.cuh), through the msm_enqueue /
 * msm_finish the streamed host-pointer entry runs for each of its pieces; the bucket array is copied out behind every piece.
 * bases (affine x|y) and scalars (32 bytes each): the n pairs, in device memory (on_device) or host memory; sizes[npieces],
 * 1 <= npieces <= 16, none zero, summing to n (one piece: a first-and-last piece).  The plan is the streamed entry's under
 * knobs[12] = c, heavy, hb, probe, compact, lazy, tile, big_slices, prepared, 0, 0, 0 -- no environment variable is read;
 * prepared != 0 hands the plan to msm_enqueue as a prepared set's as well, which a piece refuses: ARK_HIP_ERR_ARG.
 * header (u64 words): c, W, narrow, nbuckets, bytes of a stored XYZZ point, npieces, pieces run, the piece whose scalars were
 * out of range (else ~0), the reduction's L0, m, mn, nbits, Q, two_digit, npairs, lazy; from word 16, four per piece: HB, LB, n,
 * window groups.  hctr_out = NULL: the header only.  Otherwise piece k's 16 counter words (u32) go to hctr_out + 16 k and the
 * nbuckets points behind piece k to buckets_out + k * nbuckets * point bytes; ARK_HIP_ERR_SIZE when a capacity (words / bytes)
 * is too small, before anything is written.  out_xyz: the result, written behind the last piece.  ARK_HIP_ERR_SCALAR_RANGE
 * names the piece in the header; no later piece is enqueued.  On return lane 0 is idle and no job slot is taken. */
int ark_hip_test_msm_pieces(int curve, const void* bases, const void* scalars, int on_device, size_t n, int mont, const size_t* sizes,
                            int npieces, const int32_t knobs[12], uint64_t header[80], uint32_t* hctr_out, size_t hctr_cap_words,
                            void* buckets_out, size_t buckets_cap_bytes, uint64_t* out_xyz);
/* The carry-free limb arithmetic (csrc/fp28.cuh, fp28x2.cuh, fft.cuh Fft29) ONE OP AT A TIME ON RAW LIMBS: lane t reads `arity`
 * slots of L words (u32[L]: the W-bit limbs as the test chose them, not canonical words) at in[(t * arity + j) * L] and writes
 * L + 1 words at out[t * (L + 1)] (word L: the op's boolean result).  The Fp2L ops (op >= 40; field = BLS12-381 / BLS12-377 Fq)
 * own a lane pair per element: even lane c0, odd lane c1, n even.  op, arity and the (k, h) template parameters served are
 * THE TABLE of csrc/lazytest_api.hpp -- exactly those of the kernels' call sites; anything else is ARK_HIP_ERR_ARG. */
int ark_hip_test_lazy_raw_op(int field, int op, int k, int h, const uint32_t* in, uint32_t* out, size_t n);
/* The bucket additions on carry-free limbs with the accumulator in the PARKED layout of LazyK::park / unpark (4 L + 1 words; G2:
 * 8 L + 1 per lane pair) on both sides.  kind (csrc/lazytest_api.hpp AccKind): 0 / 1 acc +/- affine base (other: x | y), 2 / 3
 * acc = +/- 2 base, 4 acc += stored bucket (other: canonical XYZZ), 5 acc += parked accumulator, 6 acc = 2 acc,
 * 7 from_bucket (acc: canonical XYZZ), 8 to_bucket (out: canonical XYZZ). */
int ark_hip_test_lazy_acc_op(int curve, int kind, const void* acc, const void* other, void* out, size_t n);
/* The signed 13 x 30-bit arithmetic of the plain accumulate kernel of BLS12-381 G1 (csrc/fp30s.cuh, ec30s.cuh) ONE OP AT A TIME
 * ON RAW DIGITS: lane t reads in_words(op) int32 words and writes out_words(op) (csrc/s30test_api.hpp: a field element is a slot of
 * 13 signed digits as the test chose them, a canonical element the first 12 words of a slot).  op: 0 mul, 1 sqr, 2 sop2, 3 sub,
 * 4 add_2b, 5 from_canonical_shl, 6 to_canonical, 7 the mixed addition on a parked accumulator (4 x 13 digits + the infinity
 * flag | base x | base y -> accumulator | "equal points"); anything else is ARK_HIP_ERR_ARG. */
int ark_hip_test_s30_op(int op, const void* in, void* out, size_t n);
/* The RELAXED arithmetic on saturated 32-bit limbs (csrc/fp.cuh: residues in [0, 2p), Fp, Fp2, Fp2Half) ONE OP AT A TIME ON RAW
 * LIMBS: lane t reads `arity` slots of N words (N = 8 or 12: whatever representative the test chose) at in[(t * arity + j) * N]
 * and writes N + 1 words at out[t * (N + 1)]: the limbs as the function returns them, then its boolean result.  The Fp2 and
 * Fp2Half ops (op >= 20; field = BLS12-381 / BLS12-377 Fq) own a lane pair per element: even lane c0, odd lane c1, n even.  op,
 * arity and the fields an op is served on are THE TABLE of csrc/relaxtest_api.hpp; anything else is ARK_HIP_ERR_ARG. */
int ark_hip_test_relaxed_raw_op(int field, int op, const uint32_t* in, uint32_t* out, size_t n);
/* The XYZZ additions on relaxed residues (csrc/ec.cuh) over the field of the bucket kernels (Fp; G2: Fp2Half, a lane pair per
 * point), the accumulator in and out as raw limbs (x | y | zz | zzz).  kind (csrc/relaxtest_api.hpp AccKind): 0 xyzz_madd_relaxed
 * (other: x2 | y2, y2 as given), 1 xyzz_add_relaxed (other: XYZZ), 2 xyzz_canonical. */
int ark_hip_test_relaxed_acc_op(int curve, int kind, const void* acc, const void* other, void* out, size_t n);
/* ---- what survives between calls: poison for the scratch buffers, a canary in their slack (csrc/scratch_list.hpp) ----
 * The device workspaces live as long as the process and only grow; no call may read a cell it did not write, and no kernel may
 * write past what its enqueue asked for.  ark_hip_test_scratch_poison fills the WHOLE capacity of every scratch buffer of the
 * calling thread's device, and the pinned staging areas, with `word`, remembers where each buffer stands and resets the
 * high-water mark of the requests; ARK_HIP_ERR_ARG while an MSM job is in flight.  ark_hip_test_scratch_report gives one row per
 * buffer: regrown (the buffer moved since the poison, or did not exist then), and the bytes of [asked, cap) that no longer
 * hold the poison with the offset of the first (~0 if none).  *n_rows: the number of rows; ARK_HIP_ERR_SIZE (nothing written)
 * when cap_rows is smaller.  ark_hip_test_scratch_selfcheck runs no product kernel: 0 when an unwritten poisoned cell reads
 * back as the poison and four bytes it plants in stage_c's slack are reported as exactly that; else the failing step (> 0). */
typedef struct ark_hip_scratch_row {
  char name[40];
  uint64_t cap, asked, regrown, dirty_beyond, first_dirty_offset;
} ark_hip_scratch_row;
int ark_hip_test_scratch_poison(uint32_t word);
int ark_hip_test_scratch_report(uint32_t word, ark_hip_scratch_row* rows, size_t cap_rows, size_t* n_rows);
int ark_hip_test_scratch_selfcheck(void);
/* The transcript (csrc/transcript.cuh) piece by piece: the 512-bit reduction of 64 little-endian bytes alone, on the host or
 * (on_device) in a one-lane kernel; and the whole challenge in a one-lane kernel, the counterpart of
 * ark_hip_transcript_challenge. */
int ark_hip_test_transcript_reduce(int field, const uint8_t* bytes64, int on_device, uint64_t* out);
int ark_hip_test_transcript_challenge_device(int field, uint8_t* state, const uint64_t* elements, unsigned count, uint64_t* out);
/* One side of a CSR handle read back array by array (transpose = 1: the M^T that ark_hip_fr_csr_create built, ARK_HIP_ERR_ARG
 * without the flag): dims = {rows, cols, nnz} of that side, always written; row_ptr (rows + 1), col_idx (nnz) and vals (nnz
 * elements) into HOST arrays of the given capacities, ARK_HIP_ERR_SIZE when one is too small; all three NULL: the sizes only.
 * Waits for the device. */
int ark_hip_test_csr_dump(const ark_hip_fr_csr* m, int transpose, size_t* dims, uint32_t* row_ptr, size_t row_ptr_cap,
                          uint32_t* col_idx, uint64_t* vals, size_t nnz_cap);
/* Host only, no device needed: the home slot of `element` (4 x u64) in a lookup table of 2^capacity_log slots, from the one hash
 * function the kernels of ark_hip_fr_lookup_device use (csrc/lookup_hash.hpp), so that a test can construct colliding tables
 * instead of hoping for them.  ARK_HIP_ERR_ARG for an unknown field, a null pointer or capacity_log outside 1 .. 29. */
int ark_hip_test_lookup_slot(int field, const uint64_t* element, unsigned capacity_log, uint32_t* slot);
/* ---- the asynchrony contract under a busy context stream (tests/test_gpu_async_contract.py) ----
 * ark_hip_test_context_busy: *busy = 1 while work enqueued on the calling thread's context stream has not finished
 * (hipStreamQuery; waits for nothing).  ark_hip_test_job_lane: the MSM lane (0 or 1) an *_async entry put the job on; host only.
 * ark_hip_test_producer_marks(0): from here on no entry records the event that orders the second MSM lane behind the context
 * stream's producers (process-wide, default on; (1) restores it) -- what a forgotten mark looks like, for the negative control. */
int ark_hip_test_context_busy(int* busy);
int ark_hip_test_job_lane(const ark_hip_msm_job* job, int* lane);
int ark_hip_test_producer_marks(int on);

#endif /* ARK_HIP_TEST_HOOKS */

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
