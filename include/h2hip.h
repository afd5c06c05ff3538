/*
 * libh2hip — C ABI of the MI355X (gfx950) prover backend for halo2-lib's proving hot path.
 *
 * This is the drop-in boundary: a `halo2_proofs`-compatible Rust crate selected through
 * halo2-lib's existing backend seam (reference halo2-base/src/lib.rs:25-28, the `halo2_base::halo2_proofs`
 * re-export toggled by a cargo feature exactly like `cuda`) binds these symbols where upstream
 * halo2-axiom 0.5.3 calls its CPU kernels.  INTEGRATION.md shows the `extern "C"` block and the call sites.
 *
 * Data formats (bit-identical to halo2curves' in-memory types; reference halo2-base/src/utils/mod.rs:28-38,
 * 342-377 and halo2-ecc/benches/msm.rs:62):
 *   Fr / Fq      4 x u64 little-endian limbs, MONTGOMERY form (R = 2^256)          32 B
 *   G1Affine     { Fq x; Fq y }, identity = all-zero bytes                         64 B
 *   G1 (curve)   { Fq x; Fq y; Fq z } Jacobian, identity has z = 0                 96 B
 *
 * Conventions: every function returns H2HIP_OK (0) or a negative H2HIP_ERR_* code and never throws or
 * aborts; h2hip_last_error() returns a thread-local message.  Host buffers stay caller-owned.  A context
 * serialises its work on one HIP stream; use it from one thread at a time (the reference calls
 * create_proof from a single thread, halo2-base/src/utils/testing.rs:32-50).  DIFFERENT contexts (each with its own
 * base sets and proving keys) may be used from different threads at the same time, also on one device: the library holds no
 * mutable global state (tests/test_plonk_prover.py::test_create_proof_gpu_three_contexts_in_flight).  There is NO CPU fallback:
 * without a usable HIP device h2hip_init fails with H2HIP_ERR_NO_DEVICE.
 *
 * Functions ending in `_dev` take device pointers (from h2hip_malloc, or any HIP allocation on the
 * context's device, e.g. a torch tensor's data_ptr) so polynomials can stay resident in HBM between calls;
 * the un-suffixed forms stage host buffers through the context's stream.
 */
#ifndef H2HIP_H
#define H2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H2HIP_OK 0
#define H2HIP_ERR_INVALID (-1)   /* bad argument (message says which) */
#define H2HIP_ERR_HIP (-2)       /* HIP runtime / kernel launch failure */
#define H2HIP_ERR_NOMEM (-3)
#define H2HIP_ERR_NO_DEVICE (-4)
#define H2HIP_ERR_PEER (-5)      /* another rank of a sharded (multi-GPU) call reported an error: every rank returns */

#define H2HIP_POINT_JACOBIAN 0   /* 96 B, what best_multiexp returns (C::Curve) */
#define H2HIP_POINT_AFFINE 1     /* 64 B, normalised on the device (one field inversion) */

#define H2HIP_BASES_PLAIN 0u
#define H2HIP_BASES_PRECOMPUTE 1u /* also store 2^(c*w)*P_i for every window: fixed-base (SRS) fast path */

typedef struct h2hip_ctx h2hip_ctx;
typedef struct h2hip_bases h2hip_bases;

/* ---- context ------------------------------------------------------------------------------------- */
const char *h2hip_last_error(void);
int h2hip_version(void);
int h2hip_device_count(int *count);
/* hip_stream: an existing hipStream_t to run on (NULL: the context creates its own). */
int h2hip_init(int device, void *hip_stream, h2hip_ctx **out);
void h2hip_destroy(h2hip_ctx *ctx);
int h2hip_sync(h2hip_ctx *ctx);
/* tuning knobs (defaults are the tuned values; every knob claims the same results at every legal value).  h2hip_set_param refuses a value
 * outside the knob's legal domain with H2HIP_ERR_INVALID and keeps the stored value.  Child contexts (batch lanes, the prover's side context)
 * take every knob from their parent except the batch driver's and create_proof's, which only the caller's context reads.  Legal values:
 * MSM: "msm_window_bits" 0 (auto) or 4..16, "msm_chunk" 0 (auto) or 2..4096 (entries per accumulation lane), "msm_chunk_lone" -1 (auto: a
 * lone MSM keeps the longer entries-per-lane rule, batch lanes the shorter one), 0 (the batch rule) or 1..4096, "msm_seg" a power of two
 * <= 1024 (buckets per running-sum segment), "msm_quad_tails" 0 / 1, "msm_quad_seg_max" >= 0 (quad-lane bucket reduction up to this many
 * segments), "msm_sort_threads" 256, 512 or 1024, "msm_sort_groups" 0 (auto = 32) or 1..1024 (chunks per window of the counting sort),
 * "msm_hist_split" 0 or a power of two <= 64 (0 / 1 = the whole window per histogram workgroup, else that many bucket sub-ranges, at most
 * the window's bucket count), "msm_hist_packed" 0 / 1 (r06, 1: the sort's LDS histogram as 16-bit counter pairs whenever a chunk holds
 * < 2^16 scalars), "msm_scatter_split" 0 (auto) or a power of two <= 64, "msm_scatter_full_lds" 0 / 1 (0: the scatter declares its cursors
 * only, so that it fits beside running accumulations), "msm_table_split" 0 / 1 (r05, 1: base sets uploaded / generated AFTER the call get
 * 128-byte table entries pre-split into 9 x 29-bit limbs);
 * the batch driver (h2hip_msm_g1_batch_dev / _multi_dev): "msm_lanes" 0 (auto) or 1..4, "msm_stagger_sorts" -1 (auto: two-lane batches),
 * 0 or 1 (a batch's lanes start their first sorts together / one behind the other), "msm_fuse_cols" 0 (auto) or 1..32, "msm_defer_reduce"
 * 0 / 1, "clean_on_lane" 0 / 1 (the bucket zero-fill on the first lane's stream);
 * NTT: "ntt_tile_bits" 4..10, "ntt_min_col_bits" 0..5 (at least 2^bits adjacent columns per tile, as far as the tile leaves room for one
 * stage), "ntt_full_table" 0 / 1, "ntt_tile_kernel" 0 / 1 (1 = the specialised full-tile pass kernel, 0 = the generic one);
 * arithmetic form of the pointwise kernels: "quotient_29", "kate_29" 0 / 1 (1 = unsaturated 9 x 29-bit limbs, 0 = the saturated kernels),
 * "kate_coeffs_per_lane" 0 (by length), 1, 2, 4 or 8, "fr_invert_run" 0 (auto) or 1..1024, "lookup_big_tile_bits" 12..28;
 * r05: "host_poll" 0 / 1 (1: results of a round come back through a host-mapped flag instead of hipMemcpyAsync + hipStreamSynchronize);
 * the prover's scheduling, all 0 / 1 and the same proof bytes either way: "plonk_tail_overlap", "plonk_side_on_lanes",
 * "plonk_permute_in_commit", "plonk_warm_keygen", "plonk_merge_products" (1: one batched inversion / prefix product for the permutation set
 * and the lookups when nothing chains), "plonk_early_intt" (1: the grand products' lagrange_to_coeff is queued on the side context in front
 * of their commitment round), "plonk_gate_before_join" (0; 1: the quotient's gate identities start before the grand products' transforms
 * are joined — measured neutral), "plonk_lazy_upload" (1: host-resident advice columns 1.. are uploaded inside round 1's commitment batch,
 * each right before its MSM is queued), "plonk_route_rows" (1: sharded proofs route the grand products' rows to the column owners by
 * h2hip_comm_alltoall_dev instead of all-gathering them; every rank of a sharded proof must use the same value); "plonk_shard_side" 0, 1
 * or 2 (1: sharded proofs run the first-round columns' transforms and all-gather on a side stream where the transport allows it, 2: always);
 * profiling aid: "ntt_debug_skip" 0, 1 or 2 (produces wrong results).  The variants r01-r03 measured slower (two-level sort, bucket-major
 * sort, split streams, split windows, accumulation builds 2/5/6/7, radix-8 and wave-local NTT passes) were removed in r04, r05's (two-wave
 * accumulation, sort-first batches, split lone commitments) in r05, r05's wave-owned radix-8 NTT pass ("ntt_w8") and the 48-byte NTT tile
 * layout in r06 (tools/probes/); their A/B logs stay under profiles/. */
int h2hip_set_param(h2hip_ctx *ctx, const char *name, int value);
int h2hip_get_param(h2hip_ctx *ctx, const char *name, int *value);

/* ---- device memory (for callers without a HIP runtime of their own, e.g. the Rust shim) ----------- */
int h2hip_malloc(h2hip_ctx *ctx, size_t bytes, void **dptr);
int h2hip_free(h2hip_ctx *ctx, void *dptr);
int h2hip_upload(h2hip_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);   /* synchronous */
int h2hip_download(h2hip_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes); /* synchronous */
/* page-lock / release a caller-owned host buffer (a prover's long-lived Vec<Fr> columns): transfers from registered memory are true
 * asynchronous DMA; unregistered (pageable) buffers work everywhere too, through the runtime's staging copies */
int h2hip_host_register(h2hip_ctx *ctx, void *host_ptr, size_t bytes);
int h2hip_host_unregister(h2hip_ctx *ctx, void *host_ptr);

/* ---- per-kernel timing (HIP events on the context's stream around every launch) ------------------- */
int h2hip_profile_enable(h2hip_ctx *ctx, int on);
int h2hip_profile_reset(h2hip_ctx *ctx);
/* restrict the event brackets to kernels whose name starts with `prefix` (NULL or "" = all): a timed region can then carry the dominant
 * kernel's events only (two events per launch cost ~1 us each; a k = 19 proof has ~200 launches) */
int h2hip_profile_filter(h2hip_ctx *ctx, const char *prefix);
/* total milliseconds and launch count accumulated for kernels whose name starts with `prefix` */
int h2hip_profile_get(h2hip_ctx *ctx, const char *prefix, double *total_ms, uint64_t *launches);
/* milliseconds (since the last h2hip_profile_reset) during which at least one launch of the matching kernels was executing:
 * the union of the launch spans — with pipelined MSMs several launches of one kernel overlap */
int h2hip_profile_get_busy(h2hip_ctx *ctx, const char *prefix, double *busy_ms);
/* the whole account since the last reset as text, one "name total_ms launches busy_ms" line per kernel name (NUL-terminated, truncated at
 * cap; *needed = bytes for all of it) — what bench.py turns into the per-kernel table of a create_proof */
int h2hip_profile_dump(h2hip_ctx *ctx, char *out, size_t cap, size_t *needed);
/* bracket an arbitrary region with events on the context's stream (bench.py's timed region) */
int h2hip_timer_start(h2hip_ctx *ctx);
int h2hip_timer_stop(h2hip_ctx *ctx, double *elapsed_ms);

/* ---- K1: multi-scalar multiplication  (replaces arithmetic::best_multiexp [UPSTREAM], reached from the
 *      reference via ParamsKZG::commit / commit_lagrange inside create_proof,
 *      halo2-base/src/utils/testing.rs:40-47) ------------------------------------------------------- */
/* Upload n G1Affine bases once (the SRS `g` or `g_lagrange` of ParamsKZG, reference
 * halo2-base/src/utils/mod.rs:401-443); they stay resident in HBM. */
int h2hip_bases_upload(h2hip_ctx *ctx, const void *g1_affine_host, size_t n, uint32_t flags, h2hip_bases **out);
int h2hip_bases_from_device(h2hip_ctx *ctx, const void *g1_affine_dev, size_t n, uint32_t flags, h2hip_bases **out);
void h2hip_bases_free(h2hip_ctx *ctx, h2hip_bases *bases);
size_t h2hip_bases_len(const h2hip_bases *bases);
/* out = sum_{i<n} scalars[i] * bases[i];  n <= h2hip_bases_len.  point_format selects 96 B Jacobian or 64 B affine. */
int h2hip_msm_g1(h2hip_ctx *ctx, const h2hip_bases *bases, const void *scalars_host, size_t n, int point_format, void *out_host);
int h2hip_msm_g1_dev(h2hip_ctx *ctx, const h2hip_bases *bases, const void *scalars_dev, size_t n, int point_format, void *out_host);

/* `count` independent MSMs over the same bases (all advice columns of a phase, the pieces of h(X), ...).
 * scalars_dev: host array of `count` device pointers, n scalars each; out_host: `count` points.  The MSMs are
 * pipelined over the context's lanes ("msm_lanes" internal streams; default: chosen by size) so that one MSM's sort and latency-bound tail
 * overlap another one's accumulation.  With precomputed tables, columns of up to 2^17 scalars are FUSED into multi-column MSMs of about
 * 2^19 scalars (up to 16 columns share every launch), and the latency-bound bucket reduction is deferred: it runs once per 64 columns of
 * the batch after the lanes have joined. */
int h2hip_msm_g1_batch_dev(h2hip_ctx *ctx, const h2hip_bases *bases, const void *const *scalars_dev, size_t n, size_t count,
                           int point_format, void *out_host);
/* the same with a base set PER COLUMN: the commitments of one prover round that live over different SRS columns (Lagrange-basis and
 * monomial-basis polynomials) in one pipelined call.  The sets must share their table layout (all plain, or all precomputed with the same
 * window — true for the g / g_lagrange of one ParamsKZG). */
int h2hip_msm_g1_multi_dev(h2hip_ctx *ctx, const h2hip_bases *const *bases_per_column, const void *const *scalars_dev, size_t n, size_t count,
                           int point_format, void *out_host);
/* the same for scalar columns in HOST memory (an unmodified prover's Vec<Fr>): each column is uploaded on its lane's stream
 * right before its kernels are queued, so the upload of column j+1 overlaps the GPU work of column j */
int h2hip_msm_g1_batch(h2hip_ctx *ctx, const h2hip_bases *bases, const void *const *scalars_host, size_t n, size_t count, int point_format,
                       void *out_host);

/* MSM over G2 (the twist over Fq2).  The reference holds G2 elements only as the verifier half of ParamsKZG (g2, s*g2) and has no
 * prover-side G2 commitment: supported for completeness (8-bit windows, per-bucket lanes), not tuned like the G1 path.
 * points: n x 128 B affine (x.c0, x.c1, y.c0, y.c1 Montgomery limbs; identity all-zero); out: 128 B affine. */
int h2hip_msm_g2(h2hip_ctx *ctx, const void *g2_affine_host, const void *scalars_host, size_t n, void *out_affine_host);
int h2hip_msm_g2_dev(h2hip_ctx *ctx, const void *g2_affine_dev, const void *scalars_dev, size_t n, void *out_affine_host);

/* ---- a2: KZG SRS (ParamsKZG::<Bn256>::setup [UPSTREAM]; reference gen_srs halo2-base/src/utils/mod.rs:439-443,
 *      halo2-base/benches/mul.rs:39).  g[i] = s^i*G1 and g_lagrange[i] = L_i(s)*G1 for i < 2^k are generated on
 *      the GPU (fixed-base window tables) and stay resident as two base sets; `flags` as in h2hip_bases_upload.
 *      The G2 half (g2, s*g2) is verifier-side and stays with the host library. --------------------------- */
int h2hip_params_kzg_setup(h2hip_ctx *ctx, uint32_t k, const void *s_fr, uint32_t flags, h2hip_bases **g_out, h2hip_bases **g_lagrange_out);
/* g_to_lagrange [UPSTREAM poly/kzg/commitment.rs]: Lagrange-basis SRS from the monomial one, g_lagrange[i] = n^-1 * sum_j
 * omega^(-ij) * g[j] with n = 2^k (group-element inverse FFT on the device) — for SRS sources that carry only g
 * (ceremony files, ParamsKZG::from_parts(.., None, ..), downsize).  Uses the first 2^k bases of g. */
int h2hip_g1_to_lagrange(h2hip_ctx *ctx, const h2hip_bases *g, uint32_t k, uint32_t flags, h2hip_bases **g_lagrange_out);
/* out[i] = scalars[i] * base for a fixed G1Affine base (host pointer); scalars and out are device arrays */
int h2hip_g1_fixed_base_mul_batch_dev(h2hip_ctx *ctx, const void *base_affine, const void *scalars_dev, size_t n, void *out_affine_dev);
/* copy the resident affine points back to the host (n x 64 B) — ParamsKZG::write / tests */
int h2hip_bases_download(h2hip_ctx *ctx, const h2hip_bases *bases, void *out_host);

/* SRS files (ParamsKZG::read / gen_srs, reference halo2-base/src/utils/mod.rs:401-443).  RawBytes files carry 64-byte Montgomery points:
 * validate counts the entries that are not canonical on-curve points (the identity (0,0) is allowed).  Processed files carry 32-byte
 * compressed points: decompress fails with H2HIP_ERR_INVALID on any malformed encoding.  sign_bit / inf_bit: positions of the y-sign and
 * identity flags in the top byte (6 / 7 in halo2curves' encoding). */
int h2hip_g1_validate_dev(h2hip_ctx *ctx, const void *points_dev, size_t n, size_t *invalid);
int h2hip_g1_decompress_batch_dev(h2hip_ctx *ctx, const void *compressed_dev, size_t n, void *out_affine_dev, uint32_t sign_bit, uint32_t inf_bit);
/* The verifier's decompressor: one verdict per point, because a malformed proof is a rejection and not an error.
 * words_dev: 32-byte words; point i is words_dev[slots_dev ? slots_dev[i] : i] in halo2curves' compressed encoding (sign bit 6, identity bit 7).
 * out_affine_dev[i] = the Montgomery G1Affine, status_dev[i] (uint32) = 0 ok, 1 the identity encoding, 2 malformed (non-canonical x, not on the
 * curve, flag bits inconsistent); out is (0,0) for status != 0.  Never fails on account of the data.  Every slot must lie inside words_dev. */
int h2hip_g1_decompress_checked_dev(h2hip_ctx *ctx, const void *words_dev, const uint32_t *slots_dev, size_t n, void *out_affine_dev, uint32_t *status_dev);

/* Sum of n Jacobian points resident on the device (multi-GPU: the all-gathered per-GPU partial MSM results;
 * RCCL has no group-law reduction). */
int h2hip_g1_sum_jacobian_dev(h2hip_ctx *ctx, const void *points_dev, size_t n, int point_format, void *out_host);
/* the host half of a point-range sharded round: out[j] = sum_r gathered[r * count + j] over `world` ranks' Jacobian partials (the layout
 * h2hip_comm_allgather_host leaves), all `count` columns in one call, host arithmetic (no device round trip).  Output Jacobian (z in {0, 1}) or affine. */
int h2hip_g1_sum_partials_host(const void *gathered_jacobian, size_t world, size_t count, int point_format, void *out);

/* ---- K2/K3: NTT family  (replaces arithmetic::best_fft and EvaluationDomain::{ifft, coeff_to_extended,
 *      extended_to_coeff} [UPSTREAM]) ------------------------------------------------ */
/* in-place, natural order in and out, no scaling:  a[k] <- sum_j a[j] * omega^(jk),  len(a) = 2^log_n */
int h2hip_best_fft(h2hip_ctx *ctx, void *a_host, const void *omega, uint32_t log_n);
int h2hip_best_fft_dev(h2hip_ctx *ctx, void *a_dev, const void *omega, uint32_t log_n);
/* EvaluationDomain::ifft: best_fft with omega_inv, then every element times `divisor` (= 2^-log_n) */
int h2hip_ifft(h2hip_ctx *ctx, void *a_host, const void *omega_inv, uint32_t log_n, const void *divisor);
int h2hip_ifft_dev(h2hip_ctx *ctx, void *a_dev, const void *omega_inv, uint32_t log_n, const void *divisor);
/* EvaluationDomain::coeff_to_extended: out[0..2^ext_k) = NTT_{ext_omega}( coeffs[i] * zeta^(i mod 3), zero padded ) */
int h2hip_coeff_to_extended(h2hip_ctx *ctx, const void *coeffs_host, uint32_t k, void *out_host, uint32_t ext_k, const void *ext_omega,
                            const void *zeta);
int h2hip_coeff_to_extended_dev(h2hip_ctx *ctx, const void *coeffs_dev, uint32_t k, void *out_dev, uint32_t ext_k,
                                const void *ext_omega, const void *zeta);
/* ifft / coeff_to_extended over `count` equal-size columns at once (`cols_dev`, `coeffs_dev`, `outs_dev`: HOST arrays of device pointers):
 * 32 columns per kernel launch.  What create_proof does with every advice / permuted / product column (upstream transforms them one by
 * one on the CPU's thread pool, [UPSTREAM-RECALL plonk/prover.rs]); a wide halo2-base shape (bench_pairing.config: k = 14, 211 + 27 advice
 * columns) has ~400 columns of 2^14 rows, each far too small to fill the chip alone. */
int h2hip_ifft_batch_dev(h2hip_ctx *ctx, void *const *cols_dev, size_t count, const void *omega_inv, uint32_t log_n, const void *divisor);
int h2hip_coeff_to_extended_batch_dev(h2hip_ctx *ctx, const void *const *coeffs_dev, uint32_t k, void *const *outs_dev, uint32_t ext_k, size_t count,
                                      const void *ext_omega, const void *zeta);
/* EvaluationDomain::extended_to_coeff (without the final truncation, which is a length change on the
 * caller's Vec): in-place iNTT with ext_omega_inv, times ext_divisor, times [1, zeta_inv, zeta_inv^2][i mod 3]
 * (zeta_inv = zeta^2 because zeta^3 = 1) */
int h2hip_extended_to_coeff(h2hip_ctx *ctx, void *a_host, uint32_t ext_k, const void *ext_omega_inv, const void *ext_divisor,
                            const void *zeta_inv);
int h2hip_extended_to_coeff_dev(h2hip_ctx *ctx, void *a_dev, uint32_t ext_k, const void *ext_omega_inv, const void *ext_divisor,
                                const void *zeta_inv);

/* ---- K8: witness-column F_r batches (halo2-base GateInstructions add/sub/mul/mul_add on column values,
 *      reference halo2-base/src/gates/flex_gate/mod.rs:158-277); out may alias an input ----------------- */
int h2hip_fr_add_batch_dev(h2hip_ctx *ctx, void *out_dev, const void *a_dev, const void *b_dev, size_t n);
int h2hip_fr_sub_batch_dev(h2hip_ctx *ctx, void *out_dev, const void *a_dev, const void *b_dev, size_t n);
int h2hip_fr_mul_batch_dev(h2hip_ctx *ctx, void *out_dev, const void *a_dev, const void *b_dev, size_t n);
int h2hip_fr_mul_add_batch_dev(h2hip_ctx *ctx, void *out_dev, const void *a_dev, const void *b_dev, const void *c_dev, size_t n);
/* polynomial linear combinations (Polynomial * F and += of scaled polynomials in the multiopen argument):
 * y[i] += a * x[i]   and   y[i] *= s ; a, s: host pointers to one Montgomery Fr */
int h2hip_fr_axpy_dev(h2hip_ctx *ctx, void *y_dev, const void *a, const void *x_dev, size_t n);
int h2hip_fr_scale_dev(h2hip_ctx *ctx, void *y_dev, const void *s, size_t n);
/* y[i] = s * y[i] + a * x[i]  (Horner steps over polynomial pieces, e.g. h(X) = sum_i x^(n i) h_i(X)) */
int h2hip_fr_axpby_dev(h2hip_ctx *ctx, void *y_dev, const void *s, const void *a, const void *x_dev, size_t n);
/* out[i] = sum_j coeffs[j] * polys[j][i]: `polys` a HOST array of `count` device columns, `coeffs` `count` host Fr; every operand is read
 * once per 15 terms (the multiopen argument's sum_j y^j P_j(X) per rotation set and its linearisation
 * [UPSTREAM-RECALL poly/kzg/multiopen/shplonk/prover.rs]; `out` may be one of the operands). count = 0 gives zeros. */
int h2hip_fr_linear_combination_dev(h2hip_ctx *ctx, void *out_dev, const void *const *polys_dev, const void *coeffs_host, size_t count, size_t n);
/* y[i] -= low[i] for i < m <= 8 (`low_host`: m elements): P(X) - r(X) for the low-degree interpolant r of an opening set */
int h2hip_fr_sub_low_dev(h2hip_ctx *ctx, void *y_dev, const void *low_host, uint32_t m);

/* ---- K4: BatchInvert, in place, 0 -> 0 (ff::BatchInvert / batch_invert_assigned [UPSTREAM]; the deferred
 *      denominators come from reference halo2-base/src/gates/flex_gate/mod.rs:677-681,791-795) ---------- */
int h2hip_fr_batch_invert_dev(h2hip_ctx *ctx, void *a_dev, size_t n);

/* a5/a6: advice cells arrive as Assigned<F> — Trivial values and Rational(num, den) with the inversion deferred (reference
 * halo2-base/src/gates/flex_gate/mod.rs:677-681,791-795; columns laid out by threads/single_phase.rs:273-312).  out = num * den^-1
 * with 0^-1 := 0 (batch_invert_assigned [UPSTREAM]); Trivial cells carry den = 1.  out may alias den. */
int h2hip_assigned_resolve_dev(h2hip_ctx *ctx, void *out_dev, const void *num_dev, const void *den_dev, size_t n);

/* ---- K5: permutation / lookup grand products: out[i] = prod_{j<=i} in[j], and
 *      z[0] = 1, z[i+1] = z[i]*num[i]/den[i] (z has n+1 elements) ---------------------------------------- */
int h2hip_fr_prefix_product_dev(h2hip_ctx *ctx, void *out_dev, const void *in_dev, size_t n);
int h2hip_fr_grand_product_dev(h2hip_ctx *ctx, void *z_dev, const void *num_dev, const void *den_dev, size_t n);
/* `segments` grand products of seg_len factors each in a handful of launches (one batched inversion, one segmented prefix product):
 * num_dev / den_dev hold the factors of all segments back to back, z_dev (HOST array of device pointers) receives seg_len + 1 values per
 * segment.  chained != 0: z[s][0] = z[s-1][seg_len], z[0][0] = 1 — the sets of the permutation argument, whose chain then needs neither a
 * host round trip nor a rescaling pass; chained == 0: every z[s][0] = 1 — the lookup arguments of one proof. */
int h2hip_fr_grand_products_dev(h2hip_ctx *ctx, void *const *z_dev, const void *num_dev, const void *den_dev, size_t segments, size_t seg_len,
                                int chained);

/* factors of ONE permutation set's grand product over rows [0, rows) (columns = the equality-enabled columns of
 * halo2-base's configs, flex_gate/mod.rs:69,124-128, range/mod.rs:104):  num[i] = prod_j (v_j[i] + beta*delta^(first_col_index+j)*omega^i
 * + gamma),  den[i] = prod_j (v_j[i] + beta*sigma_j[i] + gamma);  cols / sigmas: host arrays of ncols (<= 8) device pointers.
 * z = h2hip_fr_grand_product_dev(num, den), scaled by the previous set's last value.  One set of the _sets_dev form below: the same
 * kernels, on unsaturated limbs or saturated as the knob quotient_29 says. */
int h2hip_permutation_product_terms_dev(h2hip_ctx *ctx, void *num_dev, void *den_dev, const void *const *cols_dev, const void *const *sigmas_dev,
                                        uint32_t ncols, uint32_t first_col_index, size_t rows, const void *beta, const void *gamma, const void *delta,
                                        const void *omega);
/* every set of the permutation argument at once: set s owns columns [s*chunk_len, (s+1)*chunk_len) of cols_dev / sigmas_dev (HOST arrays of
 * num_columns device pointers) and writes rows [s*rows, (s+1)*rows) of num_dev / den_dev — the layout h2hip_fr_grand_products_dev reads */
int h2hip_permutation_product_terms_sets_dev(h2hip_ctx *ctx, void *num_dev, void *den_dev, const void *const *cols_dev, const void *const *sigmas_dev,
                                             uint32_t num_columns, uint32_t chunk_len, size_t rows, const void *beta, const void *gamma,
                                             const void *delta, const void *omega);
/* ... restricted to the rows [row0, row0 + rows) of the (full-length) columns: num / den hold `rows` factors per set (the sharded prover's rank
 * forms the factors of its row range only) */
int h2hip_permutation_product_terms_rows_dev(h2hip_ctx *ctx, void *num_dev, void *den_dev, const void *const *cols_dev, const void *const *sigmas_dev,
                                             uint32_t num_columns, uint32_t chunk_len, size_t row0, size_t rows, const void *beta, const void *gamma,
                                             const void *delta, const void *omega);
/* factors of a lookup's grand product: num[i] = (a[i]+beta)(s[i]+gamma), den[i] = (a'[i]+beta)(s'[i]+gamma) */
int h2hip_lookup_product_terms_dev(h2hip_ctx *ctx, void *num_dev, void *den_dev, const void *a_dev, const void *s_dev, const void *a_perm_dev,
                                   const void *s_perm_dev, size_t rows, const void *beta, const void *gamma);

/* ---- K7: arithmetic::eval_polynomial and arithmetic::kate_division [UPSTREAM] ------------------------- */
int h2hip_fr_eval_polynomial_dev(h2hip_ctx *ctx, const void *coeffs_dev, size_t n, const void *x, void *out_host);
/* `count` evaluations in one pass: out[j] = poly_j(points[j]); coeffs_dev / lens: host arrays of device pointers and lengths, points: count
 * Montgomery elements (host), out_host: count elements — the prover's whole evaluation round with one synchronisation */
int h2hip_fr_eval_polynomial_batch_dev(h2hip_ctx *ctx, const void *const *coeffs_dev, const size_t *lens, const void *points, size_t count,
                                       void *out_host);
/* q[0..n-1) = (f(X) - f(b)) / (X - b); q_dev must not alias coeffs_dev */
int h2hip_fr_kate_division_dev(h2hip_ctx *ctx, void *q_dev, const void *coeffs_dev, size_t n, const void *b);

/* q[0..n-1) = sum_j weights[j] * (f(X) - f(points[j])) / (X - points[j]) for m <= 8 points (host arrays of m elements).  With weights[j] =
 * 1 / prod_{i != j} (points[j] - points[i]) this is (f(X) - r(X)) / prod_j (X - points[j]), r the interpolant of f on the points: the
 * quotient of one SHPLONK rotation set in a single pass over f. */
int h2hip_fr_kate_division_multi_dev(h2hip_ctx *ctx, void *q_dev, const void *coeffs_dev, size_t n, const void *points, const void *weights, uint32_t m);
/* q[0..n-1) += the same sum (SHPLONK's v-weighted sum over the rotation sets: v^i folded into the weights, no pass of its own) */
int h2hip_fr_kate_division_multi_acc_dev(h2hip_ctx *ctx, void *q_dev, const void *coeffs_dev, size_t n, const void *points, const void *weights, uint32_t m);
/* ... and for `nsets` polynomials at once (coeffs_dev: host array of device pointers, all of n coefficients; set i has set_sizes[i] points / weights, taken
 * from the flat host arrays in order): q[0..n-1) (accumulate ? += : =) the sum over the sets — SHPLONK's v-weighted sum over its rotation sets in one call */
int h2hip_fr_kate_division_sets_dev(h2hip_ctx *ctx, void *q_dev, const void *const *coeffs_dev, size_t n, const void *points, const void *weights,
                                    const uint32_t *set_sizes, size_t nsets, int accumulate);
/* The same quotient for ONE COEFFICIENT RANGE [lo, lo + n) of f (the multi-GPU prover, where a rank holds the coefficient range of its SRS
 * slice): coeffs_dev = that range; carries[j] = sum_{i >= lo + n} f_i points[j]^(i - lo - n), i.e. what the ranges above contribute (the caller
 * assembles it from the other ranks' partial evaluations; zeros for the top range); q_dev[0..n) = the quotient's coefficients lo .. lo + n - 1. */
int h2hip_fr_kate_division_range_dev(h2hip_ctx *ctx, void *q_dev, const void *coeffs_dev, size_t n, const void *points, const void *weights,
                                     const void *carries, uint32_t m);

/* ---- K6: the halo2-base custom gate's term of the quotient numerator on the extended domain:
 *      acc[i] = acc[i]*y + q[i]*(a[i] + a[i+s]*a[i+2s] - a[i+3s]), s = 2^(ext_k-k)
 *      (gate q*(a+b*c-d) at rotations 0..3, reference halo2-base/src/gates/flex_gate/mod.rs:80-91).
 *      One column of the _batch_dev form: the same kernels, on unsaturated limbs or saturated as the knob quotient_29 says ----- */
int h2hip_quotient_flex_gate_dev(h2hip_ctx *ctx, void *acc_dev, const void *q_dev, const void *a_dev, uint32_t ext_k, uint32_t k,
                                 const void *y);

/* EvaluationDomain::divide_by_vanishing_poly: a[i] *= 1 / ((zeta * ext_omega^i)^n - 1) over the 2^ext_k extended-domain
 * evaluations (n = 2^k); the 2^(ext_k-k) distinct inverses are computed on the device. */
int h2hip_divide_by_vanishing_poly_dev(h2hip_ctx *ctx, void *a_dev, uint32_t ext_k, uint32_t k, const void *ext_omega, const void *zeta);

/* Lookup argument's five identities, folded in upstream's order: l0*(1-z); l_last*(z^2-z);
 * active*(z(wX)(a'+beta)(s'+gamma) - z(a+beta)(s+gamma)); l0*(a'-s'); active*(a'-s')(a'-a'(w^-1 X)); active = 1-(l_last+l_blind).
 * All arrays: 2^ext_k extended-domain evaluations (halo2-base's lookups: halo2-base/src/gates/range/mod.rs:131-150).
 * One lookup of h2hip_quotient_lookups_dev: the same kernels, on unsaturated limbs or saturated as the knob quotient_29 says. */
int h2hip_quotient_lookup_dev(h2hip_ctx *ctx, void *acc_dev, const void *z_dev, const void *a_dev, const void *s_dev, const void *a_perm_dev,
                              const void *s_perm_dev, const void *l0_dev, const void *l_last_dev, const void *l_blind_dev, uint32_t ext_k,
                              uint32_t k, const void *beta, const void *gamma, const void *y);
/* Terms of ONE permutation set, selected by `terms` and folded into acc by y in this order:
 *   H2HIP_PERM_FIRST    l0*(1 - z)                                   (upstream: first set only)
 *   H2HIP_PERM_LAST     l_last*(z^2 - z)                             (last set only)
 *   H2HIP_PERM_CHAIN    l0*(z - z_prev(w^last_rotation X))           (every set but the first; needs z_prev_dev)
 *   H2HIP_PERM_PRODUCT  active*(z(wX)*prod_j(p_j + beta*sigma_j + gamma) - z*prod_j(p_j + delta^(first_col_index+j)*beta*X + gamma))
 * with X = zeta*ext_omega^i, active = 1 - (l_last + l_blind).  Upstream's evaluate_h folds FIRST (set 0), LAST (last set),
 * CHAIN (sets 1..) and then PRODUCT (all sets) as four separate loops over the sets: issue one call per (loop, set) to
 * reproduce that order with several sets; a single-set argument is one call with FIRST|LAST|PRODUCT.
 * cols / sigmas: host arrays of ncols (<= 8) device pointers (only read for PRODUCT). */
#define H2HIP_PERM_FIRST 1u
#define H2HIP_PERM_LAST 2u
#define H2HIP_PERM_CHAIN 4u
#define H2HIP_PERM_PRODUCT 8u
int h2hip_quotient_permutation_set_dev(h2hip_ctx *ctx, void *acc_dev, const void *z_dev, const void *z_prev_dev, const void *const *cols_dev,
                                       const void *const *sigmas_dev, uint32_t ncols, uint32_t first_col_index, const void *l0_dev,
                                       const void *l_last_dev, const void *l_blind_dev, uint32_t ext_k, uint32_t k, uint32_t terms,
                                       int32_t last_rotation, const void *beta, const void *gamma, const void *delta, const void *zeta,
                                       const void *ext_omega, const void *y);
/* The same identities for all gate columns / all lookups / the whole permutation argument of a proof: every launch folds up to 64 gate
 * columns, 32 lookups or 12 (set, term) pairs into the accumulator in evaluate_h's order (acc = acc*y + term per identity, exactly the
 * values of one call per column / lookup / (loop, set)), reading and writing the accumulator once.  A wide halo2-base shape
 * (bench_pairing.config: k = 14, 211 gate columns, 80 permutation sets, 27 lookups) needs ~20 launches instead of ~400.
 * q/a, z/a/s/a_perm/s_perm, z/cols/sigmas: HOST arrays of device pointers; permutation_sets: set i owns columns [i*chunk_len, (i+1)*chunk_len)
 * of cols_dev / sigmas_dev (num_sets = ceil(num_columns / chunk_len), chunk_len <= 8), z_dev[i] is its grand product. */
int h2hip_quotient_flex_gate_batch_dev(h2hip_ctx *ctx, void *acc_dev, const void *const *q_dev, const void *const *a_dev, size_t count, uint32_t ext_k,
                                       uint32_t k, const void *y);
int h2hip_quotient_lookups_dev(h2hip_ctx *ctx, void *acc_dev, const void *const *z_dev, const void *const *a_dev, const void *const *s_dev,
                               const void *const *a_perm_dev, const void *const *s_perm_dev, size_t count, const void *l0_dev, const void *l_last_dev,
                               const void *l_blind_dev, uint32_t ext_k, uint32_t k, const void *beta, const void *gamma, const void *y);
int h2hip_quotient_permutation_sets_dev(h2hip_ctx *ctx, void *acc_dev, const void *const *z_dev, uint32_t num_sets, const void *const *cols_dev,
                                        const void *const *sigmas_dev, uint32_t num_columns, uint32_t chunk_len, const void *l0_dev,
                                        const void *l_last_dev, const void *l_blind_dev, uint32_t ext_k, uint32_t k, int32_t last_rotation,
                                        const void *beta, const void *gamma, const void *delta, const void *zeta, const void *ext_omega, const void *y);

/* permute_expression_pair of the lookup argument: a_perm = sort(a[..usable]); s_perm[i] = a_perm[i] on
 * run starts, the other rows take the unconsumed table elements (ascending) from the last repeated row backwards.
 * Rows >= usable_rows are left untouched (blinding).  H2HIP_ERR_INVALID if an input value is missing from the table. */
int h2hip_lookup_permute_dev(h2hip_ctx *ctx, const void *a_dev, const void *s_dev, size_t usable_rows, void *a_perm_dev, void *s_perm_dev);

/* The table of a lookup is a FIXED column: its sorted keys can be prepared once (keygen) and reused by every proof.
 * sorted_out_dev: h2hip_lookup_sorted_table_bytes(usable_rows) bytes of device memory. */
size_t h2hip_lookup_sorted_table_bytes(size_t usable_rows);
int h2hip_lookup_table_sort_dev(h2hip_ctx *ctx, const void *s_dev, size_t usable_rows, void *sorted_out_dev);
int h2hip_lookup_permute_presorted_dev(h2hip_ctx *ctx, const void *a_dev, const void *sorted_table_dev, size_t usable_rows, void *a_perm_dev,
                                       void *s_perm_dev);
/* `count` input columns against ONE presorted table (all range lookups of a halo2-base circuit read the same table column,
 * halo2-base/src/gates/range/mod.rs:131-150): the multiset checks of the whole batch come back in one host synchronisation.
 * a_dev / a_perm_dev / s_perm_dev: HOST arrays of `count` device pointers. */
int h2hip_lookup_permute_presorted_batch_dev(h2hip_ctx *ctx, const void *const *a_dev, const void *sorted_table_dev, size_t usable_rows,
                                             void *const *a_perm_dev, void *const *s_perm_dev, size_t count);

/* ---- K8: Poseidon permutation batches (halo2-base PoseidonState::permutation, reference
 *      halo2-base/src/poseidon/hasher/state.rs:35-83,124-160).  The caller supplies the spec its
 *      OptimizedPoseidonSpec was derived from (hasher/spec.rs:88-175): (r_f+r_p)*t round constants and
 *      the t x t MDS matrix (row major), Montgomery limbs; t in {3, 5}.  states: n x t elements, updated
 *      in place; inputs: n x num_inputs elements (num_inputs <= t-1) added to s[1..] with the padding 1
 *      after the last input when num_inputs < t-1. -------------------------------------------------------- */
int h2hip_poseidon_set_spec(h2hip_ctx *ctx, uint32_t t, uint32_t r_f, uint32_t r_p, const void *round_constants, const void *mds);
int h2hip_poseidon_permute_batch_dev(h2hip_ctx *ctx, void *states_dev, const void *inputs_dev, uint32_t num_inputs, size_t n);
/* The sponge PoseidonHasher computes (halo2-base/src/poseidon/hasher/mod.rs, hash_fix_len_array / hash_var_len_array), one function H: start with
 * s = [2^64, 0, ..], split the message into chunks of RATE = t - 1, add each chunk to s[1..] (a chunk shorter than RATE gets 1 added to the first
 * lane after it) and permute; when the length is a multiple of RATE (0 included) permute the empty chunk once more; H = s[1].
 *
 * digests[i] = H(message i).  inputs_dev: n rows of max_len Fr (row stride max_len).  lens_dev == NULL: every message has
 * max_len elements (hash_fix_len_array); otherwise n u32 on the device, message i = the first lens[i] elements of row i
 * (hash_var_len_array / the compact-input forms).  max_len == 0 is legal (inputs_dev may be NULL): the empty hash.
 * A lens[i] > max_len makes the call return H2HIP_ERR_INVALID (h2hip_last_error says how many messages; nothing is read out of bounds, the
 * digests are then unspecified).  With lens_dev the call waits for that check; without, it is asynchronous on the context's stream. */
int h2hip_poseidon_hash_batch_dev(h2hip_ctx *ctx, void *digests_dev, const void *inputs_dev, size_t max_len,
                                  const uint32_t *lens_dev, size_t n);
/* Binary Merkle tree, heap layout: nodes_dev holds 2^(log_leaves+1) Fr; nodes[2^log_leaves + i] = leaf i (taken as given, not
 * hashed), nodes[j] = H([nodes[2j], nodes[2j+1]]) for 1 <= j < 2^log_leaves, nodes[1] = the root, nodes[0] = 0.
 * leaves_dev == NULL: the leaves are already in place in nodes_dev.  log_leaves <= 30.  Asynchronous on the context's stream. */
int h2hip_poseidon_merkle_tree_dev(h2hip_ctx *ctx, void *nodes_dev, const void *leaves_dev, uint32_t log_leaves);
/* The spec PoseidonHasher / pse-poseidon derive from (T, R_F, R_P) alone, secure-MDS index 0: Grain-LFSR round constants
 * [(r_f + r_p)][t] and the Cauchy MDS [t][t], Montgomery Fr, in the textbook (unoptimised) form set_spec takes.  Host only. */
int h2hip_poseidon_spec_generate(uint32_t t, uint32_t r_f, uint32_t r_p, void *round_constants_out, void *mds_out);
/* ---- In-circuit Poseidon traces written on the device.  A circuit that CONSTRAINS a hash needs every cell PoseidonHasher::hash_fix_len_array
 * / PoseidonSponge::squeeze write into the gate columns (fix_len_array_squeeze, halo2-base/src/poseidon/hasher/mod.rs:344-361), not the digest.
 *
 * The in-circuit permutation is OptimizedPoseidonSpec's (hasher/state.rs:35-83).  h2hip_poseidon_spec_optimize (host only) derives it from the
 * textbook arrays set_spec takes (hasher/spec.rs:108-175, mds.rs:118-171: inverse, transpose, factorise), all Montgomery Fr:
 *   start_out [r_f/2 + 1][t], partial_out [r_p], end_out [r_f/2 - 1][t]     constants.start / partial / end
 *   pre_sparse_mds_out [t][t]                                              row major, like mds
 *   sparse_out [r_p][2t - 1]                                               per partial round: SparseMDSMatrix row [t], then col_hat [t - 1]
 * h2hip_poseidon_set_optimized_spec keeps such a spec on the context (a Rust caller passes the arrays its own spec object holds); it is
 * independent of the textbook spec of h2hip_poseidon_set_spec.  t in {3, 5}.  Both refuse a spec in which a row of mds, pre_sparse_mds or a
 * sparse `row` begins with 1: inner_product_simple writes another cell form when its right operand starts with Constant(1)
 * (flex_gate/mod.rs:953-962); no spec PoseidonHasher derives has such a row, and the fill does not guess that form.
 *
 * One unit = fix_len_array_squeeze over `len` inputs from a given state: permutation(chunk, None) per chunk of RATE = t - 1 inputs and, when
 * len is a multiple of RATE (0 included) and H2HIP_POSEIDON_ABSORB_ONLY is not set, one more on the empty chunk.  Its cells, in the reference's
 * order, every one as a canonical (fully reduced) Montgomery Fr; a Constant(c) cell holds c, a copy of an earlier cell holds its value:
 *   WITH_CONSTS          2^64, 0, .., 0                          the t load_constant cells of PoseidonState::default (hasher/mod.rs:48)
 *   per permutation over m inputs (state.rs:124-161, flex_gate/mod.rs:158-168, 412-435):
 *     add                s_0, pre_0, 1, s_0 + pre_0
 *     sum, i = 1..m      s_i, in_i, 1, s_i + in_i, pre_i, 1, s_i + in_i + pre_i
 *     add, i = m+1..t-1  s_i, c, 1, s_i + c                      c = pre_i, plus the padding 1 for i = m + 1
 *     then r_f/2 - 1 times [S-boxes with start[r]; mds], S-boxes with start[r_f/2]; pre_sparse_mds, r_p times [S-box of s_0 with partial[r];
 *     sparse r], r_f/2 - 1 times [S-boxes with end[r]; mds], S-boxes with 0; mds, where
 *     S-box of x with c (mul, mul, mul_add: state.rs:97-106)     0, x, x, x^2,  0, x^2, x^2, x^4,  c, x, x^4, x^5 + c
 *     a matrix (apply_mds), per row                              0, s_0, m_0, s_0 m_0, s_1, m_1, s_0 m_0 + s_1 m_1, ...        (1 + 3t cells)
 *     sparse (apply_sparse_mds)                                  the row's inner product, then per i = 1..t-1:  s_i, s_0, col_hat_i, s_0 col_hat_i + s_i
 * A permutation over m inputs has 4 + 7m + 4(t-1-m) + r_f (12t + t(1+3t)) + r_p (12 + (1+3t) + 4(t-1)) cells: 2,250 + 3m for t = 3 (8, 57).
 * h2hip_poseidon_trace_layout (host only, pure) reports the cells of one unit and the offsets, inside its run of cells, of the t final-state
 * cells; offset [1] is the digest state.s[1].  It refuses unknown flags and a unit without a permutation (len == 0 with ABSORB_ONLY).
 *
 * h2hip_poseidon_fill_hashes_dev writes `count` units of one `len`.  Input i of a unit is inputs_dev[input_offset + i * input_stride]
 * (Fr elements); states_in_dev == NULL starts every unit from [2^64, 0, ..], else unit j starts from states_in_dev[j t .. j t + t);
 * states_out_dev (or NULL) receives the final states densely.  inputs_dev / states_in_dev are plain device pointers and may point into columns
 * of the proof (a previous level's digest cells lie at a stride); dependent levels are separate, stream-ordered calls.  With states_in_dev and
 * ABSORB_ONLY the sponge and compact-chunk forms (hasher/mod.rs:262-288) are expressible; their selects and is_final logic, hash_var_len_array
 * and hash_compact_input stay with the circuit.  Placement follows assign_witnesses (threads/single_phase.rs:273-312): the cells run down
 * from (column, row); when the cell just written sits at break_points_host[column] it is written again at row 0 of column + 1 and the run
 * goes on at row 1 (that copy is never itself a break cell); a unit may cross several breaks.  break_points_host: num_columns - 1 entries, or
 * NULL: no breaks, every unit stays in its column.
 * H2HIP_ERR_INVALID with a message, before anything is launched or uploaded (the columns are then untouched): a NULL mandatory argument
 * (inputs_dev may be NULL when len == 0); no optimised spec set; unknown flags; a unit without a permutation; a column index >= num_columns or
 * a NULL column; a run that leaves the usable rows or the last column; a break point >= usable_rows; an input index outside inputs_len
 * (computed in 64 bits); two units whose cells overlap, break copies and states_out_dev included; an operand range (a unit's first to last
 * input address, states_in_dev) that overlaps a cell this call writes — address intervals, sorted and swept, conservative as for
 * h2hip_gate_fill_chains_dev.  Cells not addressed are not touched.  columns_dev: HOST array of device columns.  count == 0 is H2HIP_OK
 * without device work.  Stream-ordered on the context's stream: one kernel, one lane per unit; the unit table, the column pointers and the
 * break points are the only uploads. */
typedef struct h2hip_poseidon_hash {
    uint32_t column, row;
    uint64_t input_offset;
    uint32_t input_stride, flags;
} h2hip_poseidon_hash;
#define H2HIP_POSEIDON_ABSORB_ONLY 1
#define H2HIP_POSEIDON_WITH_CONSTS 2
int h2hip_poseidon_spec_optimize(uint32_t t, uint32_t r_f, uint32_t r_p, const void *round_constants, const void *mds, void *start_out, void *partial_out,
                                 void *end_out, void *pre_sparse_mds_out, void *sparse_out);
int h2hip_poseidon_set_optimized_spec(h2hip_ctx *ctx, uint32_t t, uint32_t r_f, uint32_t r_p, const void *start, const void *partial, const void *end,
                                      const void *mds, const void *pre_sparse_mds, const void *sparse);
int h2hip_poseidon_trace_layout(uint32_t t, uint32_t r_f, uint32_t r_p, uint32_t len, uint32_t flags, size_t *num_cells, uint32_t *state_out_offsets);
int h2hip_poseidon_fill_hashes_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                                   const void *inputs_dev, size_t inputs_len, uint32_t len, const void *states_in_dev, void *states_out_dev,
                                   const h2hip_poseidon_hash *hashes_host, size_t count);

/* ---- a1: plonk::create_proof for halo2-base circuits, resident on the GPU -------------------------------------------------
 * Replaces create_proof::<KZGCommitmentScheme<Bn256>, ProverSHPLONK<_>, Challenge255<_>, _, Blake2bWrite<_, _, _>, _> as the
 * reference calls it (halo2-base/src/utils/testing.rs:32-50) for circuits configured by BaseConfig::configure
 * (halo2-base/src/gates/circuit/mod.rs:70-96: FlexGateConfig's gate q*(a + b*c - d), RangeConfig's lookups, the equality-enabled
 * columns) — the only constraint system halo2-lib builds.  First phase only (halo2-ecc's ECDSA / pairing circuits use no
 * challenge phases).  The Rust side keeps what it owns: circuit synthesis (it hands over the advice columns assign_witnesses
 * produced, halo2-base/src/gates/flex_gate/threads/single_phase.rs:273-312), the RNG (called back for every Fr::random the
 * prover draws, in upstream's order), the verifying key's transcript representation, and the proof bytes.
 * Everything between — 12 MSMs, ~11 NTTs, the lookup sort, grand products, h(X), evaluations, SHPLONK — runs on the device with
 * every polynomial resident in HBM; the host part is the Blake2b transcript and the O(#openings) bookkeeping of the multiopen. */
/* LIMITS, stated once: (1) This struct carries phase 0 only.  The reference's params are per-phase vectors with MAX_PHASE = 3
 * (num_advice_per_phase / num_lookup_advice_per_phase, halo2-base/src/gates/flex_gate/mod.rs:28,100,132-137, gates/range/mod.rs:87-108); a
 * circuit that uses SecondPhase / ThirdPhase columns or challenges goes through h2hip_phased_circuit_params below (the Rust shim routes
 * `num_advice_per_phase.len() > 1` there, ffi/rust/h2hip-sys/src/safe.rs).  (2) Every gate column's q_enable keeps a fixed column of its own: h2hip_plonk_keygen returns
 * H2HIP_ERR_INVALID for selector activations that upstream's compress_selectors would merge (two gate columns never enabled on a common
 * row, e.g. an empty gate column).  (3) lookup_bits: the table 0..2^lookup_bits must fit 2^k - (blinding_factors + 3) rows, as in
 * RangeConfig::configure (gates/range/mod.rs:117-121). */
typedef struct {
    uint32_t k;                 /* BaseCircuitParams (gates/circuit/mod.rs:25-45), first phase */
    uint32_t num_advice;        /* num_advice_per_phase[0] */
    uint32_t num_lookup_advice; /* num_lookup_advice_per_phase[0] */
    uint32_t num_fixed;
    uint32_t num_instance;      /* num_instance_columns */
    int32_t lookup_bits;        /* < 0: None (no RangeConfig table / lookups) */
} h2hip_base_circuit_params;

/* the ConstraintSystem BaseConfig::configure derives from the params (column order = creation order in the reference's configure) */
typedef struct {
    uint32_t num_advice_total;   /* gate advice columns, then dedicated lookup-advice columns (none when num_advice == 1: range/mod.rs:93-95) */
    uint32_t num_fixed_total;    /* [table] [constants...] [q_lookup] [q_enable per gate column] */
    int32_t table_col, first_constant_col, q_lookup_col, first_q_enable_col;   /* fixed-column indices, -1 = absent */
    uint32_t num_lookups, num_perm_columns, num_perm_sets;   /* permutation columns: constants, gate advice, lookup advice, instance */
    uint32_t degree, extended_k, blinding_factors, usable_rows, quotient_pieces;
    uint32_t num_commitments, num_evals;   /* what one proof carries: proof bytes = 32 * (num_commitments + num_evals) */
} h2hip_plonk_shape;
int h2hip_plonk_shape_of(const h2hip_base_circuit_params *params, h2hip_plonk_shape *out);

/* ---- the dynamic lookup table: BasicDynLookupConfig<KEY_COL>::new(meta, || FirstPhase, num_lu_sets) followed by FlexGateConfig::configure
 * (reference halo2-base/src/virtual_region/lookups/basic.rs:38-199, the RAMCircuit of virtual_region/tests/lookups/memory.rs:92-98).
 * LIMITS of this configuration, stated once: key_cols (= KEY_COL) in 1..4, lu_sets (= num_lu_sets) in 1..48, num_advice (gate columns,
 * phase 0) >= 1, num_fixed (constants) <= 16; no instance columns, no RangeConfig table, one challenge phase; single-GPU only
 * (h2hip_plonk_pk_set_sharding on such a key returns H2HIP_ERR_INVALID).  Anything else returns H2HIP_ERR_INVALID.
 * Layout, from the reference's call order (m = key_cols, L = lu_sets):
 *   advice columns       [table t_0..t_{m-1}] [set 0: k_0..k_{m-1}] ... [set L-1] [gate columns]
 *   fixed columns        [table_is_enabled] [key_is_enabled per set] [constants] [q_enable per gate column]
 *   permutation columns  the dynamic advice columns, the constants, the gate advice columns (enable_equality order)
 *   advice queries       every dynamic column at cur, then per gate column the rotations 0..3; fixed queries in column order
 *   lookups              one per set: input [k_0..k_{m-1}, key_is_enabled], table [t_0..t_{m-1}, table_is_enabled], compressed by
 *                        Horner in theta (acc * theta + e), so the permuted columns are computed after theta is squeezed.
 * Degree max(4, 2 + 1 + 1) = 4; blinding factors 6 (a gate column is queried at four rotations).  A key missing from the table makes
 * h2hip_plonk_create_proof return H2HIP_ERR_INVALID; the context and the key stay usable. */
typedef struct h2hip_dyn_circuit_params {
    uint32_t k;
    uint32_t num_advice;   /* gate advice columns (num_advice_per_phase[0]) */
    uint32_t num_fixed;    /* constants columns */
    uint32_t key_cols;     /* KEY_COL: 1..4 */
    uint32_t lu_sets;      /* num_lu_sets: 1..48 */
} h2hip_dyn_circuit_params;
/* the shape of that constraint system; table_col and q_lookup_col are -1 (the table is made of advice columns) */
int h2hip_plonk_shape_of_dyn(const h2hip_dyn_circuit_params *params, h2hip_plonk_shape *out);

/* ---- multi-phase BaseConfig: FlexGateConfig with SecondPhase / ThirdPhase gate columns, RangeConfig with phase-1 / 2 lookup-advice columns
 * (reference halo2-base/src/gates/flex_gate/mod.rs:62-70,121-137, gates/range/mod.rs:87-108,131-150), and the challenges a circuit declares with
 * meta.challenge_usable_after(phase).  MAX_PHASE = 3 (flex_gate/mod.rs:28).  Layout, from the reference's creation order:
 *   fixed columns        [table, if any] [constants] [q_lookup, if any] [q_enable per gate column: phase 0's, then 1's, then 2's]
 *   advice columns       gate columns of phase 0, 1, 2, then the dedicated lookup-advice columns of phase 0, 1, 2
 *   lookups              the q_lookup lookup (on gate column 0), then one per dedicated lookup-advice column
 *   permutation columns  constants, gate advice, lookup advice, instance; advice queries: gate columns at 0..3, lookup advice at 0
 * The table exists iff lookup_bits >= 0 and the lookup-advice counts sum to non-zero (gates/circuit/mod.rs:74-85); q_lookup iff
 * num_advice_per_phase[0] == 1 and num_lookup_advice_per_phase[0] != 0 (later phases always get dedicated columns, range/mod.rs:93-95).
 * Protocol: after the instances, for each phase in order: the blinding rows of the phase's columns, one blind per column, the phase's
 * commitments (index order), then num_challenges_per_phase[p] challenges squeezed (Challenge255); theta and everything after as for BaseConfig.
 * LIMITS: the column counts summed over the phases are in h2hip_base_circuit_params' ranges; phases are contiguous (a phase with columns
 * follows a phase with columns); a challenge follows a phase with columns; at most 8 challenges; the gates and lookups of THIS
 * configuration query no challenge (the one gate that does, the RLC gate, comes with h2hip_rlc_circuit_params below); single-GPU only (h2hip_plonk_pk_set_sharding on a key
 * with more than one used phase returns H2HIP_ERR_INVALID).  Anything else returns H2HIP_ERR_INVALID.  One used phase and no challenges IS a
 * BaseConfig: same shape, key and proof bytes as the h2hip_base_circuit_params of that phase. */
#define H2HIP_MAX_PHASE 3
#define H2HIP_MAX_CHALLENGES 8
typedef struct h2hip_phased_circuit_params {
    uint32_t k;
    uint32_t num_advice_per_phase[3];          /* gate columns per phase */
    uint32_t num_lookup_advice_per_phase[3];   /* lookup-advice columns per phase */
    uint32_t num_fixed;
    uint32_t num_instance;
    int32_t lookup_bits;                       /* < 0: None */
    uint32_t num_challenges_per_phase[3];      /* challenge_usable_after(phase p): squeezed after phase p's commitments */
} h2hip_phased_circuit_params;
int h2hip_plonk_shape_of_phased(const h2hip_phased_circuit_params *params, h2hip_plonk_shape *out);
/* Supplies the witness of a later phase.  Fills phase `phase`'s advice columns (gate columns, then lookup-advice columns, index order; each n
 * Fr, zeroed on entry) given every challenge squeezed so far, in squeeze order (num_challenges Montgomery Fr, host memory).  Returns 0, or
 * non-zero to abort the proof.  Contract: it runs on the calling thread while the library is quiescent on the context's stream; it may write
 * its columns with h2hip_upload, with `_dev` functions on the same context, or with any device copy it has completed before returning.  Only
 * rows < usable_rows matter: the library writes the blinding rows afterwards.  A non-zero return makes the proof return H2HIP_ERR_INVALID
 * (the last error names the phase) after the stream is drained; the key and the context serve the next proof. */
typedef int (*h2hip_phase_witness_fn)(void *user, uint32_t phase, const void *challenges_fr, size_t num_challenges, void *const *columns_dev,
                                      size_t num_columns);
typedef struct h2hip_phase_witness {
    h2hip_phase_witness_fn fill;
    void *user;
} h2hip_phase_witness;

/* ---- RLC circuits [UPSTREAM-RECALL: downstream's RlcConfig, restated from memory — it is not part of the reference tree]:
 * BaseConfig::configure(base) followed by num_rlc_advice RLC columns, each a SecondPhase advice column with a selector q_rlc and the vertical
 * gate of ROTATIONS = 3 (threads/single_phase.rs:183-193 anticipates it)
 *       q_rlc * (a[r] * gamma + a[r+1] - a[r+2]) = 0,   gamma = challenge 0, the first one squeezed after phase 0's commitments.
 * Layout: everything not listed is the multi-phase layout of `base`.
 *   advice columns       base's columns, then the RLC columns (last indices), all in phase 1: phase 1's commitment group is its gate columns,
 *                        its lookup-advice columns, then the RLC columns (index order)
 *   fixed columns        base's columns, then one q_rlc per RLC column (selectors follow the circuit's own columns in creation order)
 *   permutation columns  constants, gate advice, lookup advice, instance, then the RLC columns (enable_equality is called on them last)
 *   advice queries       base's, then per RLC column the rotations 0, 1, 2; fixed queries: base's, then the q_rlc columns
 *   gates                folded by y in the order flex gates, RLC gates (column order), permutation argument, lookups
 * The gate's degree is 2 + selector: degree, extended_k and the blinding factors (6) are base's.  LIMITS: base.num_challenges_per_phase[0] >= 1;
 * 1 <= num_rlc_advice <= 64 (0 is H2HIP_ERR_INVALID: such a circuit uses h2hip_phased_circuit_params); phase 1 always has columns, which the
 * contiguity rule counts; lookups query no challenge; RLC of variable length (a length cell) selects among the running sums in phase-1 gate columns, whose
 * cells h2hip_gate_fill_chains_dev writes from the sums where h2hip_rlc_fill_chains_dev left them.  Keygen: the selector
 * rule covers the union of the q_enable and q_rlc columns (every pair shares an enabled row), and a q_rlc enabled on a row r with
 * r + 2 >= usable_rows is H2HIP_ERR_INVALID.  Single-GPU only (h2hip_plonk_pk_set_sharding returns H2HIP_ERR_INVALID); not accepted by
 * h2hip_plonk_verify_batch.  Proofs go through h2hip_plonk_create_proof_phased: `advice` is phase 0's columns, the callback's phase-1 column
 * list ends with the RLC columns. */
typedef struct h2hip_rlc_circuit_params {
    h2hip_phased_circuit_params base;
    uint32_t num_rlc_advice;
} h2hip_rlc_circuit_params;
int h2hip_plonk_shape_of_rlc(const h2hip_rlc_circuit_params *params, h2hip_plonk_shape *out);

/* RlcChip::compute_rlc_fixed_len's cells, written on the device [UPSTREAM-RECALL].  A chain over values v_0 .. v_{len-1} is the Horner scan
 * r_0 = v_0, r_i = r_{i-1} * gamma + v_i.  chains_host lists `count` pieces; piece j reads its len values at values_dev[value_offset ..]:
 *   head piece  (flags == 0)              the cells v_0, v_1, r_1, v_2, r_2, ... (2 len - 1 cells) from (column, row) downwards
 *   carry piece (flags & H2HIP_RLC_CARRY) continues the piece before it in the list after a column break: the break cell is duplicated at the
 *               top of the next column, as assign_witnesses does — the cells r_prev, v_0, r_0', v_1, r_1', ... (2 len + 1 cells), with
 *               r_0' = r_prev * gamma + v_0 and r_prev the last r of the piece before it
 * H2HIP_ERR_INVALID before anything is launched: a column index >= num_columns, row + the cell count > usable_rows, len == 0, a value range
 * outside num_values, a carry flag on piece 0.  Cells not addressed are not touched.  columns_dev: HOST array of device columns.  gamma: one
 * Montgomery Fr on the host; 0 and 1 are ordinary values.  Stream-ordered on the context's stream: a segmented scan over the pieces' values
 * (tile, tile sums, apply) and one placement kernel; the piece table is the only upload. */
typedef struct h2hip_rlc_chain {
    uint32_t column, row, len, flags;
    uint64_t value_offset;
} h2hip_rlc_chain;
#define H2HIP_RLC_CARRY 1
int h2hip_rlc_fill_chains_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const void *values_dev,
                              size_t num_values, const h2hip_rlc_chain *chains_host, size_t count, const void *gamma);
/* Flex-gate chains written on the device: the cells of GateChip::inner_product / inner_product_left / inner_product_with_sums, sum,
 * select_by_indicator and select_from_idx [UPSTREAM: halo2-base/src/gates/flex_gate/mod.rs:412, 709-753, 940-1110] and of RangeChip's limb
 * recomposition, which all write
 *       s_0, a_1, b_1, s_1, a_2, b_2, s_2, ...      s_i = s_{i-1} + a_i * b_i   (mod r)
 * i.e. overlapping flex gates q * (a + b*c - d) at every third row.  chains_host lists `count` pieces; operand i of a piece is
 * a_dev[a_offset + i * a_stride] and b_dev[b_offset + i * b_stride] (offsets and strides in Fr elements; a stride of 0 is one constant
 * operand).  a_dev / b_dev are plain device pointers and may point into a column of the proof (the running sums of an RLC head piece lie at
 * stride 2 in its column; indicator bits in a phase-0 column).  A chain is a head piece followed by any number of carry or join pieces, in
 * list order; the cells run from (column, row) downwards:
 *   head piece   (flags == 0)            0, a_0, b_0, s_0, ..., a_{len-1}, b_{len-1}, s_{len-1} with s_0 = a_0 * b_0          (3 len + 1 cells)
 *   head piece   (H2HIP_GATE_START_A)    a_0, a_1, b_1, s_1, ..., s_{len-1} with s_0 = a_0: the "b starts with Constant(1)" case of
 *                                        inner_product_simple (:953-962).  b_0 is not read (with len > 1, b_offset must still lie inside b_len)   (3 len - 2 cells)
 *   carry piece  (H2HIP_GATE_CARRY)      s_prev, a_0, b_0, s_0', ...: continues the piece before it in the list after a column break; the break
 *                                        cell is duplicated at the top, as assign_witnesses does (threads/single_phase.rs:300-307)   (3 len + 1 cells)
 *   join piece   (H2HIP_GATE_JOIN)       a_0, b_0, s_0', ...: continues the piece before it directly below that piece's last cell, in the same
 *                                        column, so that one chain can change where its operands come from (an RLC chain with a carry
 *                                        piece of its own is read as head + join)                                             (3 len cells)
 * The fill computes the arithmetic form.  select_by_indicator's "sum = a where the bit is set" equals s + a*b under that function's own
 * assumptions (b a 0/1 indicator with at most one bit set); s + a*b satisfies the gate whatever the operands are.  Computing the operands
 * (idx_to_indicator, range-check limbs) stays with the circuit.
 * H2HIP_ERR_INVALID with a message, before anything is launched or uploaded (the columns are then untouched): a NULL argument; unknown flags
 * or more than one of CARRY / JOIN / START_A; CARRY or JOIN on piece 0; len == 0; a column index >= num_columns or a NULL column; row + the
 * cell count > usable_rows; a join piece that is not in the previous piece's column at the row after its last cell; an operand index
 * outside a_len / b_len (computed in 64 bits); more than 2^32 pairs in one call; two pieces whose cells overlap; an operand range that
 * overlaps a cell this call writes.  The last check is conservative: it compares address intervals (a piece's first to last operand address
 * against every piece's cells, sorted and swept), so a strided read that interleaves with written cells without touching one is refused
 * too.  Cells not addressed are not touched.  columns_dev: HOST array of device columns.  count == 0 is H2HIP_OK without device work.
 * Stream-ordered on the context's stream: a segmented additive scan over the pieces' products (per tile, over the tile totals) and one
 * placement kernel; the piece table and the column pointers are the only uploads. */
typedef struct h2hip_gate_chain {
    uint32_t column, row, len, flags;
    uint64_t a_offset, b_offset;
    uint32_t a_stride, b_stride;
} h2hip_gate_chain;
#define H2HIP_GATE_CARRY 1
#define H2HIP_GATE_JOIN 2
#define H2HIP_GATE_START_A 4
int h2hip_gate_fill_chains_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const void *a_dev, size_t a_len,
                               const void *b_dev, size_t b_len, const h2hip_gate_chain *chains_host, size_t count);
/* Range checks written on the device: every gate cell of RangeChip::_range_check [halo2-base/src/gates/range/mod.rs:512-564], optionally
 * behind the cells of check_less_than / is_less_than (:604-687), and the copies into the lookup-advice columns, for `count` cells of ONE
 * width per call.  range_bits, lookup_bits, shift_bits and flags are parameters of the call (different widths are separate, stream-ordered
 * calls).  With L = ceil(range_bits / lookup_bits) limbs, lb = lookup_bits and rem = range_bits mod lookup_bits, one unit's gate cells are, in
 * the reference's order, every one a canonical (fully reduced) Montgomery Fr; a Constant(c) cell holds c, a copy of an earlier cell its value:
 *   H2HIP_RANGE_LESS_THAN   a + 2^shift_bits - b, b, 1, a + 2^shift_bits, -2^shift_bits, 1, a        (7 cells, arithmetic in Fr)
 *                           a = values_dev[a_offset], b = values_dev[b_offset]; the checked value v is the first of these cells.
 *                           check_less_than: shift_bits = range_bits = num_bits; is_less_than: shift_bits = padded_bits, range_bits =
 *                           padded_bits + lookup_bits (its closing is_zero stays with the circuit).  Without the flag v = values_dev[a_offset],
 *                           b_offset is not read and there are no such cells (the copy constraint between v and the sum is keygen's).
 *   decomposition (L >= 2)  l_0, l_1, 2^lb, s_1, l_2, 2^(2 lb), s_2, ..., s_{L-1}                    (3 L - 2 cells)
 *                           inner_product_simple's "b starts with Constant(1)" form (flex_gate/mod.rs:953-962): l_i = bits [i lb, (i+1) lb)
 *                           of the canonical integer of v, s_i = its low (i+1) lb bits.  A value that does not fit gets the limbs of its low
 *                           L lb bits, as decompose_fe_to_u64_limbs truncates, and s_{L-1} != v: not a refusal, the witness check names the copy.
 *   tail (rem >= 1)         on x = the last limb (v itself when L = 1): rem = 1: 0, x, x, x (assert_bit); rem > 1: 0, x, 2^(lb-rem),
 *                           x 2^(lb-rem) (mul)                                                         (4 cells)
 * Lookup cells, in the order _range_check queues them: v when L = 1, else l_0 .. l_{L-1}; then the tail's product when rem > 1.  Cell j of a
 * unit has queue position p = lookup_slot + j and goes to lookup_columns_dev[p mod num_lookup_columns] at row p / num_lookup_columns
 * (LookupAnyManager::assign_raw, virtual_region/lookups.rs:129-156); the caller derives lookup_slot from its manager's tag order, as it
 * derives (column, row) from its threads.  values_dev is a plain device pointer and may point into a column of the proof.
 * h2hip_range_check_layout (host only, pure) reports the gate cells and the lookup cells of one unit and the offset, inside the unit's run of
 * gate cells, of the last-limb cell (UINT32_MAX when the unit has no such cell of its own: L = 1 without the prefix).
 * Placement of the gate cells follows assign_witnesses (threads/single_phase.rs:273-312): the cells run down from (column, row); when the
 * cell just written sits at break_points_host[column] it is written again at row 0 of column + 1 and the run goes on at row 1 (that copy is
 * never itself a break cell); a unit may cross several breaks.  break_points_host: num_columns - 1 entries, or NULL: no breaks.
 * H2HIP_ERR_INVALID with a message, before anything is launched or uploaded (all columns are then untouched): a NULL mandatory argument
 * (columns_dev may be NULL when the units have no gate cells); unknown flags; range_bits == 0; lookup_bits outside 1 .. 63; L lb > 253
 * (F::CAPACITY); shift_bits > 253 with LESS_THAN; num_lookup_columns == 0 or a NULL lookup column; for units with gate cells a column index
 * >= num_columns or a NULL column, a run that leaves the usable rows or the last column, a break point >= usable_rows; an operand index
 * outside values_len; a lookup row >= usable_rows; count (L + 1) > 2^32; two units whose lookup slot ranges intersect (exact, in queue
 * positions); two units whose gate cells overlap, break copies included; a gate cell and a lookup cell of the call at one address; an
 * operand address inside anything the call writes — the last three on address intervals, sorted and swept, conservative as for
 * h2hip_gate_fill_chains_dev.  Cells not addressed are not touched.  columns_dev / lookup_columns_dev: HOST arrays of device columns.
 * count == 0 is H2HIP_OK without device work.  Stream-ordered on the context's stream: one kernel, one lane per (unit, slot) with a slot per
 * limb and one for the tail; the unit table, the column pointers, the break points and the table of powers of two are the only uploads. */
typedef struct h2hip_range_check {
    uint32_t column, row;        /* first gate cell of the unit (ignored when the unit has no gate cells) */
    uint64_t a_offset, b_offset; /* values_dev indices; b_offset is read only with H2HIP_RANGE_LESS_THAN */
    uint64_t lookup_slot;        /* index of the unit's first cell in the flat lookup queue */
} h2hip_range_check;             /* 32 bytes */
#define H2HIP_RANGE_LESS_THAN 1
int h2hip_range_check_layout(uint32_t range_bits, uint32_t lookup_bits, uint32_t flags, size_t *num_cells, size_t *num_lookup_cells,
                             uint32_t *last_limb_offset);
int h2hip_range_fill_checks_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                                void *const *lookup_columns_dev, size_t num_lookup_columns, const void *values_dev, size_t values_len,
                                uint32_t range_bits, uint32_t lookup_bits, uint32_t shift_bits, uint32_t flags,
                                const h2hip_range_check *checks_host, size_t count);
/* FpChip::mul written on the device [halo2-ecc/src/fields/mod.rs:188-196]: mul_no_carry::crt [bigint/mul_no_carry.rs] followed by
 * carry_mod::crt [bigint/carry_mod.rs, with bigint/check_carry_to_zero.rs and evaluate_native, bigint/mod.rs:66-74] for `count` pairs of proper
 * CRT integers lying on the device: k = num_limbs limbs of n = limb_bits bits, then the native residue, k + 1 consecutive Fr of values_dev from
 * a_offset / b_offset.  One unit's run, in the reference's cell order, every cell a canonical Montgomery Fr (a Constant(c) cell holds c, a copy
 * of an earlier cell its value); a_i, b_i the operand limbs, m_i the limbs of p, m_nat = p mod r, q_i / o_i the limbs of quotient and
 * remainder, ip(x; y) = inner_product_simple's form from Constant(0): 0, x_0, y_0, s_0, x_1, y_1, s_1, ... (3 len + 1 cells):
 *   S1_i, i < k   ip(a_0 .. a_i; b_i .. b_0), the last cell P_i                                              [mul_no_carry.rs:24-32]
 *   S2            0, a_nat, b_nat, N = a_nat b_nat                                                          [:45]
 *   S3_i, i < k   ip(q_0 .. q_i; m_i .. m_0), the last cell prod_i; then -1, P_i, prod_i - P_i, 1, o_i,
 *                 check_i = prod_i - P_i + o_i (Fr arithmetic)                                              [carry_mod.rs:100-134]
 *   S4_i          a gap: the range check of o_i at n bits, the last at bits(p) - n (k - 1)                  [:139-142]
 *   S5_i          q_i, B, 1, q_i + B with B = 2^n, the last 2^quot_last_limb_bits; then a gap: the range check of that sum at n + 1
 *                 bits, the last at quot_last_limb_bits + 1                                                 [:145-153]
 *   S6_i          check_i, -c_i, 2^n, -c_{i-1} (0 for i = 0); -c_i, 2^rb, 1, -c_i + 2^rb; then a gap: the range check of that sum at
 *                 rb + 1 bits                                                                               [check_carry_to_zero.rs:64-85]
 *   S7            q_0, q_1, 2^n, s_1, ..., s_{k-1}  (3 k - 2 cells: evaluate_native, "b starts with Constant(1)")
 *   S8            the same over o_i; the last cell is out_native
 *   S9            m_nat, quot_native, N                                                                     [carry_mod.rs:181-184]
 * 3 k^2 + 29 k + 3 own cells.  quot_max_bits = n k - 1 + 254 - 1 - bits(p), quot_last_limb_bits = quot_max_bits - n (k - 1); with
 * max_limb_bits = max(max(n, ceil(log2 k) + 2 n) + 1, 2 n + bit_length(k)), rb = floor((max_limb_bits - n + 1 + lb) / lb) lb - 1 (lb =
 * lookup_bits).  The fill writes the own cells and leaves the gaps untouched: h2hip_range_fill_checks_dev writes them from results_dev.
 * The integers, defined for every input: A = sum (canon(a_i) mod 2^n) 2^(n i), B alike; (Q, O) = floor divmod of A B by p; q_i, o_i the low k
 * limbs of Q and O (decompose_bigint drops the rest); P_i, prod_i in Fr from the operand values themselves; c_i = trunc-toward-zero
 * ((signed(check_i) + c_{i-1}) / 2^n) with signed() = fe_to_bigint (values above r / 2 are negative).
 * results_dev (may be NULL): unit u gets 3 k + 1 Fr at index u (3 k + 1): o_0 .. o_{k-1}, out_native (a CRT integer a later call may read as
 * an operand), q_i + B for i < k, -c_i + 2^rb for i < k.
 * h2hip_fp_mul_layout (host only, pure): the unit's cells, its own cells, the lookup cells of its nine range checks; ranges[3 k] = each gap's
 * offset in the run, its cells, its width and the results entry it checks, in context order (o, then q, then c: the lookup queue order);
 * out_cell_offsets[k + 1] = the offsets of the o_i cells and of out_native.  h2hip_trace_seek (host only, pure): where cell `offset` of a run
 * from (column, row) lies under the break rule of h2hip_range_fill_checks_dev (the cell on a break point: its first position).
 * h2hip_fp_mul_range_checks (host only, pure): the 3 k count range units of `count` units in one call, checks_out[j count + u] = gap j of
 * unit u (so the units of one gap, and with them of one width, are consecutive): (column, row) by that walk, a_offset = u (3 k + 1) + the
 * gap's results index, lookup_slot = lookup_slots_host[u] + the lookup cells of the unit's gaps before j.  Gaps 0 .. k-2, k-1, k .. 2k-2,
 * 2k-1 and 2k .. 3k-1 have one width each: five h2hip_range_fill_checks_dev calls over results_dev fill them.
 * H2HIP_ERR_INVALID with a message, before anything is launched or uploaded (all columns and results_dev are then untouched): a NULL mandatory
 * argument; flags != 0; n outside 64 .. 127; k outside 2 .. 4; n k > 320; ceil(log2 k) + 2 n > 252; p = 0 or p not needing exactly k limbs;
 * quot_max_bits >= n k (together the last three always refuse k = 2: n <= 125 gives n k <= 250, and quot_max_bits < n k needs bits(p) >= 253); a limb of p equal to 1; lookup_bits outside 1 .. 63; one of the five widths whose limbs take more than 253 bits; a
 * column index >= num_columns or a NULL column; a run that leaves the usable rows or the last column; a break point >= usable_rows; an
 * operand index + k >= values_len; results_len < count (3 k + 1); count (4 k + 3) > 2^32; two units' cells overlapping (break copies and
 * gaps included); an operand range or the results range overlapping anything the call writes, the results overlapping operands of the call
 * (address intervals, conservative as for h2hip_range_fill_checks_dev).  count == 0 is H2HIP_OK without device work.  Stream-ordered on the
 * context's stream: two kernels (one lane per unit; one lane per (unit, slot), 4 k + 3 slots); the unit table, the column pointers, the break
 * points and a table of constants are the only uploads. */
typedef struct h2hip_fp_params {
    uint32_t limb_bits, num_limbs, lookup_bits, flags;   /* n, k, lb; flags must be 0 */
    uint8_t modulus[48];                                 /* p, little-endian integer */
} h2hip_fp_params;                                       /* 64 bytes */
typedef struct h2hip_fp_mul {
    uint32_t column, row;        /* first cell of the unit's run */
    uint64_t a_offset, b_offset; /* values_dev indices of the two CRT integers */
} h2hip_fp_mul;                  /* 24 bytes */
typedef struct h2hip_fp_mul_range {
    uint32_t cell_offset, num_cells, range_bits, result_index;
} h2hip_fp_mul_range;
int h2hip_fp_mul_layout(const h2hip_fp_params *params, size_t *num_cells, size_t *num_own_cells, size_t *num_lookup_cells,
                        h2hip_fp_mul_range *ranges, uint32_t *out_cell_offsets);
int h2hip_fp_mul_fill_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                          const h2hip_fp_params *params, const void *values_dev, size_t values_len, void *results_dev, size_t results_len,
                          const h2hip_fp_mul *units_host, size_t count);
int h2hip_trace_seek(const uint32_t *break_points_host, size_t num_columns, uint32_t column, uint32_t row, uint64_t offset,
                     uint32_t *column_out, uint32_t *row_out);
int h2hip_fp_mul_range_checks(const uint32_t *break_points_host, size_t num_columns, const h2hip_fp_params *params, const h2hip_fp_mul *units_host,
                              const uint64_t *lookup_slots_host, size_t count, h2hip_range_check *checks_out);
/* EccChip's ec_add_unequal, ec_sub_unequal (both is_strict = false) and ec_double written on the device [halo2-ecc/src/ecc/mod.rs:153-179,
 * :219-246, :302-327] for `count`
 * units over the limb layout of h2hip_fp_params, k = 3 or 4.  A point is 2 (k + 1) consecutive Fr of values_dev: x's k limbs and native
 * residue, then y's; P lies at p_offset, Q at q_offset (ignored for DOUBLE).  One unit's run is the reference's, cell for cell, every cell a
 * canonical Montgomery Fr; a CRT value below is its k limb cells followed by its native cell, ip(x; y) as for h2hip_fp_mul_fill_dev:
 *   sub(a, b)     per cell j <= k of the two values: a_j - b_j, b_j, 1, a_j     (4 (k + 1) cells) [bigint/sub_no_carry.rs:14-33, gate.sub
 *                 halo2-base/src/gates/flex_gate/mod.rs:184-196]
 *   add(a, b)     per cell j <= k of the two values: a_j, b_j, 1, a_j + b_j     (4 (k + 1) cells; the result is the LAST cell of each four)
 *                 [bigint/add_no_carry.rs:12-39, gate.add flex_gate/mod.rs:158-168]
 *   smul(a, c)    per cell: 0, a_j, c, c a_j                                     (4 (k + 1) cells) [bigint/scalar_mul_no_carry.rs:16-35]
 *   mul(a, b)     S1_i (i < k) and S2 of h2hip_fp_mul_fill_dev over the cells of a and b          [bigint/mul_no_carry.rs:24-32, :45]
 *   load(l)       l_0 .. l_{k-1}; l_0, l_1, 2^n, s_1, ..., s_{k-1} (evaluate_native, the last cell the native); then k gaps: the range
 *                 checks of l_i at n bits, the last at bits(p) - n (k - 1)       (4 k - 2 own cells) [fields/fp.rs:187-197, :321-339]
 *   zero(a)       per i < k: ip(q_0 .. q_i; m_i .. m_0), -1, a_i, prod_i - a_i = check_i; per i: q_i, B, 1, q_i + B and a gap (n + 1 bits,
 *                 the last quot_last_limb_bits + 1); per i: check_i, -c_i, 2^n, -c_{i-1}; -c_i, 2^rb, 1, -c_i + 2^rb and a gap (rb + 1
 *                 bits); q's evaluate_native; 0, m_nat, quot_native, a_nat        [bigint/check_carry_mod_to_zero.rs:71-124]
 *   carry(a)      S3 .. S9 of h2hip_fp_mul_fill_dev with the cell a_i in place of P_i and a_nat in place of N [bigint/carry_mod.rs:100-184]
 * ADD_UNEQUAL: dx = sub(Q.x, P.x); dy = sub(Q.y, P.y); load(lambda); ld = mul(lambda, dx); zero(sub(ld, dy)) [divide_unsafe,
 *   fields/mod.rs:217-238]; x3 = carry(sub(sub(mul(lambda, lambda), P.x), Q.x)); y3 = carry(sub(mul(lambda, sub(P.x, x3)), P.y)).
 * SUB_UNEQUAL (P - Q): dx = sub(Q.x, P.x); sy = add(Q.y, P.y); load(lambda); ld = mul(lambda, dx); zero(add(ld, sy)) [neg_divide_unsafe,
 *   fields/mod.rs:256-277]; x3 and y3 exactly as for ADD_UNEQUAL.
 * DOUBLE: y2 = smul(P.y, 2); x3_ = smul(P.x, 3); num = mul(x3_, P.x); load(lambda); zero(sub(mul(lambda, y2), num)); l2 = mul(lambda, lambda);
 *   x2 = smul(P.x, 2); x3 = carry(sub(l2, x2)); y3 = carry(sub(mul(lambda, sub(P.x, x3)), P.y)).
 * At k = 3 a unit has 458 (ADD_UNEQUAL, SUB_UNEQUAL) or 483 (DOUBLE) own cells and 9 k gaps; an add has the cells and the max_limb_bits of a
 * sub, so h2hip_ec_layout gives SUB_UNEQUAL every number it gives ADD_UNEQUAL.  max_limb_bits is threaded as the reference threads it (+1
 * per sub or add, + ceil(log2 c) per smul, ceil(log2 k) + a + b per mul) and gives each reduction its own rb: from max(a, 2 n + bit_length(k)) for
 * zero, max(max(n, a) + 1, 2 n + bit_length(k)) for carry, rb = floor((that - n + 1 + lb) / lb) lb - 1.  Fp::NUM_BITS in load is bits(p): for
 * a prime field the two are the same number by definition, so no accepted modulus differs.
 * The integers, defined for every input (nothing is asserted; a bad witness is the witness checker's business): an operand integer is X =
 * sum (canon(x_i) mod 2^n) 2^(n i); no-carry values are exact signed integers over those; limb and native cells are Fr arithmetic over the
 * operand cells themselves.  lambda = (num mod p) (den mod p)^-1 mod p with den = X2 - X1, num = Y2 - Y1 (DOUBLE: 2 Y, 3 X^2; SUB_UNEQUAL: num =
 * -(Y2 + Y1), so lambda is 0 where Y2 + Y1 = 0 mod p too, and zero's value is lambda (X2 - X1) + (Y2 + Y1)), 0 where den has
 * no inverse.  (Q, O) = FLOOR divmod of the signed value by p; q_i = the low k limbs of |Q|, negated in Fr when Q < 0 (decompose_bigint); o_i
 * the low k limbs of O; c_i as for h2hip_fp_mul_fill_dev.  x3's integer in y3 is the O of x3's reduction.
 * results_dev (may be NULL): unit u gets 9 k + 3 Fr at index u (9 k + 3): x3 and y3 (k + 1 each: a point in operand form, a later call may read
 * it), lambda (k + 1), then per reduction r < 3 (zero, x3's carry, y3's carry) q_i + B for i < k and -c_i + 2^rb_r for i < k, at 3 k + 3 + 2 k r.
 * h2hip_ec_layout (host only, pure): the unit's cells, own cells and lookup cells; ranges[9 k]: each gap's offset, cells, width and the results
 * entry it checks, in context order (the lookup queue order): lambda_i; zero's q then c; x3's o, q, c; y3's o, q, c.  out_cell_offsets[3 (k + 1)]:
 * the cells of x3 (o_i, out_native), of y3, of lambda (its witness cells, its native).
 * h2hip_ec_range_checks (host only, pure): the 9 k count range units of `count` units in one call, grouped by width: group g holds the gaps
 * of the g-th distinct range_bits of h2hip_ec_layout's ranges (order of first appearance; at most seven: n, lambda's and o's last limb,
 * n + 1, the last q, up to three carry widths), groups lie one behind the other (group g starts at count times the gaps of the groups before
 * it), and INSIDE a group the checks run unit by unit, a unit's gaps in context order: rows and lookup slots ascend.  a_offset = u (9 k + 3) +
 * the gap's results index, lookup_slot = lookup_slots_host[u] + the lookup cells of the unit's gaps before it.  One
 * h2hip_range_fill_checks_dev call per group over results_dev fills them.
 * H2HIP_ERR_INVALID with a message, before anything is launched or uploaded (all columns and results_dev are then untouched): the refusals of
 * h2hip_fp_mul_fill_dev applied to this unit (its run, its 2 (k + 1)-element operands, results_len < count (9 k + 3), count times the unit's
 * segments > 2^32), and: an unknown op; k < 3; bits(p) > 256 or p even (lambda's inversion); n k > 318 (3 X^2 would pass 2^640); ceil(log2 k) +
 * a + b > 252 for a product the op makes; a width whose limbs take more than 253 bits.  count == 0 is H2HIP_OK without device work.
 * Stream-ordered on the context's stream: two kernels (one lane per unit; one lane per (unit, segment)); the unit table, the column
 * pointers, the break points, the constants and the segment table are the only uploads. */
#define H2HIP_EC_ADD_UNEQUAL 0   /* ecc/mod.rs ec_add_unequal, is_strict = false */
#define H2HIP_EC_DOUBLE 1        /* ecc/mod.rs ec_double */
#define H2HIP_EC_SUB_UNEQUAL 3   /* ecc/mod.rs ec_sub_unequal, is_strict = false: P - Q (2 is no operation: it stays refused as an unknown op) */
typedef struct h2hip_ec_op {
    uint32_t column, row;        /* first cell of the unit's run */
    uint64_t p_offset, q_offset; /* values_dev indices of the two points; q_offset is ignored for H2HIP_EC_DOUBLE */
} h2hip_ec_op;                   /* 24 bytes */
int h2hip_ec_layout(const h2hip_fp_params *params, uint32_t op, size_t *num_cells, size_t *num_own_cells, size_t *num_lookup_cells,
                    h2hip_fp_mul_range *ranges, uint32_t *out_cell_offsets);
int h2hip_ec_fill_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                      const h2hip_fp_params *params, uint32_t op, const void *values_dev, size_t values_len, void *results_dev, size_t results_len,
                      const h2hip_ec_op *units_host, size_t count);
int h2hip_ec_range_checks(const uint32_t *break_points_host, size_t num_columns, const h2hip_fp_params *params, uint32_t op,
                          const h2hip_ec_op *units_host, const uint64_t *lookup_slots_host, size_t count, h2hip_range_check *checks_out);
/* FpChip's comparisons written on the device for `count` pairs of CRT integers lying on the device (operands as for h2hip_fp_mul_fill_dev: k
 * limb cells, then the native cell, from a_offset / b_offset of values_dev; only the limb cells are read).  op is a non-empty mask; one unit's
 * run is, in this order and in the reference's cell order, every cell a canonical Montgomery Fr:
 *   H2HIP_FP_CMP_REDUCE_A (1)  enforce_less_than_p(a)                                   [halo2-ecc/src/fields/fp.rs:123-142]
 *   H2HIP_FP_CMP_REDUCE_B (2)  enforce_less_than_p(b)
 *   H2HIP_FP_CMP_EQUAL    (4)  big_is_equal::assign(a, b)                                [bigint/big_is_equal.rs]
 * so 1 is enforce_less_than / into_strict_point, 4 is is_equal_unenforced, 7 is FieldChip::is_equal, and 4, 5, 6, 7 are the cells of
 * check_points_are_unequal for a strict / non-strict P.x and Q.x [ecc/mod.rs:183-202] (assert_is_const writes no cell: it is a constant
 * equality the circuit puts on the cell out_cell_offsets names).  a_offset is not read for op = 2, b_offset not for op = 1.
 * enforce_less_than_p(x), with pad = ceil(n / lb) lb, t_0 = p_0 and borrow_i the outcome of limb i, per limb i < k:
 *   i >= 1:     p_i, borrow_{i-1}, 1, t_i = p_i + borrow_{i-1}                           [gate.add, flex_gate/mod.rs:158-168]
 *   is_less_than: s_i = x_i + 2^pad - t_i, t_i, 1, x_i + 2^pad, -2^pad, 1, x_i           [range/mod.rs:646-687]
 *   a gap:      the range check of s_i at pad + lb bits: pad / lb + 1 limbs, no tail gate (3 (pad / lb + 1) - 2 cells), flags 0
 *   is_zero:    z, l_i, inv, 1, 0, l_i, z, 0; the second z is borrow_i                   [flex_gate/mod.rs:789-809]
 * 19 k - 4 own cells and k gaps per enforced operand.  big_is_equal(a, b), per limb i < k:
 *   a_i - b_i, b_i, 1, a_i [gate.sub]; is_zero of that difference (8 cells), its second z is eq_i; for i >= 1: 0, eq_i, partial_{i-1},
 *   partial_i = eq_i partial_{i-1} [gate.and = mul], partial_0 = eq_0
 * 16 k - 4 cells, no gap.  The values, defined for every input (nothing is asserted): s_i and a_i - b_i in Fr over the cell values themselves;
 * l_i = (canon(s_i) >> pad) mod 2^lb, the last limb cell h2hip_range_fill_checks_dev writes for s_i (one decomposition serves both); z = [x = 0]
 * and inv = x^-1 in Fr, 1 for x = 0, for the cell x an is_zero is given.  For limbs below 2^n the final borrow is [X < p] and partial_{k-1} is
 * [A = B].
 * results_dev (may be NULL): unit u gets h2hip_fp_cmp_layout's results_per_unit Fr at index u results_per_unit: for each enforced operand, in
 * order, s_0 .. s_{k-1} and the final borrow; for EQUAL the equality cell's value.
 * h2hip_fp_cmp_layout (host only, pure): the unit's cells, own cells, lookup cells and results; ranges[k per enforced operand]: each gap's
 * offset, cells, width pad + lb and the results entry it checks, in context order (the lookup queue order); out_cell_offsets[3]: the final
 * borrow cell of a's check, of b's, and the equality cell (partial_{k-1}), UINT32_MAX where the mask has none.
 * h2hip_fp_cmp_range_checks (host only, pure): the range units of `count` units, unit by unit, a unit's gaps in context order (rows and
 * lookup slots ascend): a_offset = u results_per_unit + the gap's results index, lookup_slot = lookup_slots_host[u] + the lookup cells of
 * the unit's gaps before it.  All have one width: one h2hip_range_fill_checks_dev call over results_dev fills them (none for op = 4).
 * H2HIP_ERR_INVALID with a message, before anything is launched or uploaded (all columns and results_dev are then untouched): the refusals of
 * h2hip_fp_mul_fill_dev applied to this unit (its parameters, its run, its operands, results_len < count results_per_unit, count times the
 * unit's segments > 2^32: 2 k segments per enforced operand, k for EQUAL), and: op = 0 or op > 7; pad + lb > 253.  count == 0 is H2HIP_OK
 * without device work.  Stream-ordered on the context's stream: two kernels (one lane per unit; one lane per (unit, segment), an is_zero
 * segment's lane doing its own inversion); the unit table, the column pointers, the break points, the constants and the segment table are
 * the only uploads. */
#define H2HIP_FP_CMP_REDUCE_A 1
#define H2HIP_FP_CMP_REDUCE_B 2
#define H2HIP_FP_CMP_EQUAL 4
int h2hip_fp_cmp_layout(const h2hip_fp_params *params, uint32_t op, size_t *num_cells, size_t *num_own_cells, size_t *num_lookup_cells,
                        size_t *results_per_unit, h2hip_fp_mul_range *ranges, uint32_t *out_cell_offsets);
int h2hip_fp_cmp_fill_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                          const h2hip_fp_params *params, uint32_t op, const void *values_dev, size_t values_len, void *results_dev, size_t results_len,
                          const h2hip_fp_mul *units_host, size_t count);
int h2hip_fp_cmp_range_checks(const uint32_t *break_points_host, size_t num_columns, const h2hip_fp_params *params, uint32_t op,
                              const h2hip_fp_mul *units_host, const uint64_t *lookup_slots_host, size_t count, h2hip_range_check *checks_out);
/* EccChip's point selections written on the device for `count` units over the limb layout of h2hip_fp_params, k = 3 or 4 (only n, k and the
 * parameter checks of h2hip_fp_mul_fill_dev matter: no big integer is computed).  Points are in the operand form of h2hip_ec_fill_dev: 2 (k + 1)
 * consecutive Fr of values_dev, x's k limbs and native residue, then y's.  One unit's run is the reference's, cell for cell, every cell a
 * canonical Montgomery Fr (a Constant(c) cell holds c, a copy of an earlier cell its value); all products and sums are Fr arithmetic over the
 * cell values themselves and are defined for every input (nothing is asserted):
 *   H2HIP_EC_SELECT (0), window_bits = 0: ec_select(P, Q, sel) = sel ? P : Q [halo2-ecc/src/ecc/mod.rs:402-415, bigint/select.rs:26-50].  P lies
 *     at p_offset, Q at q_offset, sel is the one Fr at sel_offset.  For x, then y, per limb j < k, then the native cell, one GateChip::select
 *     [halo2-base/src/gates/flex_gate/mod.rs:1144-1170]:  a - b, 1, b, a, b, sel, a - b, out  with out = (a - b) sel + b.  16 (k + 1) cells.
 *   H2HIP_EC_SELECT_FROM_BITS (1), window_bits = w in 1 .. 8, m = 2^w: ec_select_from_bits [ecc/mod.rs:442-456]; strict_ec_select_from_bits
 *     and ec_select_by_indicator behind bits_to_indicator write the same cells.  The m table points lie packed at p_offset + j 2 (k + 1), the w
 *     bits little-endian at sel_offset .. sel_offset + w; q_offset is not read.
 *       bits_to_indicator [flex_gate/mod.rs:609-656], 2^(w+3) - 12 cells:  1 - b_{w-1}, b_{w-1}, 1, 1;  then for idx = 1 .. w - 1 with bit =
 *         b_{w-1-idx}, for each of the 2^idx entries ind of the level before, in order:  (1 - bit) ind, ind, bit, ind;  0, ind, bit, ind bit.
 *         Entry v of the last level is the indicator of v = sum b_i 2^i.
 *       for x, then y [bigint/select_by_indicator.rs:29-69]: per limb j < k a chain  0, a_0, ind_0, s_0, ..., a_{m-1}, ind_{m-1}, s_{m-1}
 *         (3 m + 1 cells) with s_i = s_{i-1} + a_i ind_i, the arithmetic form of h2hip_gate_fill_chains_dev (the reference's "sum = a where
 *         ind != 0" equals it for the one-hot indicator boolean bits give; this form satisfies the gate for any input); then the native
 *         cell: for m > k evaluate_native over the k output limbs, o_0, o_1, 2^n, s_1, ... (3 k - 2 cells), else one more chain over the
 *         table's native cells.
 *     2^(w+3) - 12 + 2 (k (3 m + 1) + (m > k ? 3 k - 2 : 3 m + 1)) cells: 424 at k = 3, w = 4.
 * There are no gaps and no lookup cells.  results_dev (may be NULL): unit u gets 2 (k + 1) Fr at index u 2 (k + 1), the selected point in
 * operand form (the out cells, or the chains' last sums and the native): consecutive units leave a packed table that h2hip_ec_fill_dev,
 * h2hip_fp_cmp_fill_dev and a later select read directly.
 * h2hip_ec_select_layout (host only, pure): the run's length and out_cell_offsets[2 (k + 1)], the offsets of the result cells.
 * H2HIP_ERR_INVALID with a message, before anything is launched or uploaded (all columns and results_dev are then untouched): the refusals of
 * h2hip_fp_mul_fill_dev applied to this unit (its parameters, its run, results_len < count 2 (k + 1), count times the unit's segments > 2^32),
 * and: an unknown op; window_bits outside 1 .. 8 for op 1 or non-zero for op 0; k < 3; a point, a table, sel or the bits outside values_len.
 * count == 0 is H2HIP_OK without device work.  Stream-ordered on the context's stream: two kernels (one lane per unit; one lane per (unit,
 * segment): an 8-cell select, an indicator node, two entries of a chain, or evaluate_native); the unit table, the column pointers, the break
 * points and the constants are the only uploads. */
#define H2HIP_EC_SELECT 0
#define H2HIP_EC_SELECT_FROM_BITS 1
typedef struct h2hip_ec_select {
    uint32_t column, row;                    /* first cell of the unit's run */
    uint64_t p_offset, q_offset, sel_offset; /* values_dev indices: P or the table; Q (op 0 only); sel or the first bit */
} h2hip_ec_select;                           /* 32 bytes */
int h2hip_ec_select_layout(const h2hip_fp_params *params, uint32_t op, uint32_t window_bits, size_t *num_cells, uint32_t *out_cell_offsets);
int h2hip_ec_select_fill_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                             const h2hip_fp_params *params, uint32_t op, uint32_t window_bits, const void *values_dev, size_t values_len,
                             void *results_dev, size_t results_len, const h2hip_ec_select *units_host, size_t count);
/* GateChip::num_to_bits written on the device [flex_gate/mod.rs:1215-1241] for `count` values of one width nb = num_bits, the value of unit u
 * the Fr at a_offset of values_dev.  One unit's run, 7 nb - 2 cells, every cell a canonical Montgomery Fr:
 *   l_0, l_1, 2, s_1, l_2, 4, s_2, ..., s_{nb-1}   the inner product against the powers of two in inner_product_simple's "b starts with
 *                                                   Constant(1)" form, 3 nb - 2 cells (one cell for nb = 1)
 *   0, l_i, l_i, l_i for i < nb                     assert_bit per bit, in order [flex_gate/mod.rs:303-305]
 * l_i is bit i of the canonical integer of the value, s_i its low i + 1 bits.  A value that does not fit gets the bits of its low nb bits (as
 * to_u64_limbs truncates) and s_{nb-1} differs from it: no refusal, the copy between the value and the sum is keygen's and the witness
 * check reports it.  results_dev (may be NULL): unit u gets nb Fr at index u nb, the bits little-endian, so scalar chunks in consecutive
 * units leave the consecutive bit string H2HIP_EC_SELECT_FROM_BITS reads.
 * h2hip_num_to_bits_layout (host only, pure): the run's length and the offset of s_{nb-1} (of l_0 for nb = 1); bit 0 sits at offset 0, bit i at
 * 1 + 3 (i - 1).
 * H2HIP_ERR_INVALID with a message, before anything is launched or uploaded: a NULL mandatory argument; num_bits outside 1 .. 254; count
 * num_bits > 2^32; and what h2hip_range_fill_checks_dev refuses of gate cells, operands and results (a column index >= num_columns or a NULL
 * column; a run that leaves the usable rows or the last column; a break point >= usable_rows; a_offset >= values_len; results_len < count
 * num_bits; two units' cells overlapping; a value or the results overlapping anything the call writes).  count == 0 is H2HIP_OK without
 * device work.  Stream-ordered on the context's stream: one kernel, one lane per (unit, bit). */
typedef struct h2hip_bits_unit {
    uint32_t column, row; /* first cell of the unit's run */
    uint64_t a_offset;    /* values_dev index of the value */
} h2hip_bits_unit;        /* 16 bytes */
int h2hip_num_to_bits_layout(uint32_t num_bits, size_t *num_cells, uint32_t *sum_cell_offset);
int h2hip_num_to_bits_fill_dev(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host,
                               const void *values_dev, size_t values_len, void *results_dev, size_t results_len, uint32_t num_bits,
                               const h2hip_bits_unit *units_host, size_t count);
/* The RLC gates' terms of the quotient numerator on the extended domain, folded in order for j < count:
 *      acc[i] = acc[i]*y + q_j[i]*(a_j[i]*gamma + a_j[i+s] - a_j[i+2s]),  s = 2^(ext_k-k), indices mod 2^ext_k.
 * q_dev / a_dev: HOST arrays of device pointers; 64 columns per launch. */
int h2hip_quotient_rlc_gate_batch_dev(h2hip_ctx *ctx, void *acc_dev, const void *const *q_dev, const void *const *a_dev, size_t count, uint32_t ext_k,
                                      uint32_t k, const void *gamma, const void *y);

typedef struct h2hip_plonk_pk h2hip_plonk_pk;
/* keygen_vk + keygen_pk [UPSTREAM], reference halo2-base/src/utils/testing.rs:224-227.  fixed_host: num_fixed_total columns of 2^k
 * Montgomery Fr (Lagrange values, as the circuit's synthesize assigned them).  copies: ncopies x 4 u32 = (column, row, column, row)
 * with `column` indexing the permutation columns — the copy constraints in the order the circuit emitted them (the cycle
 * representation depends on it).  g / g_lagrange: ParamsKZG's resident base sets (borrowed: they must outlive the key).
 * Builds sigma polynomials, all coefficient / extended-domain forms and the l_0 / l_last / l_blind cosets on the device. */
int h2hip_plonk_keygen(h2hip_ctx *ctx, const h2hip_base_circuit_params *params, const h2hip_bases *g, const h2hip_bases *g_lagrange,
                       const void *const *fixed_host, const uint32_t *copies, size_t ncopies, h2hip_plonk_pk **out);
/* the same for the dynamic-lookup configuration above (fixed_host: num_fixed_total columns in its layout; copies index its permutation columns).
 * Proofs of such a key go through h2hip_plonk_create_proof: the key carries the shape. */
int h2hip_plonk_keygen_dyn(h2hip_ctx *ctx, const h2hip_dyn_circuit_params *params, const h2hip_bases *g, const h2hip_bases *g_lagrange,
                           const void *const *fixed_host, const uint32_t *copies, size_t ncopies, h2hip_plonk_pk **out);
/* the same for the multi-phase configuration above (fixed_host and copies in its layout) */
int h2hip_plonk_keygen_phased(h2hip_ctx *ctx, const h2hip_phased_circuit_params *params, const h2hip_bases *g, const h2hip_bases *g_lagrange,
                              const void *const *fixed_host, const uint32_t *copies, size_t ncopies, h2hip_plonk_pk **out);
/* the same for the RLC configuration above (fixed_host and copies in its layout) */
int h2hip_plonk_keygen_rlc(h2hip_ctx *ctx, const h2hip_rlc_circuit_params *params, const h2hip_bases *g, const h2hip_bases *g_lagrange,
                           const void *const *fixed_host, const uint32_t *copies, size_t ncopies, h2hip_plonk_pk **out);
void h2hip_plonk_pk_free(h2hip_ctx *ctx, h2hip_plonk_pk *pk);
/* VerifyingKey contents: fixed_commitments (num_fixed_total x 64 B affine) and permutation commitments (num_perm_columns x 64 B) */
int h2hip_plonk_pk_commitments(const h2hip_plonk_pk *pk, void *fixed_out, void *permutation_out);
/* vk.transcript_repr — upstream hashes the Debug rendering of the pinned key; it is computed by the Rust side and handed over */
int h2hip_plonk_pk_set_transcript_repr(h2hip_plonk_pk *pk, const void *fr);

/* ---- multi-GPU: one process per GPU (north star: "MSM ranges and independent transforms shard across the 8 GPUs of one node
 * with RCCL over xGMI").  h2hip_comm is the exchange step, inside the library so that the Rust host needs no collective library of its own:
 *   - RCCL transport: librccl.so is dlopen'ed on first use (libh2hip does not link it); rank 0 obtains a 128-byte id with
 *     h2hip_comm_rccl_unique_id and hands it to the other ranks over any channel the host has; h2hip_comm_init_rccl is collective.
 *     ncclAllGather then runs on the context's stream over device buffers (xGMI peer-to-peer, no host staging);
 *   - callback transport: allgather(user, local, bytes, all) gathers `bytes` of host memory from every rank into all[rank * bytes ...] and
 *     returns 0 — torch.distributed / gloo in the CPU tests, MPI, ...; device payloads are staged through pinned memory.
 * The reference has no counterpart (single process, rayon threads). */
typedef struct h2hip_comm h2hip_comm;
typedef int (*h2hip_allgather_fn)(void *user, const void *local, size_t bytes, void *all);
int h2hip_comm_rccl_unique_id(void *out128);
int h2hip_comm_init_rccl(h2hip_ctx *ctx, const void *unique_id128, int world, int rank, h2hip_comm **out);
int h2hip_comm_init_callback(int world, int rank, h2hip_allgather_fn allgather, void *user, h2hip_comm **out);
int h2hip_comm_info(const h2hip_comm *comm, int *world, int *rank, int *is_rccl);
void h2hip_comm_destroy(h2hip_comm *comm);
/* recv[r * bytes ...] = rank r's send[0 .. bytes): device buffers, ordered on the context's stream (RCCL: queued there, returns at once) /
 * host buffers (the 96-byte commitment partials of a round; RCCL: staged through device memory) */
int h2hip_comm_allgather_dev(h2hip_comm *comm, h2hip_ctx *ctx, const void *send_dev, size_t bytes, void *recv_dev);
int h2hip_comm_allgather_host(h2hip_comm *comm, h2hip_ctx *ctx, const void *send_host, size_t bytes, void *recv_host);
/* all-to-all over device buffers: recv[p * bytes ...] = the block rank p put at its send[me * bytes ...] (RCCL: one group of ncclSend / ncclRecv
 * per peer on the context's stream — point-to-point xGMI links, 1 / world of the matching all-gather's inbound traffic; callback transport:
 * through the all-gather callback).  The sharded prover routes the grand products' rows to the ranks that own the columns' lagrange_to_coeff. */
int h2hip_comm_alltoall_dev(h2hip_comm *comm, h2hip_ctx *ctx, const void *send_dev, size_t bytes, void *recv_dev);

/* Sharded create_proof: all ranks run the same h2hip_plonk_create_proof call on the same inputs (same circuit, same RNG stream) and emit
 * identical proof bytes.
 *   - every commitment is a partial MSM over this rank's point range [offset, offset + len) of the SRS — g_shard / g_lagrange_shard hold
 *     just that slice (1/N of the table memory) — followed by ONE all-gather of the 96-byte Jacobian partials per commitment round and
 *     an N-term sum (RCCL has no group-law reduction);
 *   - with H2HIP_SHARD_QUOTIENT, h(X)'s numerator is evaluated by cosets: the extended domain of 2^(ek-k) cosets of the original domain is
 *     dealt round-robin to the ranks (coset c to rank c mod N), each rank runs coeff_to_extended and the quotient identities for its
 *     cosets only (identities are pointwise up to rotations, which stay inside a coset), ONE device-to-device all-gather (2^ek x 32 B in
 *     total) precedes extended_to_coeff.  Ranks >= 2^(ek-k) take no part in this stage.
 *   - evaluations and SHPLONK's polynomial work run on the rank's COEFFICIENT range (= its point range): partial evaluations x^lo * sum_j c[lo + j] x^j
 *     are exchanged and summed (32 bytes per query); the divisions by (X - root) take the ranges above as a carry assembled from one exchange of
 *     partial evaluations (h2hip_fr_kate_division_range_dev);
 *   - with H2HIP_SHARD_PRODUCTS the grand products of the permutation and lookup arguments are formed by ROW range: local factors, inversion
 *     and prefix products, one 32-byte exchange per product, a scaling by everything before the range, ONE device-to-device all-gather of
 *     the rows (every rank needs the complete columns for their coefficient forms);
 *   - with H2HIP_SHARD_QUOTIENT extended_to_coeff runs by cosets too (the size-n inverse transform of a coset where the coset is, a pointwise
 *     combine on every rank after the all-gather); with H2HIP_SHARD_NTT_COLUMNS lagrange_to_coeff is dealt by column;
 *   - replicated on every rank: uploads, the lookup permutation (and lagrange_to_coeff without H2HIP_SHARD_NTT_COLUMNS).
 * Safety: at its first exchange a proof checks that all ranks agree on the shape and the RNG stream and that the point ranges tile
 * [0, 2^k) (H2HIP_ERR_INVALID otherwise); every host exchange carries a status word, and a rank that fails takes part in the next
 * exchange with an error status, so that all ranks return (H2HIP_ERR_PEER on the others) instead of waiting in a collective.
 * comm == NULL or world 1 switches sharding off.  The bases and the communicator must outlive the key (or the next set_sharding call). */
#define H2HIP_SHARD_QUOTIENT 1u
#define H2HIP_SHARD_PRODUCTS 4u /* the grand products (permutation and lookup arguments) by row range: local prefix products, one 32-byte exchange per
                                 product, one device-to-device all-gather of the columns */
#define H2HIP_SHARD_NTT_COLUMNS 8u /* lagrange_to_coeff by column: column j on rank j mod N, one device-to-device all-gather of the coefficient forms per
                                    batch (first-round columns, product columns); pays when a transform outlasts moving a column between GPUs */
#define H2HIP_SHARD_FORCE 2u /* run the sharded code path even with a one-rank communicator (tests: a 1-GPU box exercises RCCL and the coset kernels) */
int h2hip_plonk_pk_set_sharding(h2hip_plonk_pk *pk, h2hip_comm *comm, const h2hip_bases *g_shard, const h2hip_bases *g_lagrange_shard, size_t offset,
                                size_t len, uint32_t flags);
/* the host exchanges of the key's last sharded proof in order — payload bytes per rank, each sent with an 8-byte status word (count: how many;
 * sizes: the first min(count, cap)): hello, the commitment rounds, the products' totals, the go-ahead, evaluations, SHPLONK's carries ... */
int h2hip_plonk_pk_last_exchanges(const h2hip_plonk_pk *pk, size_t *sizes, size_t cap, size_t *count);
/* coefficient / extended-domain helpers of the sharded prover: f(X) -> f(s X) for `count` columns of n coefficients; the listed cosets
 * (count <= 16) of an (n << log_cosets)-point array one after the other; and the inverse with slots[c] = position of coset c in `in` */
int h2hip_fr_coset_scale_batch_dev(h2hip_ctx *ctx, void *const *outs_dev, const void *const *ins_dev, size_t count, size_t n, const void *s);
int h2hip_fr_coset_gather_dev(h2hip_ctx *ctx, void *out_dev, const void *in_dev, const uint32_t *cosets, uint32_t count, uint32_t log_cosets, size_t n);
int h2hip_fr_coset_interleave_dev(h2hip_ctx *ctx, void *out_dev, const void *in_dev, const uint32_t *slots, uint32_t log_cosets, size_t n);
/* ... and the coefficients of a polynomial of degree < n << log_cosets from its PER-COSET inverse transforms P_c (iNTT of size n of coset c's
 * evaluations, then the scaling by s_c^-t; at in[slots[c] * n ...]): out[q n + t] = zeta_n_inv^q / C * sum_c P_c[t] * rho_inv^(c q), C = 2^log_cosets,
 * rho = ext_omega^n, zeta_n_inv = zeta^-n — extended_to_coeff with the size-n transforms done where the cosets are */
int h2hip_fr_coset_combine_dev(h2hip_ctx *ctx, void *out_dev, const void *in_dev, const uint32_t *slots, uint32_t log_cosets, size_t n, const void *rho_inv,
                               const void *zeta_n_inv);

/* `Fr::random(rng)` x n into out (Montgomery limbs); called in upstream's draw order */
typedef void (*h2hip_rng_fill_fn)(void *user, void *out_fr, size_t n);
/* a ready-made h2hip_rng_fill_fn for callers that pre-draw their randomness (tests, deterministic replays, a host RNG running ahead of the
 * prover): serves `count` Montgomery Fr from `values` in order; past the end it writes zeros and sets `exhausted`, which the caller checks
 * after create_proof.  `user` = pointer to the h2hip_array_rng. */
typedef struct {
    const void *values;
    size_t count, pos;
    int exhausted;
} h2hip_array_rng;
void h2hip_array_rng_fill(void *user, void *out_fr, size_t n);
/* The `Fr::random(&mut rng)` stream of a seeded rand_chacha generator (the reference's prover RNG, halo2-base/src/utils/testing.rs:38
 * `StdRng::seed_from_u64(0)` = ChaCha12; gen_srs's `ChaCha20Rng::from_seed([0; 32])`, halo2-base/src/utils/mod.rs:441): element j of the
 * stream = keystream block j (counter mode) reduced mod r as Fr::from_u512 does.  `pos` = the number of elements drawn so far.
 * h2hip_chacha_rng_fill is a ready-made h2hip_rng_fill_fn, `user` = the h2hip_chacha_rng, that generates on ONE host thread; when it is the
 * function handed to h2hip_plonk_create_proof the prover generates its large draws (the n scalars of the random polynomial) ON THE DEVICE
 * with h2hip_rng_chacha_fill_dev instead — same values, same final `pos`, no host generation and no upload.  The block function is pinned
 * to RFC 8439's vectors; the stream layout is [UPSTREAM-RECALL]. */
typedef struct {
    uint8_t seed[32];
    int32_t rounds;   /* 12: rand 0.8's StdRng; 20: ChaCha20Rng; 8: ChaCha8Rng */
    uint64_t pos;
} h2hip_chacha_rng;
void h2hip_rng_seed_from_u64(uint64_t state, uint8_t *seed_out32);   /* rand_core's SeedableRng::seed_from_u64 (PCG32 expansion) */
void h2hip_chacha_rng_init(h2hip_chacha_rng *rng, const uint8_t *seed32, int rounds);
void h2hip_chacha_block(const uint8_t *seed32, uint64_t counter, uint64_t stream, int rounds, uint8_t *out64);
void h2hip_chacha_rng_fill(void *user, void *out_fr, size_t n);
/* out_dev[i] = stream element first_block + i, i < n (Montgomery Fr), on the context's stream */
int h2hip_rng_chacha_fill_dev(h2hip_ctx *ctx, void *out_dev, size_t n, const uint8_t *seed32, int rounds, uint64_t first_block);
#define H2HIP_PLONK_STAGES 12
const char *h2hip_plonk_stage_name(int stage);
/* advice: num_advice_total columns of 2^k Montgomery Fr (host pointers, or device pointers when advice_on_device != 0); rows >=
 * usable_rows are ignored (blinding rows).  instances: num_instance host arrays of instance_lens[i] Fr.  proof_out: capacity
 * proof_cap bytes, *proof_len receives 32 * (num_commitments + num_evals).  stage_ms (optional, H2HIP_PLONK_STAGES doubles):
 * host wall-clock per stage, synchronising the stream at stage boundaries. */
int h2hip_plonk_create_proof(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *advice, int advice_on_device, const void *const *instances_host,
                             const size_t *instance_lens, h2hip_rng_fill_fn rng, void *rng_user, uint8_t *proof_out, size_t proof_cap,
                             size_t *proof_len, double *stage_ms);

/* create_proof for a key of the multi-phase configuration: `advice` carries phase 0's columns only (gate columns, then lookup-advice columns);
 * witness->fill supplies every later phase (see h2hip_phase_witness_fn).  witness may be NULL when the key has one phase.  A BaseConfig or
 * dynamic-lookup key is H2HIP_ERR_INVALID here, and a key with more than one phase is H2HIP_ERR_INVALID for the single-phase entry. */
int h2hip_plonk_create_proof_phased(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *advice, int advice_on_device,
                                    const void *const *instances_host, const size_t *instance_lens, h2hip_rng_fill_fn rng, void *rng_user,
                                    const h2hip_phase_witness *witness, uint8_t *proof_out, size_t proof_cap, size_t *proof_len, double *stage_ms);

/* ---- a caller-supplied transcript.  Upstream's create_proof / verify_proof are generic over the transcript (T: TranscriptWrite<_, E> /
 * TranscriptRead<_, E>); the entries above serve Blake2bWrite / Blake2bRead + Challenge255.  Like the RNG, the transcript is the caller's:
 * with h2hip_transcript the library calls back for every transcript operation, in upstream's order, and never sees the proof's bytes.
 * Values cross as everywhere else in the ABI: a point is 64 B (Montgomery x, y), a scalar or challenge one Montgomery Fr (4 x u64).
 * The proof's byte encoding belongs to the transcript: write_* absorb the value AND serialise it into the caller's own buffer; read_* parse the
 * next value from the caller's buffer (decompressing, if the encoding compresses), absorb it and hand it over; common_* only absorb;
 * squeeze_challenge writes the next challenge.  Every callback returns 0, or non-zero for a failure of that operation.
 * Callbacks run on the calling thread.  They may run while the library has work in flight on the context's streams, so they must not call
 * into the library with that context (h2hip_blake2b and the other host-only entries that take no context are fine). */
typedef int (*h2hip_transcript_point_fn)(void *user, const void *g1_affine);       /* 64 B: Montgomery x, y */
typedef int (*h2hip_transcript_scalar_fn)(void *user, const void *fr);              /* Montgomery Fr */
typedef int (*h2hip_transcript_read_fn)(void *user, void *out);                     /* read_point: 64 B out; read_scalar / squeeze_challenge: Fr out */
typedef struct h2hip_transcript {
    void *user;
    h2hip_transcript_point_fn common_point, write_point;
    h2hip_transcript_scalar_fn common_scalar, write_scalar;
    h2hip_transcript_read_fn read_point, read_scalar, squeeze_challenge;
} h2hip_transcript;

/* create_proof over the caller's transcript, for a key of any of the four configurations: exactly the proof h2hip_plonk_create_proof /
 * h2hip_plonk_create_proof_phased compute (same device schedule, same RNG draws), with every transcript operation going to `t`.  witness follows
 * h2hip_plonk_create_proof_phased's rules: NULL for a key with one phase.  Needs t->common_scalar, write_point, write_scalar and
 * squeeze_challenge: a missing one is H2HIP_ERR_INVALID before any device work.  Returns no bytes: they are in the caller's transcript.
 *   - A callback that returns non-zero aborts the proof with H2HIP_ERR_INVALID; h2hip_last_error names the operation and how many calls of
 *     that operation the proof had made, counting from 1 ("write_point #7").  The proof leaves by the path a commitment at infinity takes:
 *     every stream is drained, and the key and the context serve the next proof.
 *   - A commitment at infinity is refused by the library (H2HIP_ERR_INVALID) in front of write_point, as Blake2bWrite refuses it.
 *   - A squeeze_challenge result that is not a canonical Fr (limbs >= r) is H2HIP_ERR_INVALID: the caller's transcript is broken.
 *   - A key with h2hip_plonk_pk_set_sharding applied is H2HIP_ERR_INVALID. */
int h2hip_plonk_create_proof_transcript(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *advice, int advice_on_device,
                                        const void *const *instances_host, const size_t *instance_lens, h2hip_rng_fill_fn rng, void *rng_user,
                                        const h2hip_phase_witness *witness, const h2hip_transcript *t, double *stage_ms);

/* ---- witness check: what MockProver::run(k, &circuit, instances).verify() answers (halo2-base/src/utils/testing.rs:183-188), specialised to the
 * one gate form and the lookup forms of the three configurations above; not a generic expression evaluator.  Over the usable rows r < usable_rows,
 * exactly in Fr (advice rows >= usable_rows are ignored, as create_proof ignores them):
 *   GATE    gate column g, row r with q_enable_g[r] != 0: q * (a[r] + b[r+1] * c[r+2] - d[r+3]) == 0 (the prover's quotient term); a row with
 *           r + 3 >= usable_rows fails whatever the values (those cells are blinding rows: MockProver reports them unassigned)
 *   LOOKUP  every row's input expression (q_lookup * a, a lookup-advice column a, or the dynamic tuple [k_0..k_{m-1}, key_is_enabled]) occurs
 *           among the table expression's values at rows < usable_rows (a tuple: exact membership of every component)
 *   COPY    every permutation column c, row r: the cell equals sigma(c, r), the next cell of its cycle (constants from the key, instances
 *           zero-padded as create_proof pads them)
 * advice: every advice column of the key's layout (all phases of a multi-phase key, advice index order), host or device (advice_on_device)
 * pointers, usable_rows rows read; instances as for create_proof.  *num_failures = the exact number of failures; failures_out[0 ..
 * min(max_failures, total)) = the first ones in canonical order (gate, then lookup, then copy; by column or lookup index, then by row);
 * failures_out may be NULL when max_failures == 0.  A witness with failures is not an error (H2HIP_OK).  Synchronous; a sharded key is checked
 * locally.  The key and the context serve the next create_proof unchanged. */
#define H2HIP_WITNESS_GATE 1   /* column = gate column (advice index), row = the gate's row */
#define H2HIP_WITNESS_LOOKUP 2 /* column = lookup index (shape order), row = the input row */
#define H2HIP_WITNESS_COPY 3   /* column, row = permutation column and row; peer_* = sigma of that cell */
typedef struct h2hip_witness_failure {
    uint32_t kind, column, row, peer_column, peer_row;
} h2hip_witness_failure;
int h2hip_plonk_check_witness(h2hip_ctx *ctx, const h2hip_plonk_pk *pk, const void *const *advice, int advice_on_device,
                              const void *const *instances_host, const size_t *instance_lens, h2hip_witness_failure *failures_out,
                              size_t max_failures, size_t *num_failures);

/* h2hip_plonk_check_witness plus the gates that query a challenge: with challenges_fr (num_challenges Montgomery Fr on the host, squeeze
 * order) every RLC column c, row r with q_rlc_c[r] != 0 must satisfy a[r] * challenge_0 + a[r+1] - a[r+2] == 0; a row with r + 2 >=
 * usable_rows fails whatever the values.  Failures are H2HIP_WITNESS_GATE with column = the RLC column's advice index, behind the flex
 * gates' in canonical order.  A key of the RLC configuration needs num_challenges >= 1 (H2HIP_ERR_INVALID otherwise) and is H2HIP_ERR_INVALID
 * for h2hip_plonk_check_witness, whose error names this entry; every other key is checked exactly as h2hip_plonk_check_witness does. */
int h2hip_plonk_check_witness_challenges(h2hip_ctx *ctx, const h2hip_plonk_pk *pk, const void *const *advice, int advice_on_device,
                                         const void *const *instances_host, const size_t *instance_lens, const void *challenges_fr,
                                         size_t num_challenges, h2hip_witness_failure *failures_out, size_t max_failures, size_t *num_failures);

/* verify_proof::<KZGCommitmentScheme<Bn256>, VerifierSHPLONK<_>, Challenge255<_>, Blake2bRead<_, _, _>, SingleStrategy<_>> as the reference runs
 * it after every proof (check_proof, halo2-base/src/utils/testing.rs:64-88).  Host code (the reference verifies on the CPU too): transcript
 * replay, the quotient identity rebuilt from the openings, SHPLONK's folded opening and one pairing check.  fixed / permutation commitments:
 * the verifying key (h2hip_plonk_pk_commitments); g1: params.g[0] (64 B); g2, s_g2: 128 B each, SerdeFormat::RawBytes (x.c0, x.c1, y.c0, y.c1).
 * *accepted = 1 iff the proof verifies; a malformed proof is a rejection, not an error. */
int h2hip_plonk_verify_proof(const h2hip_base_circuit_params *params, const void *fixed_commitments, const void *permutation_commitments,
                             const void *transcript_repr, const void *g1, const void *g2, const void *s_g2, const void *const *instances_host,
                             const size_t *instance_lens, const uint8_t *proof, size_t proof_len, int *accepted);

/* h2hip_plonk_verify_proof for the dynamic-lookup configuration: the compressed input and table evaluations come from the openings (no instances) */
int h2hip_plonk_verify_proof_dyn(const h2hip_dyn_circuit_params *params, const void *fixed_commitments, const void *permutation_commitments,
                                 const void *transcript_repr, const void *g1, const void *g2, const void *s_g2, const uint8_t *proof, size_t proof_len,
                                 int *accepted);

/* h2hip_plonk_verify_proof for the multi-phase configuration: the advice commitments are read phase by phase and the challenges squeezed */
int h2hip_plonk_verify_proof_phased(const h2hip_phased_circuit_params *params, const void *fixed_commitments, const void *permutation_commitments,
                                    const void *transcript_repr, const void *g1, const void *g2, const void *s_g2, const void *const *instances_host,
                                    const size_t *instance_lens, const uint8_t *proof, size_t proof_len, int *accepted);

/* h2hip_plonk_verify_proof for the RLC configuration: the RLC gates' terms q * (a0 * gamma + a1 - a2) from the openings enter the quotient
 * identity with gamma = challenge 0 of the transcript replay */
int h2hip_plonk_verify_proof_rlc(const h2hip_rlc_circuit_params *params, const void *fixed_commitments, const void *permutation_commitments,
                                 const void *transcript_repr, const void *g1, const void *g2, const void *s_g2, const void *const *instances_host,
                                 const size_t *instance_lens, const uint8_t *proof, size_t proof_len, int *accepted);

/* verify_proof for num_proofs proofs under ONE verifying key, with one pairing: accepted = 1 iff every proof verifies.  The proofs' points are
 * decompressed in one launch, the transcripts replayed on the host, and every scalar multiplication of every proof goes into one MSM on the
 * GPU.  kind / params: one of the three params structs.  vk and SRS arguments as for the single verifier above.
 * instances_host / instance_lens: num_proofs * num_instance entries, proof-major (NULL when the configuration has no instance columns).  rng
 * draws the num_proofs combiners rho_i in ONE call; a zero rho_i is H2HIP_ERR_INVALID, because that proof would go unchecked.  rejected_out
 * (optional, num_proofs bytes): 1 for every proof that does not verify; when the pairing fails the well-formed proofs are re-verified one by
 * one to find out which (without rejected_out only *accepted = 0 is reported).  acc_out (optional, 2 x 64 B affine, identity all-zero):
 * L = sum rho_i * W'_i and R = sum rho_i * outer_i over the well-formed proofs, i.e. accepted <=> no proof malformed and
 * e(L, s_g2) * e(-R, g2) = 1.  num_proofs = 0 is accepted without device work. */
#define H2HIP_CIRCUIT_BASE 0
#define H2HIP_CIRCUIT_DYN 1
#define H2HIP_CIRCUIT_PHASED 2
int h2hip_plonk_verify_batch(h2hip_ctx *ctx, int kind, const void *params, const void *fixed_commitments, const void *permutation_commitments,
                             const void *transcript_repr, const void *g1, const void *g2, const void *s_g2, size_t num_proofs,
                             const void *const *instances_host, const size_t *instance_lens, const uint8_t *const *proofs, const size_t *proof_lens,
                             h2hip_rng_fill_fn rng, void *rng_user, int *accepted, uint8_t *rejected_out, void *acc_out);

/* verify_proof over the caller's transcript (see h2hip_transcript).  kind / params: H2HIP_CIRCUIT_BASE / _DYN / _PHASED with their params
 * struct as for h2hip_plonk_verify_batch, or H2HIP_CIRCUIT_RLC with an h2hip_rlc_circuit_params, which this entry alone accepts.  vk, SRS
 * and instance arguments as for h2hip_plonk_verify_proof (a configuration without instance columns passes NULL).  Needs t->common_scalar,
 * read_point, read_scalar and squeeze_challenge (H2HIP_ERR_INVALID otherwise).  Host code.
 *   - A non-zero return from read_point / read_scalar, or a read value that is off the curve, the identity, or not canonical (limbs >= the
 *     modulus), is a REJECTION (*accepted = 0, H2HIP_OK), as malformed bytes are for the built-in reader; no callback runs after it.
 *   - A non-zero return from common_scalar or squeeze_challenge, or a squeezed value that is not a canonical Fr, is H2HIP_ERR_INVALID.
 *   - Trailing input is the reader's business: the library cannot see it.
 * acc_out (optional, 2 x 64 B affine, identity all-zero; zeroed when the proof is malformed): the proof's own KZG accumulator (W', outer):
 * *accepted <=> well-formed and e(W', s_g2) * e(-outer, g2) = 1 — what an aggregator defers instead of pairing. */
#define H2HIP_CIRCUIT_RLC 3
int h2hip_plonk_verify_proof_transcript(int kind, const void *params, const void *fixed_commitments, const void *permutation_commitments,
                                        const void *transcript_repr, const void *g1, const void *g2, const void *s_g2,
                                        const void *const *instances_host, const size_t *instance_lens, const h2hip_transcript *t, int *accepted,
                                        void *acc_out);

/* The final CPU-side pairing check of the north star as an entry of its own: *is_one = 1 iff prod_i e(P_i, Q_i) == 1 in Fq12 (what
 * DualMSM::check / halo2curves' multi_miller_loop + final_exponentiation decide for KZG's two pairs).  g1_points: n x 64 B G1Affine
 * (Montgomery, identity all-zero); g2_points: n x 128 B G2Affine in SerdeFormat::RawBytes order (x.c0, x.c1, y.c0, y.c1; identity all-zero).
 * Host code.  Points off the curve / twist are H2HIP_ERR_INVALID.  Pinned by an EIP-197 vector (tests/test_external_vectors.py). */
int h2hip_pairing_check(const void *g1_points, const void *g2_points, size_t n, int *is_one);
/* BLAKE2b (RFC 7693), unkeyed, digest_len 1..64, optional 16-byte personalisation (NULL = none): the hash of the Blake2bWrite / Blake2bRead
 * transcripts (personalisation "Halo2-Transcript"), exported so that it is pinned by the RFC's vectors, not only by proofs. */
int h2hip_blake2b(const void *personal16, unsigned digest_len, const void *msg, size_t len, void *out);

/* ---- diagnostics: 254-bit Montgomery multiplier throughput (the integer roofline bench.py quotes) ------ */
int h2hip_bench_modmul(h2hip_ctx *ctx, uint32_t blocks, uint32_t iters, uint32_t chains, double *elapsed_ms, double *modmuls);
/* HBM-counter calibration probes: kind 0 = coalesced stream of table_bytes, kind 64 / 128 = lanes * per_lane random gathers of aligned
 * 64- / 128-byte entries from a table of table_bytes (the base-table access pattern of the MSM's accumulation) */
int h2hip_bench_gather(h2hip_ctx *ctx, uint32_t kind, size_t table_bytes, uint32_t lanes, uint32_t per_lane, double *elapsed_ms, double *useful_bytes);
/* the same probe on the unsaturated 9 x 29-bit representation the MSM / NTT kernels multiply in (chains: 1 or 2) */
int h2hip_bench_modmul29(h2hip_ctx *ctx, uint32_t blocks, uint32_t iters, uint32_t chains, double *elapsed_ms, double *modmuls);

#ifdef __cplusplus
}
#endif
#endif /* H2HIP_H */
