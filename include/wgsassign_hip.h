/*
 * wgsassign_hip.h -- C ABI of libwgsassign_hip.so, the MI355X (gfx950) implementation of
 * WGSassign's hot path: the per-population EM allele-frequency estimator and the per-SNP
 * assignment log-likelihood summation.
 *
 * The reference exposes this path as Python-callable Cython functions (no C plugin ABI), so
 * the boundary is: Python shim (the modules of wgsassign_amd/, same module/function names as the
 * reference) -> ctypes -> the functions below.  Each entry point names the reference
 * interface it stands in for (paths relative to the reference repository).
 *
 * Conventions
 *   - plain pointers and sizes only; all matrices are float32, C-contiguous, exactly as the
 *     reference's typed memoryviews require (emMAF_cy.pyx:10, glassy_cy.pyx:12);
 *   - every function returns 0 on success, non-zero on failure; wgs_last_error() then holds a
 *     message for the calling thread (the shim raises RuntimeError/ValueError from it);
 *   - "host" pointers are ordinary process memory; "dev" pointers are HIP device memory of the
 *     context's device (so a caller that owns device buffers -- e.g. an RCCL bounce buffer
 *     allocated elsewhere -- can hand them in directly);
 *   - arithmetic mode: WGS_MODE_EXACT reproduces the reference's rounding sequence operation
 *     by operation (double products rounded to float32, float32 (p0+p1)+p2, serial float32
 *     accumulation over individuals in file order) and is bit-identical to the reference for
 *     allele frequencies and EM iteration counts; WGS_MODE_FAST evaluates each term in float32: the
 *     n x K sums stay within 1.2e-7 relative at full size, the EM frequencies drift up to 7e-6 at 10M SNPs
 *     (iteration counts unchanged) -- see DESIGN.md; the host side only ever defaults to EXACT.
 */
#ifndef WGSASSIGN_HIP_H
#define WGSASSIGN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WGS_MODE_EXACT 0
#define WGS_MODE_FAST 1

typedef struct wgs_ctx wgs_ctx;       /* one HIP device + stream + workspace */
typedef struct wgs_beagle wgs_beagle; /* device-resident genotype-likelihood matrix (SNP shard) */
typedef struct wgs_em wgs_em;         /* a batch of EM fits over one wgs_beagle */

/* ------------------------------------------------------------------ context */
const char *wgs_last_error(void);
/* ABI version of this header (WGS_ABI_VERSION).  2 (round 4): wgs_assign lost its `P` / `parts` arguments and
 * wgs_fisher_obs_ind was removed in round 3 while the number stayed 1 -- a caller built against the older header must
 * compare wgs_version() with the WGS_ABI_VERSION it was compiled with and refuse to run on a mismatch (the ctypes shim does:
 * wgsassign_amd/_lib.py); wgs_beagle_codes_info fills 20 entries; wgs_comm_info is new.  3 (round 5): self-checking
 * collectives (wgs_coll_tag, wgs_comm_check, wgs_comm_next_generation, wgs_comm_allreduce_host_tagged).  The z-score entry points
 * (wgs_depth_*, wgs_zscore_*, wgs_zkeep_*, wgs_em_fit_masked) were ADDED under 3: no existing signature changed; so were the
 * integer-table reader (wgs_reader_open_table), the depth ingest (wgs_depth_ingest_*), wgs_depth_create_shape and
 * wgs_depth_download_rows, the deep tier of the z-scores (wgs_zscore_deep_sites, wgs_zkeep_create_deep), and the z-scores over SNP
 * shards (wgs_zscore_classes_sharded, wgs_em_fit_masked_sharded, wgs_depth_ingest_set_first_row, WGS_OP_Z_CLASS, WGS_OP_Z_CHAIN), and
 * windowed scoring (wgs_score_stream_*, wgs_beagle_set_window).  4: --ne_obs in site windows (wgs_fisher_stream_*); no existing
 * signature changed.  --get_assignment_z_score in site windows (wgs_zsum_*, wgs_zscore_classes_carry, wgs_zscore_stats_dev,
 * wgs_depth_copy_rows, wgs_depth_ingest_set_selectors) was ADDED under 4, and so was --get_reference_z_score in site windows
 * (wgs_em_stream_push_masked), and --loo_downsampled_beagle in site windows (wgs_loo_stream_push_scored). */
#define WGS_ABI_VERSION 4
int wgs_version(void);
/* sha256[:16] over every source of the library / over the sources of the EM and scoring kernels (em_kernels.hip,
 * assign_kernels.hip, beagle_kernels.hip, codes_kernels.hip, common.h, log_table.h), fixed at build time: profiles record them, bench.py quotes hardware
 * counters only from a profile whose kernels id equals the loaded library's. */
const char *wgs_build_id(void);
const char *wgs_kernels_id(void);
/* ... and over the sources of the ingest kernels (ingest.hip, inflate.hip, common.h): recorded with the ingest profiles. */
const char *wgs_ingest_kernels_id(void);
int wgs_device_count(int *count);
int wgs_ctx_create(int device, wgs_ctx **out);
void wgs_ctx_destroy(wgs_ctx *ctx);
int wgs_ctx_sync(wgs_ctx *ctx);
/* The context's hipStream_t (all work of the library is enqueued on it). */
void *wgs_ctx_stream(wgs_ctx *ctx);
/* Free / total device memory right now (hipMemGetInfo): used to size leave-one-out batches. */
int wgs_ctx_mem_info(wgs_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);
/* Device name / CU count / total memory of the context's device (for reports). */
int wgs_ctx_info(wgs_ctx *ctx, char *name, int name_len, int *cus, int64_t *mem_bytes);

/* ------------------------------------------------------------------ (1) thin mirrors
 * Same arguments, in-place semantics and results as the Cython kernels; host pointers.
 * They upload, run the HIP kernel and download -- meant for drop-in use and parity tests on
 * inputs the reference handles in seconds, not for the at-scale path (use (2)). */

/* emMAF_cy.emMAF_update(L, f, t)            -- emMAF_cy.pyx:10-23.  f is updated in place. */
int wgs_emmaf_update(wgs_ctx *ctx, const float *L, int64_t m, int64_t n, float *f, int mode);
/* emMAF_cy.rmse1d(v1, v2) -> float          -- emMAF_cy.pyx:26-33.  Bit-exact serial float32
 * accumulation (see wgs_em_rmse_chain). */
int wgs_rmse1d(wgs_ctx *ctx, const float *v1, const float *v2, int64_t m, double *out);
/* glassy_cy.loglike(L, A, loglike_vec, t, i, k) -- glassy_cy.pyx:12-21.  vec is accumulated
 * into, in place.  A is (m, K). */
int wgs_loglike(wgs_ctx *ctx, const float *L, int64_t m, int64_t n, const float *A, int64_t K,
                float *vec, int64_t i, int64_t k, int mode);

/* ------------------------------------------------------------------ (2) device-resident path */

/* Genotype-likelihood matrix of m SNPs x n individuals (reader_cy.pyx:71-77 layout on the
 * host: row s = g0_0 g1_0 g0_1 g1_1 ...).  On the device it is kept as one SNP-major slab of
 * (g0,g1) float2 pairs per group of individuals ("population slab"): slab g is m x ld_g, its
 * columns are the individuals with group_of[i] == g in file order -- the on-device equivalent
 * of the per-population column gather at WGSassign.py:227-233 / glassy.py:69-77, done once.
 * group_of == NULL puts every individual in one group (the --get_pop_like case).
 * site0 is the global index of the shard's first SNP (partition labels use global indices). */
int wgs_beagle_create(wgs_ctx *ctx, int64_t m, int64_t n, const int32_t *group_of, int32_t n_groups,
                      int64_t site0, wgs_beagle **out);
/* Destroying a matrix first destroys every EM batch and score made from it; a later wgs_em_destroy or wgs_score_destroy of
 * such a handle is a no-op (as long as nothing has been created since: a new object may reuse the address). */
void wgs_beagle_destroy(wgs_beagle *b);
/* Copy host rows [row0, row0+nrows) of an (m, 2n) float32 matrix into the slabs. */
int wgs_beagle_upload_rows(wgs_beagle *b, const float *L_rows, int64_t row0, int64_t nrows);
/* Copy rows back into (nrows, 2n) host layout (tests, CPU-baseline sample). */
int wgs_beagle_download_rows(wgs_beagle *b, float *L_rows, int64_t row0, int64_t nrows);
/* Fill the slabs with synthetic low-depth genotype likelihoods on the device (SURVEY 8d:
 * Philox-4x32-10 counter RNG keyed by (seed, global SNP, individual), HWE genotypes from
 * per-group frequencies, Poisson(depth) reads, error 0.01, GLs rounded to 6 decimals). */
int wgs_beagle_synth(wgs_beagle *b, uint64_t seed, double depth);
/* The same with QUALITY-DEPENDENT likelihoods, as ANGSD's -GL 2 writes them for real reads: every read draws its base quality
 * from n_bins bins (Phred values quals[], probabilities probs[]; n_bins <= 8) and enters with its own error rate -- 80-100
 * distinct (g0, g1) per SNP among 1000 individuals with the four bins of current instruments instead of the 27 of the fixed
 * error of wgs_beagle_synth (bench.py: extra.realistic_gl; the NumPy twin of the model is tests/synth.py: make_beagle_quality). */
int wgs_beagle_synth_quality(wgs_beagle *b, uint64_t seed, double depth, int32_t n_bins, const double *quals, const double *probs);
int64_t wgs_beagle_bytes(const wgs_beagle *b);
/* A matrix created with room for more sites than the file turned out to hold (wgs_reader_estimate_sites): rows becomes its
 * number of sites (0 < rows <= the rows it was created with; the rows behind were never written).  Slabs more than a tenth
 * too large are moved into allocations of the right size.  Only before anything was made FROM the matrix (EM batches,
 * scores: rc 2 otherwise); its class codes are dropped. */
int wgs_beagle_set_rows(wgs_beagle *b, int64_t rows);
/* A matrix that is about to be filled again with another range of the same file (the two window matrices of windowed scoring):
 * site0 becomes the global index of its first SNP and rows (0 < rows <= its rows now) its number of sites.  Unlike wgs_beagle_set_rows
 * nothing is allocated, moved or cleared, however few rows remain -- the matrix is swept once more and closed.  What the last tile of
 * 64 SNPs holds BEHIND row `rows` is therefore undefined (the values of the range before), where wgs_beagle_create and
 * wgs_beagle_set_rows leave zeros: the scoring sweeps and the class encoder stop at `rows` and never read it, and no other consumer
 * may rely on zeros there.  Only before anything was made FROM the matrix (rc 2 otherwise); its class codes are dropped when the
 * rows change. */
int wgs_beagle_set_window(wgs_beagle *b, int64_t site0, int64_t rows);
/* Class codes of the matrix: low-depth genotype likelihoods take few distinct (g0, g1) values per SNP (29 on average in
 * the bundled 85-individual data, 27 among 1000 individuals of the 2x synthetic matrices, ~80 with binned base qualities), so
 * the kernels evaluate the EM term's quotient / the per-site log-likelihood once per CLASS and SNP and look it up per
 * individual -- same values, same order of accumulation, same bits.  Built by ONE pass over the matrix when a sweep that
 * profits asks for them (a scoring sweep with shared columns; an EM fit with enough iterations ahead): one byte per (SNP,
 * individual) + a dictionary, and the same again in every population slab's own numbering (csrc/codes.hip).
 * WGSASSIGN_CODES=0 disables them.  A SNP with more classes than the tables hold is left uncoded and taken from the
 * float32 slab by every sweep (nothing matrix-wide depends on it); a matrix whose typical SNP has that many is not coded.
 * info[0..19] = available, classes of the richest coded SNP, bytes held, build milliseconds (sample pass, allocation and
 * encode pass), mean classes per coded SNP, milliseconds of the encode pass alone, of the sample pass, bytes of the slabs' own
 * numbering, rows of the coded EM sweep's quotient table, share of (slab, tile) pairs with more classes than rows (swept
 * directly), hash slots per SNP of the encoder (64 / 128 / 256), share of SNPs left uncoded, dictionary rows per tile, hash
 * probe rounds beyond the first per 16 lookups, milliseconds of the allocation, rows of the coded scoring sweep's table, mean classes
 * per SNP and per (population slab, SNP) in the sample pass, SNPs per table of the coded scoring sweep, milliseconds the building call
 * waited for the codes' memory ([14] is what its hipMalloc took on the helper thread). */
int wgs_beagle_codes_info(wgs_beagle *b, double *info);
/* 1: the codes exist, 0: nothing has asked for them yet, -1: the matrix was found not worth coding (or no memory).  Builds nothing. */
int wgs_beagle_codes_state(wgs_beagle *b);
/* The codes' device memory is allocated on a helper thread (hipMalloc of VRAM an earlier process used takes seconds on this driver);
 * a sweep that wants the codes waits WGSASSIGN_CODES_ALLOC_WAIT_MS (3) for it and otherwise runs over the float32 slabs.  This call
 * waits for an allocation in flight, builds nothing; *alloc_ms = what that hipMalloc took (0: none was in flight).  While one is in
 * flight wgs_em_fit_stats and wgs_assign_last_ms report -1 for kernel times (hipEventElapsedTime would wait for it). */
int wgs_beagle_codes_wait(wgs_beagle *b, double *alloc_ms);
/* Seconds the calling threads of this process have spent inside hipMalloc through the library so far (a running total; the
 * helper thread's allocation of the class codes' memory is not in it).  The driver clears VRAM an earlier process used when
 * it hands it out again, so the same allocation costs 0.3 ms or seconds by what the box did before; callers that time whole
 * paths (bench.py) report the share. */
double wgs_malloc_seconds(void);
/* What the library's cost models predict for this matrix (csrc/em_api.hip: em_codes_model; csrc/codes.hip: wgs_codes_pay_for_scoring),
 * so that a caller can put the prediction beside its measurement.  out[0..11]: one EM sweep of all population slabs over the float32
 * matrix in ms | share of it a coded sweep saves | encode pass (with the slabs' own numbering) in ms | sweeps the decision counts |
 * 1 = the model builds the codes for a fit | one scoring sweep over K_score populations over the float32 matrix in ms | share of
 * that the coded sweep costs | encode pass for scoring alone in ms | 1 = the model builds them for scoring | 1 = from the matrix's
 * own sample pass | classes per (slab, SNP) and per SNP in the sample.  K_score = 0: the EM entries only. */
int wgs_codes_model(wgs_beagle *b, int32_t K_score, double *out);
/* Builds the codes now rather than at the first sweep that asks.  (`em` is ignored since version 2: one pass builds all.) */
int wgs_beagle_codes_prepare(wgs_beagle *b, int em);

/* A batch of EM fits (emMAF.py:15-27) over slabs of `b`.  Fit j estimates the frequency of
 * every SNP from the individuals of group fit_group[j], leaving out individual fit_skip[j]
 * (global individual index, must belong to that group) or nobody when fit_skip[j] < 0 --
 * the leave-one-out re-fit of glassy.py:65-78.  All fits start at f = 0.25 (emMAF.py:17-18). */
int wgs_em_create(wgs_beagle *b, int32_t n_fits, const int32_t *fit_group, const int32_t *fit_skip,
                  int mode, wgs_em **out);
/* A no-op for a batch that is gone already: destroyed before, or together with its matrix (wgs_beagle_destroy) -- as long
 * as nothing has been created since. */
void wgs_em_destroy(wgs_em *em);
/* One EM update (emMAF_cy.pyx:10-23) of every still-active fit in ONE sweep over the slabs,
 * fused with the float64 sum over this shard's SNPs of (f_new - f_old)^2 per fit.  After the
 * call each swept fit's current frequencies are the updated ones and its previous ones are
 * kept (for wgs_em_rmse_chain).  ssq_host (n_fits doubles, may be NULL) receives the sums;
 * fits that were not swept report 0.  Synchronises the context's stream. */
int wgs_em_step(wgs_em *em, double *ssq_host);
/* Same, but leaves the sums in device memory at ssq_dev (n_fits doubles, zeroed by the call)
 * and does NOT synchronise -- for callers that all-reduce them on the device with RCCL. */
int wgs_em_step_dev(wgs_em *em, double *ssq_dev);
/* The reference's convergence metric (emMAF_cy.pyx:26-33) is a SERIAL float32 accumulation
 * over all m SNPs.  This continues that exact chain over this shard's SNPs for one fit:
 * carry_in is the float32 running sum after the preceding shards (0 for the first shard),
 * carry_out the running sum after this shard; diff = sqrt((double)(carry / (float)m_total)). */
int wgs_em_rmse_chain(wgs_em *em, int32_t fit, float carry_in, float *carry_out);
/* Duration in milliseconds of the sweep kernel(s) of the last wgs_em_step*, measured with HIP
 * events recorded on the context's stream around the launch (waits for the kernel). */
int wgs_em_last_sweep_ms(wgs_em *em, float *ms);
/* Freeze (active = 0) or re-activate a fit: frozen fits are skipped by wgs_em_step and keep
 * the frequencies of their last update -- emMAF.py:23-25 `break`s after the update. */
int wgs_em_set_active(wgs_em *em, int32_t fit, int active);
int wgs_em_n_active(wgs_em *em);
/* emMAF.emMAF(L, iter, tole, t) -- emMAF.py:15-27 -- for EVERY fit of the batch in one call: update,
 * `rmse1d(f, f_prev) < tole` -> stop (after the update), at most max_iter updates.  iters_out[j] = the
 * 1-based iteration at which fit j converged, 0 if max_iter was exhausted (the reference prints nothing
 * then).  m_total = SNPs of ALL shards (the metric divides by it); comm = the RCCL communicator of the
 * SNP shards or NULL for one shard.  Iterations are enqueued one ahead of the host: a device kernel
 * decides the clear cases from the (all-reduced) float64 sums; only sums within the band
 * max(guard_floor, m_total * 2^-24) of tole^2 * m_total -- where the reference's serial float32 sum can
 * fall on either side -- go through the exact chain (wgs_em_rmse_chain's, batched over fits, carries
 * handed from shard to shard in rank order).  Identical iteration counts and frequencies to the
 * step-by-step protocol of wgsassign_amd/device.py:run_em (kept for communicators other than RCCL). */
typedef struct wgs_comm wgs_comm;
int wgs_em_fit(wgs_em *em, int32_t max_iter, double tole, int64_t m_total, wgs_comm *comm, double guard_floor,
               int32_t *iters_out);
/* Iterations enqueued / batched exact-chain resolutions / wall seconds of the last wgs_em_fit, and the summed
 * duration in ms of its sweep kernels (HIP events recorded on the context's stream around every sweep; read by this
 * call, not inside the fit).  *sweep_ms = -1 while the class codes' memory is being allocated (wgs_beagle_codes_wait). */
int wgs_em_fit_stats(wgs_em *em, int32_t *iterations, int32_t *chain_batches, double *seconds, double *sweep_ms);
/* Clamp fit j's frequencies to [lo, hi] the way WGSassign.py:236-240 does (float32 compares,
 * NaN untouched). */
int wgs_em_clamp(wgs_em *em, int32_t fit, float lo, float hi);
/* Copy fit j's current frequencies (m floats) to the host / get their device address. */
int wgs_em_get_f(wgs_em *em, int32_t fit, float *f_host);
int wgs_em_set_f(wgs_em *em, int32_t fit, const float *f_host);
/* Rows [row0, row0+nrows) of fit j's current (previous == 0) or previous-iteration (previous != 0)
 * frequencies: the two vectors emMAF.py:22 hands to rmse1d. */
int wgs_em_get_f_range(wgs_em *em, int32_t fit, int previous, int64_t row0, int64_t nrows, float *f_host);
const float *wgs_em_f_dev(wgs_em *em, int32_t fit);

/* Frequency vectors kept on the device for the assignment kernels: K vectors of m floats
 * (population-major), uploaded from the reference's (m, K) matrix (`.pop_af.npy`,
 * WGSassign.py:243,303). */
typedef struct wgs_afset wgs_afset;
int wgs_afset_create(wgs_ctx *ctx, int64_t m, int32_t K, wgs_afset **out);
/* Destroying a frequency set first destroys every score made over it; a later wgs_score_destroy of such a handle is a
 * no-op (as long as nothing has been created since). */
void wgs_afset_destroy(wgs_afset *a);
int wgs_afset_upload(wgs_afset *a, const float *A_mK);           /* host (m, K) -> K device vectors */
int wgs_afset_download(wgs_afset *a, float *A_mK);               /* K device vectors -> host (m, K) */
int wgs_afset_set_column_from_em(wgs_afset *a, int32_t col, wgs_em *em, int32_t fit); /* device copy */
const float *wgs_afset_col_dev(wgs_afset *a, int32_t col);

/* glassy.assignLL(L, af, t) -- glassy.py:18-44 -- for ALL n x K pairs in one sweep over the
 * slabs: out[i*K + k] = sum over this shard's SNPs of the float32 per-site log-likelihood
 * (glassy_cy.pyx:18-21), accumulated in float64 (the reference sums with np.sum(dtype=float),
 * glassy.py:38) in a fixed order (run-to-run reproducible).  colptr (may be NULL) overrides the frequency vector per (individual, k):
 * colptr[i*K + k] is a device pointer to m floats -- this is how the leave-one-out scoring of
 * glassy.py:87-105 (per-individual columns, sticky overwrite) is expressed.  out is a host float64
 * buffer [n*K], summed into (caller zeroes).  Partition sums (utils.py:129-151): wgs_assign_parts_exact. */
int wgs_assign(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int mode, double *out);

/* utils.partition_loglikes(per_site_ll, P) -- utils.py:129-151 -- for every (individual, population)
 * pair, BIT-EXACT: the reference accumulates each partition serially in float32 in site order
 * (np.add.at).  carry_in (float32 [n*P*K], NULL for the first SNP shard) is the running value after the
 * preceding shards, parts_out (float32 [n*P*K], index (i*P + p)*K + k) the value after this one.
 * Always exact-mode arithmetic.  One call = wgs_score_create + _sums + _chains_prepare + _chains_walk
 * below (block-parallel); more than ~64 partitions fall back to one literal chain per GPU lane. */
int wgs_assign_parts_exact(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int32_t P,
                           const float *carry_in, float *parts_out);

/* The scoring step of glassy.py:31-42 / 92-109 as an object, for callers that need the pieces separately
 * (leave-one-out in batches, SNP shards whose chains are joined by float32 carries):
 *   wgs_score_create          b, a, colptr as for wgs_assign; only individuals [row_lo, row_hi) (file order)
 *                             are scored -- a leave-one-out batch scores its own individuals only;
 *   wgs_score_sums            the n x K float64 sums, ONE launch over all population slabs; every
 *                             (individual, population, block of 4096 SNPs) sum has one writer and the blocks
 *                             are added in order: reproducible bit for bit (host `out`, n*K, overwritten);
 *   wgs_score_chains_prepare  block functions of the exact float32 partition chains on the ulp grid predicted
 *                             from those sums; `start` (host n*K float64 or NULL) = the sums over the
 *                             preceding SNP shards.  All shards can prepare in parallel;
 *   wgs_score_chains_walk     walks this shard's chains from carry_in (host float32 [n*P*K] or NULL) -- the
 *                             only step that follows the previous shard -- into parts_out. */
typedef struct wgs_score wgs_score;
int wgs_score_create(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int32_t row_lo, int32_t row_hi,
                     wgs_score **out);
/* A no-op for a score that is gone already: destroyed before, or together with its matrix or frequency set -- as long as
 * nothing has been created since. */
void wgs_score_destroy(wgs_score *sc);
int wgs_score_sums(wgs_score *sc, int mode, double *out);
/* ... continued from the SNP shards before this one (NumPy's running total handed from shard to shard): see api.hip. */
int wgs_score_total_from(wgs_score *sc, const double *carry_in, double *out);
/* The same for ALL shards in one call: the running total goes from shard to shard in SNP order ON THE STREAM -- `world`
 * broadcasts of n*K float64, one readback.  totals_out: the totals (every rank); before_out (may be NULL): the total of
 * the shards before this one (wgs_score_chains_prepare's `start`).  comm NULL = one shard.  Needs wgs_score_sums first. */
int wgs_score_totals_all(wgs_score *sc, wgs_comm *comm, double *totals_out, double *before_out);
int wgs_score_chains_prepare(wgs_score *sc, int32_t P, const double *start);
int wgs_score_chains_walk(wgs_score *sc, const float *carry_in, float *parts_out);
/* The walks of ALL shards in one call (every rank has prepared its block functions): `world` broadcasts of n*P*K
 * float32 on the stream, one readback; parts_out receives the values after the last shard on every rank. */
int wgs_score_chains_walk_all(wgs_score *sc, wgs_comm *comm, float *parts_out);
/* Windowed scoring: the n x K totals of glassy.py:31-42 over a file whose matrix does not fit the device, from consecutive WINDOWS of
 * its sites, each an ordinary device matrix with site0 = its first site.  The accumulator keeps np.sum's running float64 total on the
 * device and continues it over every pushed window's 8192-site chunk sums -- wgs_score_total_from's hand-over from SNP shard to SNP
 * shard, in time instead of in space -- so the totals equal those of one resident matrix bit for bit.
 *   wgs_score_stream_create   for n individuals, K populations and m_total sites in all;
 *   wgs_score_stream_push     scores one window (the sweep of wgs_score_sums; shared columns).  window->site0 must equal the number of
 *                             sites pushed so far and be a multiple of WGS_WINDOW_ALIGN; every window but the last holds a multiple of
 *                             WGS_WINDOW_ALIGN sites.  Anything else: rc 2 and a message, nothing launched.  Returns when the device is
 *                             done with the window (its matrix and frequency set may be refilled); nothing is read back;
 *   wgs_score_stream_finish   the totals (host, n*K float64, overwritten): the one read-back.  rc 2 before all m_total sites were pushed;
 *   wgs_score_stream_destroy  a no-op for a stream that is gone already (as long as nothing has been created since).
 * A stream keeps its context's address and is no child of it in the library's registry: like every object made from a wgs_ctx it
 * must be destroyed, or at least no longer pushed to or finished, BEFORE wgs_ctx_destroy (destroying it afterwards is safe: its two
 * buffers are plain device allocations).  The Python wrapper closes a context's streams before the context. */
#define WGS_WINDOW_ALIGN 8192
typedef struct wgs_score_stream wgs_score_stream;
int wgs_score_stream_create(wgs_ctx *ctx, int64_t n, int32_t K, int64_t m_total, wgs_score_stream **out);
int wgs_score_stream_push(wgs_score_stream *stream, wgs_beagle *window, wgs_afset *window_af, int mode);
int wgs_score_stream_finish(wgs_score_stream *stream, double *out_nK);
void wgs_score_stream_destroy(wgs_score_stream *stream);

/* Windowed fits: --get_reference_af for a file whose matrix does not fit the device.  The EM update is per
 * site; only the stopping test couples the sites, through one sum per iteration over all of them.  A ROUND pushes every window of
 * the file once, in file order; the stream keeps, on the device and across pushes, S[t][fit] (float64: the sum of squared
 * differences of iteration t) and C[t][fit] (float32: the running value of the reference's serial sum, handed from window to window).
 *   wgs_em_stream_create        for n_fits fits of at most max_iter iterations over m_total sites;
 *   wgs_em_stream_push          one window through the EM batch `window_em` made from its matrix: every fit starts at 0.25 and runs
 *                               run_iters[fit] iterations; with add_sums the window's sum of iteration t joins S[t][fit]; the chains
 *                               (chain_fit[i], chain_iter[i]), sorted by iteration, go on from C[t][fit]; a fit with final[fit] != 0
 *                               (final may be NULL) ends at run_iters[fit], is clamped to [clamp_lo[fit], clamp_hi[fit]] and its window
 *                               rows are copied to f_out[fit * f_stride ...] (host).  All of it is enqueued at once; nothing is read
 *                               back but f_out.  The matrix's site0 must equal the sites pushed so far in this round and be a multiple
 *                               of WGS_WINDOW_ALIGN; every window but the last holds a multiple of WGS_WINDOW_ALIGN sites; the batch
 *                               has n_fits fits.  Anything else: rc 2 and a message, nothing launched.  Returns when the device is
 *                               done with the window;
 *   wgs_em_stream_read          the round's one read-back: S and C (host, max_iter * n_fits each, either may be NULL).  rc 2 before
 *                               all m_total sites were pushed; the next push starts the next round at site 0, its chains from zero;
 *   wgs_em_stream_move_window   wgs_beagle_set_window for the matrix under `window_em`, which stays: rows may be anything up to the
 *                               rows the batch was made for.  The batch must be the only object made from the matrix;
 *   wgs_em_stream_destroy       a no-op for a stream that is gone already. */
typedef struct wgs_em_stream wgs_em_stream;
int wgs_em_stream_create(wgs_ctx *ctx, int32_t n_fits, int32_t max_iter, int64_t m_total, wgs_em_stream **out);
int wgs_em_stream_push(wgs_em_stream *stream, wgs_em *window_em, const int32_t *run_iters, const int32_t *final, const float *clamp_lo,
                       const float *clamp_hi, const int32_t *chain_fit, const int32_t *chain_iter, int32_t n_chain, int add_sums,
                       float *f_out, int64_t f_stride);
int wgs_em_stream_read(wgs_em_stream *stream, double *S_host, float *C_host);
int wgs_em_stream_move_window(wgs_em *window_em, int64_t site0, int64_t rows);
void wgs_em_stream_destroy(wgs_em_stream *stream);
/*   wgs_em_stream_push_keep     wgs_em_stream_push for fits the host does not want (leave-one-out re-fits): a final fit is clamped and
 *                               STAYS in the batch -- wgs_em_f_dev finds it until the batch is pushed again -- and nothing of the window's
 *                               size is copied.  sums_from (may be NULL: no sums are added): the window's sum of iteration t joins
 *                               S[t][fit] for t > sums_from[fit] only (0 <= sums_from[fit] <= run_iters[fit]), so a round that runs a
 *                               fit further than an earlier round did adds what is new and nothing twice: S is zeroed when the stream is
 *                               made and never again.  Refuses what wgs_em_stream_push refuses. */
int wgs_em_stream_push_keep(wgs_em_stream *stream, wgs_em *window_em, const int32_t *run_iters, const int32_t *final, const float *clamp_lo,
                            const float *clamp_hi, const int32_t *chain_fit, const int32_t *chain_iter, int32_t n_chain,
                            const int32_t *sums_from);

/* The leave-one-out run in site windows: what wgs_loo does after its re-fits, window by window.  The stream
 * keeps, on the device and across pushes, np.sum's running float64 totals (n x K) and -- for P > 0 -- the serial float32 partition sums
 * so far (n x P x K); a window continues both as the SNP shard of a rank > 0 does in wgs_loo, so they equal those of one resident matrix
 * bit for bit.
 *   wgs_loo_stream_create    for n individuals, K populations, m_total sites and P partitions (0: no partition sums);
 *   wgs_loo_stream_push      one window: `window_em` is the batch of n re-fits over the window's matrix (fit i: the population of
 *                            individual i without i) at their stopping iterations and clamped (wgs_em_stream_push_keep), window_af the
 *                            window's rows of the full-population frequencies.  Builds the column table of glassy.py:87-105, runs the
 *                            per-individual sweep (exact whenever P > 0, else `mode`), folds the window's 8192-site chunk sums onto the
 *                            totals and walks the partition chains on from the carries (labels (site0 + s) % P; the literal chains beyond
 *                            WGS_MAX_BLOCK_PARALLEL_PARTS partitions).  The window rules of wgs_score_stream_push hold, the window has
 *                            the stream's n and K and the batch is the n re-fits; anything else: rc 2 and a message, nothing launched;
 *   wgs_loo_stream_push_scored  the same with the matrix that is scored given apart (--loo_downsampled_beagle: the downsampled file's window
 *                            of the same kept sites; wgs_loo's `scored`): the column table comes from window_em and window_af, the sweep,
 *                            the chunk sums and the chains read scored_window.  It must be of the stream's context and have the fitted
 *                            window's n, m, site0, n_groups and group_of: anything else is rc 2 and a message, nothing launched, the
 *                            stream unchanged.  scored_window == the matrix of window_em is wgs_loo_stream_push;
 *   wgs_loo_stream_finish    the one read-back: ll_out (host, n*K float64), parts_out (host, n*P*K float32, index (i*P + p)*K + k; NULL
 *                            when P == 0).  rc 2 before all m_total sites were pushed;
 *   wgs_loo_stream_destroy   a no-op for a stream that is gone already.  Like the other streams, to be destroyed before its context. */
#define WGS_MAX_BLOCK_PARALLEL_PARTS 64
typedef struct wgs_loo_stream wgs_loo_stream;
int wgs_loo_stream_create(wgs_ctx *ctx, int64_t n, int32_t K, int64_t m_total, int32_t P, wgs_loo_stream **out);
int wgs_loo_stream_push(wgs_loo_stream *stream, wgs_em *window_em, wgs_afset *window_af, int mode);
int wgs_loo_stream_push_scored(wgs_loo_stream *stream, wgs_em *window_em, wgs_beagle *scored_window, wgs_afset *window_af, int mode);
int wgs_loo_stream_finish(wgs_loo_stream *stream, double *ll_out, float *parts_out);
void wgs_loo_stream_destroy(wgs_loo_stream *stream);

/* --ne_obs in site windows: what wgs_fisher_obs and wgs_fisher_ind_means give on one resident matrix, from one
 * pass over consecutive windows, bit for bit.  One fused sweep per window gives the window's rows of f_obs / ne_obs and, per individual,
 * the 128-site leaf sums of NumPy's pairwise float32 sum over the window's full 8192-site chunks; np.mean's running float32 totals (n
 * floats, by individual in file order) stay on the device across pushes.
 *   wgs_fisher_stream_create    for n individuals, K populations and m_total sites in all;
 *   wgs_fisher_stream_push      one window: `window` a matrix with one slab per population (none empty), window_af the window's rows of
 *                               the fitted frequencies; f_obs_rows / ne_obs_rows (host, rows x K float32, site-major, overwritten) the
 *                               window's rows of .fisher_obs.npy / .ne_obs.npy.  The window rules of wgs_score_stream_push hold and the
 *                               window has the stream's n and K; anything else: rc 2 and a message, nothing launched.  Returns when the
 *                               device is done with the window;
 *   wgs_fisher_stream_sweep_ms  kernel time of the last push's fused sweep, between events;
 *   wgs_fisher_stream_finish    ne_ind_out (host, n float32): float32(float64(total) / m_total) per individual, np.mean's last step.
 *                               rc 2 before all m_total sites were pushed, and for a second call;
 *   wgs_fisher_stream_destroy   a no-op for a stream that is gone already.  Like the other streams, to be destroyed before its context. */
typedef struct wgs_fisher_stream wgs_fisher_stream;
int wgs_fisher_stream_create(wgs_ctx *ctx, int64_t n, int32_t K, int64_t m_total, wgs_fisher_stream **out);
int wgs_fisher_stream_push(wgs_fisher_stream *stream, wgs_beagle *window, wgs_afset *window_af, float *f_obs_rows, float *ne_obs_rows);
int wgs_fisher_stream_sweep_ms(wgs_fisher_stream *stream, float *ms);
int wgs_fisher_stream_finish(wgs_fisher_stream *stream, float *ne_ind_out);
void wgs_fisher_stream_destroy(wgs_fisher_stream *stream);

/* glassy.loo(L, af, IDs, t, maf_iter, maf_tole, downsampled_L, num_partitions) -- glassy.py:47-112 -- in one
 * call on device-resident data: per individual (file order) the re-fit of its population without it
 * (wgs_em_fit, a batch of individuals at once), the clamp with n_pop - 1, the never-restored overwrite of
 * the population's column of `a` (in: full-population estimates, out: each population's last re-fit), the
 * K float64 sums and -- when parts_out is given -- the serial float32 partition sums.
 * scored: the matrix that is scored (NULL = b).  batch: re-fits per EM batch (0 = what fits the free
 * device memory, agreed across ranks).  em_mode / score_mode: arithmetic of the re-fits and of the sums
 * (the partition sums are always exact).  ll_out: host float64 [n*K]; parts_out: host float32 [n*P*K] or
 * NULL; iters_out: [n] convergence iterations of the re-fits (0 = max_iter exhausted). */
int wgs_loo(wgs_beagle *b, wgs_beagle *scored, wgs_afset *a, int32_t max_iter, double tole, int64_t m_total,
            wgs_comm *comm, int32_t P, int32_t batch, int em_mode, int score_mode, double *ll_out, float *parts_out,
            int32_t *iters_out);
/* Phases of the last wgs_loo of this process: stats[0..6] = seconds in the EM re-fits (wgs_em_fit incl. its exact
 * chains), in the scoring sweeps (+ cross-rank totals), in the exact partition chains; EM sweep kernel ms; EM batches;
 * batched chain resolutions of the re-fits; EM iterations enqueued. */
int wgs_loo_stats(double *stats);

/* (chain, block) pairs of the last walk that took the literal serial loop / walked in all (diagnostics). */
int wgs_score_last_serial_blocks(wgs_score *sc, int64_t *total_blocks);

/* ------------------------------------------------------------------ RCCL communicator (SNP shards)
 * The one collective of the sharded path -- a sum all-reduce of a few float64 over xGMI -- without
 * a tensor framework: librccl is dlopen'ed on first use.  Rank 0 creates the 128-byte unique id,
 * the host side distributes it (wgsassign_amd/comm.py: TCP on MASTER_ADDR), every rank inits. */
int wgs_comm_unique_id(uint8_t *id128);
int wgs_comm_init(wgs_ctx *ctx, const uint8_t *id128, int rank, int world, wgs_comm **out);
/* A communicator over the caller's own transport: fn sums n host doubles in place over all ranks (0 = success).  The
 * library's loops (wgs_em_fit, wgs_loo) stage their device buffers through pinned host memory for it. */
typedef int (*wgs_allreduce_fn)(double *buf, int64_t n, void *user);
int wgs_comm_create_host(wgs_ctx *ctx, int rank, int world, wgs_allreduce_fn fn, void *user, wgs_comm **out);
void wgs_comm_destroy(wgs_comm *c);
int wgs_comm_rank(wgs_comm *c, int *rank, int *world);
/* Self-checking collectives (ABI 3).  The ranks of the sharded path must issue the same collectives in the same order with the
 * same meaning; every collective of a wgs_comm therefore carries -- inside the SAME transfer as its payload -- a row per rank:
 * {sequence number on this communicator, op, generation, iteration, shape_a, shape_b, payload elements, aux}.  An all-reduce
 * all-gathers the rows (each rank fills its own, the sum fills in the rest) and every rank compares all of them with its own; a
 * broadcast carries the root's row and every receiver compares.  A rank that is out of step makes the NEXT wgs_comm_check -- every
 * entry point that takes a communicator calls it wherever it synchronises -- fail with rc 1 and a wgs_last_error() that starts
 * "collective mismatch:" and names both ranks' tuples; the communicator refuses all further collectives.  `aux` is not compared:
 * a free word per rank that all ranks get to see (wgs_em_fit: "this rank could run two iterations per sweep").  The reference has
 * no counterpart (its only parallelism is OpenMP inside one process, emMAF_cy.pyx:16). */
typedef struct wgs_coll_tag {
    int32_t op;                 /* WGS_OP_*: which exchange step of the path */
    int32_t generation;         /* which fit / scoring call / leave-one-out batch of this communicator (wgs_comm_next_generation) */
    int32_t iteration;          /* EM sweep number, rank hop, ... */
    int32_t shape_a, shape_b;   /* what the payload means: fits in the sweep and EM iterations they run, cells, root of a broadcast */
    int32_t aux;                /* not compared */
} wgs_coll_tag;
enum { WGS_OP_GENERIC = 0, WGS_OP_EM_SUMS = 1, WGS_OP_EM_CHAIN = 2, WGS_OP_EM_FIT_END = 3, WGS_OP_SCORE_TOTALS = 4,
       WGS_OP_PART_CHAINS = 5, WGS_OP_LOO_BATCH = 6, WGS_OP_TIMING = 7, WGS_OP_HOST = 8, WGS_OP_Z_CLASS = 9, WGS_OP_Z_CHAIN = 10 };
int32_t wgs_comm_next_generation(wgs_comm *c);
int wgs_comm_check(wgs_comm *c);
/* Sum all-reduce of n host float64 with a caller-given tag; rows_out (NULL or world * 8 float64) receives every rank's row
 * (rows_out[r * 8 + 7] = rank r's aux).  Returns after the rows have been compared. */
int wgs_comm_allreduce_host_tagged(wgs_comm *c, double *host_buf, int64_t n, const wgs_coll_tag *tag, double *rows_out);
/* In-place sum of n float64 in device memory, enqueued on the context's stream (pairs with wgs_em_step_dev); tagged
 * WGS_OP_GENERIC (sequence number and size are still compared), staged through the communicator's bounce buffer. */
int wgs_comm_allreduce_f64_dev(wgs_comm *c, double *dev_buf, int64_t n);
/* Broadcast of `bytes` bytes (a multiple of 4) of DEVICE memory from rank `root`, enqueued on the context's stream: how
 * a running value -- np.sum's float64 total, a float32 chain carry -- passes from SNP shard to SNP shard without a host
 * round trip (ncclBroadcast; over a host-backed communicator: 32-bit words widened to float64 through its sum all-reduce). */
int wgs_comm_bcast_dev(wgs_comm *c, void *dev_buf, int64_t bytes, int root);
/* stats[0..3]: all-reduces, broadcasts, payload bytes, host round trips (stream synchronisations) of this
 * communicator's collectives so far. */
int wgs_comm_stats(wgs_comm *c, int64_t *stats);
/* info[0..7]: 1 = RCCL communicator / 0 = host-backed; the number of ranks, this rank and the device as RCCL ITSELF reports
 * them for the communicator it built (ncclCommCount / ncclCommUserRank / ncclCommCuDevice; -1 where unavailable) -- wgs_comm_init
 * fails when they differ from what was asked for --; world and rank as given at creation; [6] collectives issued so far, [7] 1 once
 * a rank was found out of step. */
int wgs_comm_info(wgs_comm *c, int64_t *info);
/* Mean device microseconds (HIP events on the context's stream) of `reps` sum all-reduces of n float64 and of `reps`
 * broadcasts of n float64 from rank 0: us_out[0..1].  Collective. */
int wgs_comm_time_collectives(wgs_comm *c, int32_t reps, int64_t n, double *us_out);
/* Same for a host buffer (staged through the device); returns when the result is back. */
int wgs_comm_allreduce_f64(wgs_comm *c, double *host_buf, int64_t n);
/* The communicator's device bounce buffer (>= n float64), e.g. as the target of wgs_em_step_dev;
 * wgs_comm_allreduce_buffer reduces its first n elements in place on the stream, copies them to
 * host_out and synchronises: sweep -> all-reduce -> one readback, nothing in between on the host. */
double *wgs_comm_buffer(wgs_comm *c, int64_t n);
int wgs_comm_allreduce_buffer(wgs_comm *c, int64_t n, double *host_out);

/* ------------------------------------------------------------------ Fisher information (--ne_obs)
 * fisher.fisher_obs(L, af, IDs, t) -- fisher.py:11-44 over fisher_cy.fisher_obs / ne_obs
 * (fisher_cy.pyx:12-39): per (SNP, population) the serial float32 sum over the population's
 * individuals of the observed-information term, and n_tilde = 0.5 * f * a * (1 - a).  The slabs of
 * `b` must be the populations of `a`'s columns.  Outputs are host (m, K) float32 matrices. */
int wgs_fisher_obs(wgs_beagle *b, wgs_afset *a, float *f_obs_mK, float *ne_obs_mK);
/* fisher.fisher_obs_ind -- fisher.py:46-60 over fisher_cy.pyx:41-65 -- is wgs_fisher_ind_means / _sums below.
 * The per-site float32 values themselves for individuals [i0, i0+count) of ONE population
 * (rows_out[(i - i0) * m + s]), so the host can apply np.mean to each row exactly as fisher.py:59. */
int wgs_fisher_ind_sites(wgs_beagle *b, wgs_afset *a, int32_t i0, int32_t count, float *rows_out);
/* ... and np.mean of each of those rows formed on the device exactly as NumPy forms it (pairwise float32 sum, float64
 * division, float32 result): means_out[i - i0], fisher.py:59 without moving the rows to the host. */
int wgs_fisher_ind_means(wgs_beagle *b, wgs_afset *a, int32_t i0, int32_t count, float *means_out);
/* ... over SNP shards: NumPy's running float32 total after this shard, continued from the one before (carry_in, NULL on the
 * first shard); the last shard's totals / number of sites (float64 division) are the means. */
int wgs_fisher_ind_sums(wgs_beagle *b, wgs_afset *a, int32_t i0, int32_t count, const float *carry_in, float *sums_out);

/* ------------------------------------------------------------------ streamed Beagle reader (host)
 * reader_cy.readBeagle(path) -- reader_cy.pyx:16-77 -- as a chunked native reader: gzip inflate,
 * lines parsed in parallel into float32 (rows, 2n) chunks the caller owns (and typically hands
 * to wgs_beagle_upload_rows), so files larger than host RAM can be streamed.  Needs no GPU. */
typedef struct wgs_reader wgs_reader;
int wgs_reader_open(const char *path, int threads, wgs_reader **out);      /* parses the header line */
void wgs_reader_close(wgs_reader *r);
int wgs_reader_n_individuals(wgs_reader *r);
const char *wgs_reader_sample_name(wgs_reader *r, int i);
/* Parse up to max_rows further sites into rows[max_rows][2n]; *nrows = sites parsed (0 at EOF). */
int wgs_reader_next(wgs_reader *r, float *rows, int64_t max_rows, int64_t *nrows);
/* Skip up to max_rows sites without parsing them (SNP-sharded reading: each rank parses only its range). */
int wgs_reader_skip(wgs_reader *r, int64_t max_rows, int64_t *nrows);
/* Same, keeping the skipped lines' site names (read them with wgs_reader_chunk_sites): a names-only pass. */
int wgs_reader_skip_names(wgs_reader *r, int64_t max_rows, int64_t *nrows);
/* Site names of the last chunk, '\n'-terminated each, *bytes long. */
const char *wgs_reader_chunk_sites(wgs_reader *r, int64_t *bytes);
/* Number of data lines (sites) of a gzipped Beagle file: one inflate pass, no parsing. */
int wgs_reader_count_sites(const char *path, int64_t *sites);
/* About how many sites a BGZF file holds, from five samples of a quarter megabyte (newlines per compressed byte x file size):
 * milliseconds.  For sizing a device matrix before the exact count is known (wgs_beagle_set_rows trims it afterwards).
 * rc 3: not BGZF. */
int wgs_reader_estimate_sites(const char *path, int64_t *estimate);
/* The same pass can leave an INDEX behind (index_path): header fields, the site count and at most max_points
 * access points about span_bytes of text apart (deflate-block boundaries with their 32 KiB dictionaries; member
 * boundaries of BGZF / concatenated gzip need none), and the site names, '\n'-terminated (names_path) -- so that
 * one pass per file serves the count, the names-only pass of the downsampled-LOO site masks and every rank's
 * start position.  wgs_reader_open_indexed returns a reader whose next row is first_row without inflating what
 * precedes the access point before it: a rank that owns a later SNP range reads only its own range. */
int wgs_reader_build_index(const char *path, const char *index_path, const char *names_path, int64_t span_bytes,
                           int32_t max_points, int64_t *sites);
int wgs_reader_index_sites(const char *path, const char *index_path, int64_t *sites);
/* The same pass over a BGZF file SPLIT over the ranks of a node (and the threads of each): rank `part` of `nparts` finds the
 * first block of its byte range by its 16-byte signature, inflates and summarises its blocks into part_path
 * (= parts_prefix + "." + part); after a barrier one rank chains the parts -- accepted only if every part starts exactly
 * where the one before ended -- into the index.  rc 3: the file cannot be done in parts (not BGZF, a range off the block
 * chain); one rank then calls wgs_reader_build_index. */
int wgs_reader_index_part(const char *path, const char *part_path, int part, int nparts, int threads);
int wgs_reader_index_merge(const char *path, const char *index_path, const char *parts_prefix, int nparts, int64_t span_bytes,
                           int32_t max_points, int64_t *sites);
int wgs_reader_open_indexed(const char *path, const char *index_path, int64_t first_row, int threads, wgs_reader **out);

/* An INTEGER TABLE instead of a Beagle file: lines of whitespace-separated small integers as np.loadtxt reads them -- the
 * allele depths of --ind_ad_file (WGSassign.py:321, skip_lines 0) or ANGSD's -dumpCounts 4 output (allele_counts_beagle.py:11,
 * skip_lines 1).  Plain text, gzip or BGZF, told apart by the file's first bytes, not by its name.  No header is parsed and no
 * site-name column kept; blank lines and lines that start with '#' are no rows.  Such a reader serves wgs_depth_ingest_create
 * only (wgs_reader_next and the Beagle ingest refuse it).  wgs_reader_table_columns: columns of the first data line (0: none). */
int wgs_reader_open_table(const char *path, int threads, int skip_lines, wgs_reader **out);
int wgs_reader_table_columns(wgs_reader *r);

/* ------------------------------------------------------------------ device-side ingest
 * reader_cy.pyx:52-66 (strtok + atof per value) on the MI355X: the reader only inflates, finds the newlines and keeps
 * the site names; the TEXT goes to the device through page-locked buffers and a HIP kernel tokenises it straight into
 * the population slabs of `b` (csrc/ingest.hip).  Values the kernel does not convert itself (inf/nan, hex, 16+ digits)
 * flag their line, which the host then parses with strtod -- the results equal wgs_reader_next's bit for bit.
 * `r` is a reader positioned at the first wanted row (wgs_reader_open / wgs_reader_open_indexed); after
 * wgs_ingest_create it must only be used through the ingest, which is destroyed BEFORE the reader is closed.
 * limit_rows < 0: to the end of the file.  chunk_bytes <= 0: 256 MiB of text per chunk. */
typedef struct wgs_ingest wgs_ingest;
int wgs_ingest_create(wgs_beagle *b, wgs_reader *r, int64_t limit_rows, int64_t chunk_bytes, wgs_ingest **out);
void wgs_ingest_destroy(wgs_ingest *g);
/* Next chunk: its lines fill the slab rows row0, row0 + 1, ... (keep != NULL: keep[i] != 0 keeps the i-th line of this
 * chunk, dropped lines take no row; keep_len = entries available).  *file_rows = lines consumed (0: end of the file or
 * of the row limit), *rows_written = rows filled.  Synchronises the context's stream. */
int wgs_ingest_next(wgs_ingest *g, int64_t row0, const uint8_t *keep, int64_t keep_len, int64_t *file_rows, int64_t *rows_written);
/* Site names of that chunk's lines (kept or not), '\n'-terminated each, *bytes long. */
const char *wgs_ingest_chunk_sites(wgs_ingest *g, int64_t *bytes);
/* stats[0..13]: seconds the caller waited for the producer thread; producer seconds in inflate / in the newline scan (host
 * inflate); device ms (copies + kernels); lines parsed on the host; text bytes; lines; chunks; ms of the device inflate
 * kernel; BGZF members inflated on the device (csrc/inflate.hip: BGZF files take the device-resident pipeline unless
 * WGSASSIGN_INFLATE=host); members the device left to the host's inflater; producer seconds reading compressed members; seconds inside
 * wgs_ingest_create and inside wgs_ingest_next. */
int wgs_ingest_stats(wgs_ingest *g, double *stats);

/* ------------------------------------------------------------------ z-scores (--get_reference_z_score, --get_assignment_z_score)
 * zscore.py / zscore_cy.pyx / WGSassign.py:311-446 on device-resident data.  The host keeps what is a few dozen numbers per
 * individual (key filter, tables: wgsassign_amd/zscore.py); everything that touches every site runs here.  A depth pair
 * (Ar, Aa) of depth d = Ar + Aa <= wgs_zscore_max_depth() (21) has the class index d (d + 1) / 2 + Aa; WGS_Z_CLASSES of them: the
 * dense tier, one class per thread of the class sweep.  Deeper pairs -- up to 255 reads per allele, what the table's bytes hold,
 * i.e. depth 510 -- form a sparse second tier: the class sweep counts them, wgs_zscore_deep_sites lists them for the host's
 * dictionary, and a kept-site set made by wgs_zkeep_create_deep carries the rows of the deep depths that survived the key
 * filter.  Data without such sites never enters the second tier. */
#define WGS_Z_CLASSES 253
typedef struct wgs_depth wgs_depth;   /* allele-depth table of a matrix: one byte pair per (individual, site), next to the slabs */
typedef struct wgs_zkeep wgs_zkeep;   /* the kept sites (L_keep) of a batch of individuals */
/* The AD table of WGSassign.py:321 / 409 (np.loadtxt, (m, 2n) int32: reference- and alternative-allele reads per individual) for the
 * SNP shard of `b`.  Destroyed with its matrix; a later wgs_depth_destroy of such a handle is a no-op (as for wgs_em_destroy). */
int wgs_depth_create(wgs_beagle *b, wgs_depth **out);
void wgs_depth_destroy(wgs_depth *d);
/* Host rows [row0, row0 + nrows) of the (m, 2n) int32 table.  rc 2: a count outside 0..255 (does not fit the table). */
int wgs_depth_upload_rows(wgs_depth *d, const int32_t *AD_rows, int64_t row0, int64_t nrows);
/* The mirror: rows [row0, row0 + nrows) of the table back into (nrows, 2n) int32 host layout (tests, tools). */
int wgs_depth_download_rows(wgs_depth *d, int32_t *AD_rows, int64_t row0, int64_t nrows);
/* A table of m sites x n individuals that belongs to no matrix (python -m wgsassign_amd.allele_counts: only filled and read back;
 * wgs_zscore_classes and wgs_zkeep_create refuse it).  Destroyed by wgs_depth_destroy. */
int wgs_depth_create_shape(wgs_ctx *ctx, int64_t m, int64_t n, wgs_depth **out);
/* The table filled FROM A FILE on the device (csrc/ingest.hip: depth_tokenise_kernel), through the hand-overs of the Beagle
 * ingest: plain text and plain gzip come as text through page-locked buffers (the host inflates), BGZF members are inflated on
 * the device unless WGSASSIGN_INFLATE=host.  `r` comes from wgs_reader_open_table and is used through the ingest only, which is
 * destroyed before the reader is closed and before the table.
 *   WGS_DEPTH_PAIRS   individual i of a line owns tokens 2i, 2i + 1 (--ind_ad_file); columns behind 2n are ignored;
 *   WGS_DEPTH_COUNTS  tokens 4i .. 4i + 3 (A, C, G, T reads); majmin[site][2] (host, m x 2 bytes, each 0..3) selects the pair
 *                     (token 4i + major, token 4i + minor) -- allele_counts_beagle.py:19-23.
 * The kernel converts runs of 1-3 digits up to 255; a line with anything else, or too few columns, is parsed on the host by
 * np.loadtxt's rules (a decimal or exponent form is truncated, as NumPy still does with a deprecation warning): rc 2 names the 1-based line of the file for a token np.loadtxt refuses as int32, a short line, or a count
 * outside 0..255.  limit_rows < 0: to the end of the file.  chunk_bytes <= 0: 4 MiB of text per chunk (32 MiB when the device
 * inflates) -- host memory stays at the staging buffers, never the table.
 * wgs_depth_ingest_next: the next chunk's data lines fill rows row0, row0 + 1, ...; *file_rows = data lines consumed (0: end),
 * *rows_written = rows filled.  Lines beyond the table's last row are counted, not stored (*rows_written = 0 from there on): the
 * caller compares the total with the rows it expected.
 * wgs_depth_ingest_set_first_row (before the first wgs_depth_ingest_next, or rc 2): the table holds the file's data rows
 * [first_row, first_row + m) -- a SNP shard's -- instead of the first m.  Data lines before the range are read and checked like any
 * other (a token np.loadtxt refuses, or a short line, is still reported with its line of the file; in pairs mode a count outside
 * 0..255 too), take no row and count in *file_rows; lines behind the range are counted and dropped, as lines beyond the table always
 * were, but no longer stop the rows of the same chunk from being stored.  majmin then holds the selectors of the range's m rows.
 * wgs_depth_ingest_stats, stats[0..7]: largest single host buffer held, in bytes | device ms (copies + kernels) | lines parsed
 * on the host | text bytes | data lines | chunks | BGZF members inflated on the device | ms of the tokeniser kernel alone
 * (0 unless WGSASSIGN_INGEST_TIME_KERNEL is set: timing it costs a synchronisation per chunk). */
#define WGS_DEPTH_PAIRS 0
#define WGS_DEPTH_COUNTS 1
typedef struct wgs_depth_ingest wgs_depth_ingest;
int wgs_depth_ingest_create(wgs_depth *d, wgs_reader *r, int mode, const uint8_t *majmin, int64_t limit_rows, int64_t chunk_bytes,
                            wgs_depth_ingest **out);
void wgs_depth_ingest_destroy(wgs_depth_ingest *g);
int wgs_depth_ingest_set_first_row(wgs_depth_ingest *g, int64_t first_row);
int wgs_depth_ingest_next(wgs_depth_ingest *g, int64_t row0, int64_t *file_rows, int64_t *rows_written);
int wgs_depth_ingest_stats(wgs_depth_ingest *g, double *stats);
int wgs_zscore_max_depth(void);
/* zscore.AD_summary, the dictionary (zscore.py:11-21), for individuals [i0, i0 + count) in ONE launch: per (individual, class)
 * the number of sites, the float32 sums of (g0, g1, 1 - g0 - g1) in site order (np.mean's numerator; the caller divides), the
 * first site of the class (-1: none; the dictionary's insertion order) and per individual the sites deeper than
 * wgs_zscore_max_depth(), which have no class here (the caller lists them with wgs_zscore_deep_sites, or refuses such data).
 * counts_out / first_out: [count][WGS_Z_CLASSES]; sums_out: [count][WGS_Z_CLASSES][3]; over_out: [count]. */
int wgs_zscore_classes(wgs_depth *d, int32_t i0, int32_t count, int32_t *counts_out, float *sums_out, int32_t *first_out,
                       int32_t *over_out);
/* The same dictionary when the sites are cut into SNP shards, one per rank of `comm` (collective: every rank calls it with the same
 * i0 and count; comm = NULL: one shard).  The three float32 sums are serial chains in site order and do not associate, so the sweep
 * goes from shard to shard: for r = 0 .. world - 1 rank r walks its shard -- from 0 when r = 0, else from the running sums hop r - 1
 * left on the device (a class without a site in the shard hands them on untouched) -- and broadcasts count x 256 x 3 float32 on the
 * context's stream (op WGS_OP_Z_CLASS, iteration = the hop, shape_a = i0; the broadcast's own row carries the root and the payload
 * size, i.e. count).  One host all-reduce (same op, iteration = world, shapes i0 / count) then adds the counts and gathers first
 * sites and `over`.  On every rank: counts_out = sites of ALL shards, sums_out = the sums after the last shard, first_out = the
 * smallest GLOBAL site number (site0 + local) of a class, -1: none; over_out[r][j] = rank r's sites deeper than
 * wgs_zscore_max_depth() of individual i0 + j ([world][count]; each rank lists its own with wgs_zscore_deep_sites).  The sweep is
 * serial across ranks: rank r waits for hop r - 1; a (batch, hop) step depends on nothing but that, so batches could be skewed over
 * the ranks -- not done here.  A rank out of step fails with "collective mismatch". */
int wgs_zscore_classes_sharded(wgs_depth *d, int32_t i0, int32_t count, wgs_comm *comm, int32_t *counts_out, float *sums_out,
                               int64_t *first_out, int32_t *over_out);
/* The sites deeper than wgs_zscore_max_depth() of individuals [i0, i0 + count), per individual in site order, the individuals one
 * after the other: over[j] = the number wgs_zscore_classes reported for individual j (the sizes of the outputs; rc 2 if the
 * table says otherwise).  site_out[e] = site index, depth_out[e][0..1] = (Ar, Aa), g_out[e][0..1] = (g0, g1) of the matrix.  One
 * ballot word per (individual, tile) from the depth table, a scan, and a gather that reads the slabs only where a word is set. */
#define WGS_Z_DEEP_MAX 510
int wgs_zscore_deep_sites(wgs_depth *d, int32_t i0, int32_t count, const int32_t *over, int32_t *site_out, int32_t *depth_out,
                          float *g_out);
/* zscore.get_L_keep (zscore.py:43-61) for individuals [i0, i0 + count) in one launch.  key_comp[j][class] = -1: the class did
 * not survive the key filter; otherwise the component (0..2) at which its mean is largest, key_mean[j][class] that mean.  A site
 * is kept when its class survived and its own value at that component is within float32(0.01) of the mean.  kept_out[j] = sites
 * kept.  The set stays on the device (one bit per site + the positions in the compacted order) for wgs_zscore_stats and
 * wgs_em_fit_masked; destroyed with its matrix or depth table. */
int wgs_zkeep_create(wgs_depth *d, int32_t i0, int32_t count, const float *key_mean, const int32_t *key_comp, int64_t *kept_out,
                     wgs_zkeep **out);
/* ... with a deep table: deep_map[j][d], d = 0 .. WGS_Z_DEEP_MAX, = the first of the d + 1 rows of depth d in deep_rows, or -1
 * (depth not kept; always -1 for d <= wgs_zscore_max_depth()); deep_rows[r][0..7], row r = deep_map[j][d] + a for a = 0 .. d:
 * [0] the component (0, 1 or 2) at which the mean of class (Ar = d - a, Aa = a) is largest, [1] that mean, [2..4] AD_like and
 * [5..7] AD_factorial at AD_index[a, d - a] (transposed, as in wgs_zscore_stats' tables).  A site of a kept deep depth is then
 * filtered like any other, and wgs_zscore_stats runs its loops over these rows, which stay in global memory.  deep_map = NULL:
 * wgs_zkeep_create.  rc 2 for a map that points outside the n_deep_rows rows. */
int wgs_zkeep_create_deep(wgs_depth *d, int32_t i0, int32_t count, const float *key_mean, const int32_t *key_comp,
                          const int32_t *deep_map, const float *deep_rows, int64_t n_deep_rows, int64_t *kept_out, wgs_zkeep **out);
void wgs_zkeep_destroy(wgs_zkeep *zk);
/* L_keep of individual i0 + slot: the kept sites' indices, ascending (kept_out[slot] of them). */
int wgs_zkeep_sites(wgs_zkeep *zk, int32_t slot, int32_t *sites_out);
/* zscore_cy.expected_W_l / variance_W_l (zscore_cy.pyx:10-57) for every kept site of every individual of the set in one launch.
 * tables[j][class d (d + 1) / 2 + a][0..5] = AD_like[r][0..2], AD_factorial[r][0..2] for r = AD_index[a, d - a] (the reference
 * reads the index transposed); freq_dev[j] = DEVICE pointer to the m frequencies individual j is tested against (a column of a
 * wgs_afset, a fit of a wgs_em).  Outputs (host): the individuals' compacted arrays one after the other, kept_out[j] floats
 * each, in site order -- W_l_obs per site, W_l, var_W_l; the caller forms NumPy's pairwise float32 sums of them. */
int wgs_zscore_stats(wgs_zkeep *zk, const float *tables, const float *const *freq_dev, float *wobs_out, float *wl_out, float *var_out);
/* emMAF.emMAF on the rows L[L_keep] (WGSassign.py:361) for every fit of the batch: the per-site update does not depend on which
 * other sites are present, so the sweeps are wgs_em_step's over all sites; the convergence metric (emMAF_cy.rmse1d, a serial
 * float32 chain) runs over the kept sites of individual i0 + fit_slot[j] of `zk` only and divides by their number.
 * iters_out[j] = iteration at which fit j converged, 0 if max_iter was exhausted.  One SNP shard. */
int wgs_em_fit_masked(wgs_em *em, wgs_zkeep *zk, const int32_t *fit_slot, int32_t max_iter, double tole, int32_t *iters_out);
/* ... across SNP shards (collective; comm = NULL: one shard).  `em` and `zk` are this rank's shard; the sweeps are local and no sum is
 * all-reduced, since every iteration is decided by the exact chain: it crosses the shards in rank order on the stream as wgs_em_fit's
 * chains do (rank r sets its carries from hop r - 1's and broadcasts nj float32: op WGS_OP_Z_CHAIN, iteration = the EM iteration,
 * shape_a = fits still active), and the divisor is kept_total[slot], the individual's kept sites over ALL ranks ([zk's count]).  Every
 * rank takes the same decision from the same broadcast value.  An individual that kept no site in this shard hands its carry on;
 * rc 2 only when kept_total[slot] is 0. */
int wgs_em_fit_masked_sharded(wgs_em *em, wgs_zkeep *zk, const int32_t *fit_slot, int32_t max_iter, double tole,
                              const int64_t *kept_total, wgs_comm *comm, int32_t *iters_out);

/* ---- --get_assignment_z_score in site windows: what is defined over all sites of an individual is continued
 * from window to window on the device.  A wgs_zsum holds, for `count` individuals, (a) the running sums of the class sweep and (b) per
 * (individual, array) of the three per-site arrays the state of np.sum's float32 order: NumPy adds the sums of consecutive
 * 8192-element chunks -- each its pairwise routine's tree over 64 leaves of 128 -- serially to a running float32 that starts at +0.0,
 * so the state is that running value and the fewer than 8192 elements of the open chunk.  Added under ABI version 4: new symbols only. */
typedef struct wgs_zsum wgs_zsum;
int wgs_zsum_create(wgs_ctx *ctx, int32_t count, wgs_zsum **out);
void wgs_zsum_destroy(wgs_zsum *zs);
/* wgs_zscore_classes for the next window of a pass: `d` is the depth table of the window's matrix.  The first call on a state runs
 * the sweep from 0, every later one from the running sums the call before left on the device (a class without a site in the window
 * hands them on untouched).  counts_out, first_out (LOCAL site numbers, -1: none) and over_out speak of this window alone -- the
 * caller adds counts and `over` and keeps the smallest site0 + first -- and sums_out are the running sums after this window. */
int wgs_zscore_classes_carry(wgs_depth *d, int32_t i0, int32_t count, wgs_zsum *zs, int32_t *counts_out, float *sums_out, int32_t *first_out,
                             int32_t *over_out);
/* wgs_zscore_stats that downloads nothing: *dev_out = DEVICE pointer to [3][*all_out] floats -- W_l_obs, W_l, var_W_l, inside each
 * the individuals' compacted arrays one after the other (kept_out[j] floats each) -- owned by `zk`, valid until its next call of
 * this function or its destruction.  *all_out = 0 (and *dev_out = NULL) when nobody kept a site. */
int wgs_zscore_stats_dev(wgs_zkeep *zk, const float *tables, const float *const *freq_dev, const float **dev_out, int64_t *all_out);
/* A window's arrays into the sums: dev_arrays as wgs_zscore_stats_dev leaves them ([3][all], device), kept[j] elements of individual
 * slot j.  Per (individual, array) the push completes the open chunk with the first elements, reduces every full chunk in NumPy's order
 * (all chunks of all individuals and arrays in one launch), adds the chunk sums to the running value in chunk order and stores the new
 * open chunk.  Waits for the stream: the arrays may be released when it returns. */
int wgs_zsum_push(wgs_zsum *zs, const float *dev_arrays, int64_t all, const int64_t *kept);
/* total_out[j] = elements pushed for individual slot j so far; total % 8192 of them are in its open chunk. */
int wgs_zsum_totals(wgs_zsum *zs, int64_t *total_out);
/* run_out[j][a] = the running float32 over the closed chunks; tails_out = the open chunks, packed: for j, for a = 0..2, total[j] % 8192
 * floats.  The caller closes the sum as NumPy does: run + np.sum(tail) -- exact, because a running value that started at +0.0 is
 * never -0.0 -- and adds nothing for an empty tail. */
int wgs_zsum_finish(wgs_zsum *zs, float *run_out, float *tails_out);
/* Rows [src_row0, src_row0 + nrows) of one depth table into rows dst_row0 .. of another of the same individuals, on the device: a depth
 * file is read ONCE per pass through a small table of its own (one chunk of the file at a time) and its rows go on to the window's
 * table from there, whichever window edge the chunk straddles. */
int wgs_depth_copy_rows(wgs_depth *dst, int64_t dst_row0, wgs_depth *src, int64_t src_row0, int64_t nrows);
/* WGS_DEPTH_COUNTS: the selectors of the table's rows 0 .. nrows - 1 for the chunks to come (majmin[row][2], each 0..3), in place of
 * those wgs_depth_ingest_create was given -- for an ingest whose table takes every chunk at row 0. */
int wgs_depth_ingest_set_selectors(wgs_depth_ingest *g, const uint8_t *majmin, int64_t nrows);

/* ---- --get_reference_z_score in site windows: the leave-one-out fit of every individual's population whose
 * stopping test runs over THAT individual's kept sites (wgs_em_fit_masked), window by window.  wgs_em_stream_push_masked is
 * wgs_em_stream_push_keep without sums, plus the window's kept-site set: the exact chain of (fit, t) named in chain_fit / chain_iter runs
 * over (f_t, f_t-1) at the sites slot fit_slot[fit] of `zk` kept in this window, compacted in site order (every chain job of an iteration
 * by one launch), goes on from C[t][fit] and leaves its carry there -- as the chain of wgs_em_fit_masked_sharded goes from SNP shard to
 * SNP shard.  A fit whose individual kept nothing in this window hands C[t][fit] on bit for bit.  A final fit is clamped and stays in
 * the batch (wgs_em_f_dev).  Nothing joins S, nothing of the window's size crosses to the host, and nothing is read back between the
 * iterations: the host reads C once per round (wgs_em_stream_read) and decides with wgs_em_fit_masked's rule, carry against the
 * kept sites of ALL windows.  The compacted vectors (2 x n_fits x the window's largest kept count, zero behind a fit's own count) are
 * the stream's and grow when a window needs more.  Refused before any launch (rc 2): what wgs_em_stream_push_keep refuses, a `zk` made
 * from another matrix than the batch's, a fit_slot outside `zk`, a chain of an iteration beyond its fit's run_iters.  `zk` and its
 * depth table must be destroyed before wgs_em_stream_move_window moves the matrix.  Added under ABI version 4: a new symbol only. */
int wgs_em_stream_push_masked(wgs_em_stream *stream, wgs_em *window_em, wgs_zkeep *zk, const int32_t *fit_slot, const int32_t *run_iters,
                              const int32_t *final, const float *clamp_lo, const float *clamp_hi, const int32_t *chain_fit,
                              const int32_t *chain_iter, int32_t n_chain);

/* Blocks of 4096 elements that fell back to the serial loop in the last wgs_em_rmse_chain of an EM batch (diagnostics). */
int wgs_em_last_chain_serial_blocks(wgs_em *em);

/* Kernel time (HIP events on the context's stream) of the context's last wgs_assign / wgs_score_* call; -1 while the class
 * codes' memory is being allocated (wgs_beagle_codes_wait): ask again afterwards. */
int wgs_assign_last_ms(wgs_ctx *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* WGSASSIGN_HIP_H */
