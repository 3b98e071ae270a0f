/*
 * wgsassign_hip_debug.h -- test hooks of libwgsassign_hip.so: entry points that exist for the test suite and the
 * micro-benchmarks (cross-check kernels, exhaustive checks of the arithmetic building blocks, host-only drivers of the
 * reader's hand-overs).  NOT part of the drop-in boundary (include/wgsassign_hip.h): nothing on the product path calls them,
 * and they may change without a bump of WGS_ABI_VERSION.
 */
#ifndef WGSASSIGN_HIP_DEBUG_H
#define WGSASSIGN_HIP_DEBUG_H

#include "wgsassign_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Named process-wide switches of the test suite (the product path reads no environment variable for them; 0 = off):
 *   codes_alloc_delay_ms              the helper thread's hipMalloc of the class codes' memory takes this much longer
 *   codes_alloc_release_after_sweeps  ... and is handed over only once the matrix has been swept directly this many times (or after
 *                                     2 s): which sweep of a fit finds the codes is then decided by a count, not by a race
 *   em_fuse_without_agreement         wgs_em_fit runs two iterations per sweep whenever THIS rank can, without the ranks' agreement
 *                                     (replays the defect of commit 807a461: the collectives' tags must catch it)
 *   em_coded_extra_lds                bytes of LDS em_coded_kernel requests beyond its table (occupancy experiment)
 *   staging_bytes                     size of the device buffer wgs_beagle_upload_rows / wgs_beagle_download_rows stage their rows through
 *                                     (0 = the 256 MB of the product: their loops then run once for anything a test can afford) */
int wgs_debug_hook(const char *name, int64_t value);

/* The literal one-lane-per-chain kernel behind wgs_assign_parts_exact, whatever P. */
int wgs_debug_parts_exact_literal(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int32_t P,
                                  const float *carry_in, float *parts_out);

/* BGZF inflate on the device (csrc/inflate.hip; RFC 1951, one lane per block): `nblocks` raw deflate streams -- BGZF members
 * without header and trailer -- lying in the host buffer `comp` (in_off, in_len) are inflated into `out` (out_off, isize);
 * status[i] != 0 marks a stream the device did not accept (the host inflates those).  *kernel_ms: the kernel alone. */
int wgs_debug_inflate(wgs_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, const uint64_t *in_off, const uint32_t *in_len,
                      const uint64_t *out_off, const uint32_t *isize, int32_t nblocks, uint8_t *out, int64_t out_bytes,
                      uint8_t *status, float *kernel_ms);

/* Test hook, needs no GPU: drains the reader through the text hand-over (producer thread, carried partial lines,
 * parallel newline scan, row limit) with ordinary memory and the host parser in place of the device tokeniser. */
int wgs_debug_reader_text_rows(wgs_reader *r, int64_t chunk_bytes, int64_t limit_rows, float *rows, int64_t max_rows, int64_t *nrows);
int64_t wgs_debug_reader_text_chunks(wgs_reader *r);   /* chunks that hand-over produced */
/* The same for an integer table (wgs_reader_open_table): every listed line through the host parser of flagged lines, `need`
 * columns each; linenos[i] = the 1-based line of row i in the file.  rc 2: a short line or a token np.loadtxt refuses. */
int wgs_debug_reader_table_rows(wgs_reader *r, int64_t chunk_bytes, int32_t need, int32_t *rows, int64_t max_rows, int64_t *nrows,
                                int64_t *linenos);
/* That parser on one line: 0 = ok, 1 = fewer than `need` columns, 3 = a token that is no int32 by np.loadtxt's rules. */
int wgs_debug_table_parse_line(const char *line, int64_t len, int32_t need, int32_t *out);
/* Test hook, needs no GPU: the COMPRESSED hand-over of a BGZF file (what the device-resident ingest consumes: whole members
 * in caller-allocated staging + the text the header calls had inflated already), inflated on the host into text[0 .. cap).
 * info[0..3] = chunks, members, largest text of one chunk, chunks that carried pre-inflated text. */
int wgs_debug_reader_comp_text(wgs_reader *r, int64_t comp_bytes, int64_t text_cap, int nbuf, char *text, int64_t cap, int64_t *bytes,
                               int64_t *info);

/* Test hooks for the convergence chain: wgs_rmse1d's value through the literal one-lane serial
 * kernel (serial != 0) or through the block-parallel exact emulation, reporting the number of
 * 4096-element blocks that fell back to the serial loop; the same count for the last
 * wgs_em_rmse_chain of an EM batch. */
int wgs_debug_rmse1d(wgs_ctx *ctx, const float *v1, const float *v2, int64_t m, double *out, int serial,
                     int *serial_blocks);
/* n_jobs chains of m elements each at once (a, b: n_jobs x m on the host), the way a later SNP shard of a batch of fits runs them: the
 * jobs are built with carry 0, chain_set_carry_kernel then sets carry_in[j] from a device array, and launch_rmse_chain_batch walks
 * them.  carry_out[j]: the running float32 value after job j (NOT divided by m); serial_blocks[j]: blocks that took the literal
 * loop.  With nblocks = ceil(m / 4096), expo ([n_jobs][nblocks], may be NULL) receives what rmse_predict_kernel predicted and cand
 * ([n_jobs][nblocks][6], may be NULL) what rmse_candidates_kernel composed: cand[..][2 * c + p] for the biased exponent
 * expo - 1 + c and the entry mantissa's parity p. */
int wgs_debug_rmse_chain_batch(wgs_ctx *ctx, const float *a, const float *b, int32_t n_jobs, int64_t m, const float *carry_in,
                               float *carry_out, int32_t *serial_blocks, int32_t *expo, int64_t *cand);

/* Sweeps this EM batch has enqueued so far through each of its four sweep kernels (csrc/em_api.hip: em_enqueue_sweep):
 * counts[0] em_sweep_kernel, [1] em_sweep_group_kernel, [2] em_coded_kernel, [3] em_coded_group_kernel.  A sweep counts once
 * however many launches it takes and however many iterations it runs. */
int wgs_debug_em_sweep_paths(wgs_em *em, int64_t counts[4]);

/* What the last build of the class codes left for this matrix (csrc/common.h: wgs_codes), copied to the host and de-interleaved;
 * waits for the codes' memory (wgs_beagle_codes_wait), builds nothing, and fails (rc 2) when no codes are built.  Every array but
 * geom may be NULL (a first call learns the sizes).  tiles = ceil(m / 64); slabs follow each other in population order.
 *   geom[0] hash slots per SNP, [1] drows, [2] lrows, [3] score_batch, [4] 1 when the slabs' own numbering was built, [5] slabs,
 *        [6] tile_rows bytes per tile, [7] classes an aligned group of score_batch SNPs may sum to
 *   ncls       [m]
 *   dict       [m][drows][2]             the (g0, g1) bit patterns of class 0 .. drows - 1 of the SNP (rows beyond ncls: whatever was there)
 *   codes      [m][n]                    class byte of every individual, the individuals of slab 0 first (slab order within a slab)
 *   lcodes     [m][n]                    the same in the slab's own numbering            (untouched unless geom[4])
 *   ldict      [slabs][m][lrows][2]      the slab's own dictionary                        (untouched unless geom[4])
 *   tile_rows  [slabs][tiles][geom[6]] */
int wgs_debug_codes_download(wgs_beagle *b, int32_t geom[8], uint8_t *ncls, uint32_t *dict, uint8_t *codes, uint8_t *lcodes, uint32_t *ldict,
                             uint8_t *tile_rows);

/* Test hook for the EM kernel's correctly rounded divide (csrc/em_kernels.hip: div_exact): number of
 * 2^20 x per_thread pseudo-random EM-shaped operand pairs whose quotient differs bitwise from the
 * compiler's IEEE double divide. */
int wgs_debug_div_mismatch(wgs_ctx *ctx, uint64_t seed, uint64_t per_thread, uint64_t *mismatch);
/* ... over the operands the enumerated EM terms show to exist (tests/em_cases.py): p2 of either sign, sums that cancel to a few ulps,
 * negative numerators, denominators from the smallest float32 subnormal to 2^127, |num| / den from 2^-277 to 2^277.  mismatch[0]: the
 * divide with its fixup, over all pairs; mismatch[1]: the fixup-free form of the hot loop, over the pairs with a positive finite
 * denominator and a finite numerator (its precondition). */
int wgs_debug_div_mismatch_signed(wgs_ctx *ctx, uint64_t seed, uint64_t per_thread, uint64_t mismatch[2]);
/* ... and the accuracy of its once-refined reciprocal: the largest relative error over ALL 2^23 float32 mantissas of
 * the denominator at binary exponent `exponent` (its exactness argument needs < 2^-48; see em_kernels.hip). */
int wgs_debug_rcp_error(wgs_ctx *ctx, int exponent, double *max_rel);

/* Test hooks for the assignment kernel's double-precision log of float32 arguments
 * (csrc/assign_kernels.hip: log_f32arg): number of float32 bit patterns in [b0, b1) whose
 * float32-rounded log differs from the device math library's, and the values themselves. */
int wgs_debug_log_mismatch(wgs_ctx *ctx, uint32_t b0, uint32_t b1, uint64_t *count, uint32_t *first);
int wgs_debug_log_values(wgs_ctx *ctx, const float *x, float *out, int64_t n, int use_libm);

/* Test hooks for the two hardware steps of the float32 modes (csrc/fast_math.h; which = 0: fast_log, the natural log the scoring
 * kernels take of a likelihood sum; 1: fast_rcp, the reciprocal the EM kernels multiply by): the values for n float32 arguments, and
 * an exhaustive pass over the bit patterns [b0, b1) against the correctly rounded function on the device -- log_f32arg((double)x),
 * or the IEEE double division 1.0 / (double)x:
 *   stats[0] the largest error in float32 ulps of the true value (ulp of a value below 2^-126: 2^-149), [1] the first argument (bit
 *            pattern) that attains it, [2] the largest error as it is, [3] its first argument -- both over the arguments for which
 *            the result and the true value are finite and not zero (-1 and 0 where there is none);
 *   stats[4] arguments whose result is of another class -- finite, -inf, +inf, NaN, zero -- than the true value rounded to
 *            float32, [5] the first of them (-1: none). */
int wgs_debug_fast_values(wgs_ctx *ctx, int which, const float *x, float *out, int64_t n);
int wgs_debug_fast_scan(wgs_ctx *ctx, int which, uint32_t b0, uint32_t b1, double stats[6]);

/* Test hook for the one step of the synthetic generators (csrc/beagle_kernels.hip) that goes through the device math library: the
 * population frequency pop_freq (cospif, logf, sqrtf) of the m global sites site0 .. site0 + m - 1 of one group, as synth_kernel and
 * synth_quality_kernel take it (the same device function), and the expf(-depth) their Poisson inversion starts from.  Everything else
 * of the generators is plain IEEE arithmetic, which tests/synth_twin.py restates exactly from these two. */
int wgs_debug_synth_freq(wgs_ctx *ctx, uint64_t seed, int64_t site0, int64_t m, int32_t group, double depth, float *p_out, float *cdf0_out);

/* The m values at wgs_afset_col_dev(a, col), copied to the host on the context's stream: what a kernel handed that pointer reads. */
int wgs_debug_afset_col(wgs_afset *a, int32_t col, float *out);

/* The sums of the last wgs_score_sums per chunk of 8192 sites (the addends of np.sum's running float64 total): out (NULL: only
 * *nchunks is set) receives ceil(blocks / 2) x n*K float64, out[c * n*K + i * K + k]. */
int wgs_debug_score_chunks(wgs_score *sc, double *out, int64_t *nchunks);

/* The three kernels that turn the scoring sweeps' 4096-site block sums into the n x K float64 totals (csrc/assign_kernels.hip), each
 * launched ONCE through the launcher of the product path on host arrays the caller makes up; `cells` stands for n*K.
 *   block_prefix   S (nblocks x cells, read and rewritten): out[cell] = the blocks added in np.sum's order, total = total +
 *                  (S[2c] + S[2c+1]); with keep_prefix S[b] becomes the total before block b's chunk (b even) or that + the old
 *                  S[b - 1] (b odd), otherwise S comes back unchanged; chunks (NULL: the kernel is handed a null pointer) receives
 *                  ceil(nblocks / 2) x cells chunk sums.  nblocks = 0 is allowed (S may be NULL).
 *   chunk_total    out[cell] = ((carry + C[0]) + C[1]) + ... over nchunks x cells chunk sums; carry NULL: from 0.0.
 *   combine_parts  S[e] = ((Sp[0][e] + Sp[1][e]) + ...) over parts x total partial sums. */
int wgs_debug_block_prefix(wgs_ctx *ctx, double *S, int32_t nblocks, int64_t cells, int keep_prefix, double *out, double *chunks);
int wgs_debug_chunk_total(wgs_ctx *ctx, const double *chunks, int32_t nchunks, int64_t cells, const double *carry, double *out);
int wgs_debug_combine_parts(wgs_ctx *ctx, const double *Sp, int64_t total, int32_t parts, double *S);

/* What the last wgs_score_sums of this object decided before it enqueued anything (csrc/score_api.hip: score_plan_sums):
 * info[0] 0 = the sweep over the float32 slabs, 1 = through the class codes; [1] populations per register batch and [2] pairs of
 * individuals per wavefront of the sweep; [3], [4] the same of the chain kernel of wgs_score_chains_prepare (both known from
 * wgs_score_create on); and of the coded sweep (0, 0, 1 otherwise): [5] SNPs per table, [6] bytes per table element, [7] workgroups
 * that share a block. */
int wgs_debug_score_plan(wgs_score *sc, int32_t info[8]);

/* The two device kernels around a tagged RCCL collective (csrc/rccl_comm.hip: the row every rank writes behind the payload, the
 * comparison of all ranks' rows with one's own behind the all-reduce) on rows made up by the caller: what the ranks of a world-rank
 * job would run -- RCCL refuses two ranks on one GPU, so no test reaches them otherwise.  rows: world x 8 float64 {sequence number,
 * step, generation, iteration, shape, shape, payload elements, free word}; as_rank: whose check runs.  fault_out (18 float64):
 * [0] = 1 when the check reported a difference, [1] the other rank, [2..9] this rank's row, [10..17] the other's. */
int wgs_debug_comm_tag_kernels(wgs_ctx *ctx, int32_t world, const double *rows, int32_t as_rank, double *fault_out);

/* Test hook for the window-to-window float32 sums (wgs_zsum_*): a push of HOST arrays -- host_arrays[3][all], inside each the
 * individuals' kept[j] elements one after the other -- through the kernels of wgs_zsum_push.  A state comes from wgs_zsum_create and is
 * read with wgs_zsum_totals / wgs_zsum_finish. */
int wgs_debug_zsum_push(wgs_zsum *zs, const float *host_arrays, int64_t all, const int64_t *kept);

/* Cross-check only: FLOAT64 partition sums parts[(i*P + p)*K + k] (labels = global site index % P) and totals from the
 * round-1 kernel (lanes <-> pairs of individuals, tile ranges combined with float64 atomics): ~1e-5 from the
 * reference's serial float32 partition sums, not reproducible run to run.  Not on the product path. */
int wgs_debug_assign_parts_f64(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int32_t P, int mode,
                               double *out, double *parts);

#ifdef __cplusplus
}
#endif
#endif /* WGSASSIGN_HIP_DEBUG_H */
