// Scoring of the C ABI (include/wgsassign_hip.h: wgs_score_*, wgs_assign, wgs_loo, exact partition sums): glassy.py:18-112 and
// utils.py:129-151 on device-resident data.  Host-side orchestration only; the arithmetic is in assign_kernels.hip.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>

#include "common.h"
#include "em_state.h"
#include "stream_checks.h"
#include "streams.h"

struct wgs_score {
    wgs_beagle *b = nullptr;
    wgs_afset *a = nullptr;
    int32_t K = 0, row_lo = 0, row_hi = 0, nblocks = 0, P = 0;
    int64_t n = 0, cells = 0;
    bool per_ind = false, have_prefix = false;
    const float **d_acol = nullptr, **d_colptr = nullptr;
    ScoreSlab *d_slabs[2] = {nullptr, nullptr};      // [0] table of the sweep, [1] table of the chain kernel
    int n_slabs[2] = {0, 0}, total_pg[2] = {0, 0};
    double *d_S = nullptr, *d_out = nullptr, *d_start = nullptr, *d_run = nullptr, *d_chunks = nullptr;     // d_chunks: [ceil(nblocks/2)][cells]
    uint32_t *d_cand = nullptr;
    float *d_carry = nullptr, *d_parts = nullptr;
    int32_t *d_nserial = nullptr;
    int32_t last_serial_blocks = 0;
    CodedSlab *d_coded = nullptr;         // slab table of the sweep through the class codes (shared columns)
    int n_coded = 0, coded_quads = 0;     // its records and the quads of individuals they cover
    int64_t coded_generation = -1;        // wgs_codes::generation of the build d_coded was made from
    ScorePlan plan;                       // the shape since wgs_score_create, all of it of the last wgs_score_sums (wgs_debug_score_plan)
};

/* f(g, slab, col_lo, col_hi) for every population slab that holds individuals of [row_lo, row_hi): the members of a slab are in
 * file order, so those are a contiguous column range. */
template <class F>
static void for_scored_slabs(const wgs_beagle *b, int64_t row_lo, int64_t row_hi, F f)
{
    for (int g = 0; g < b->n_groups; ++g) {
        const Slab &s = b->slabs[g];
        const int lo = (int)(std::lower_bound(s.members.begin(), s.members.end(), row_lo) - s.members.begin());
        const int hi = (int)(std::lower_bound(s.members.begin(), s.members.end(), row_hi) - s.members.begin());
        if (hi > lo) f(g, s, lo, hi);          // (an empty slab has no members)
    }
}

// A slab table in pooled device memory (*d: what it replaces, or nullptr; stays nullptr for an empty table)
template <class T>
static int upload_table(wgs_ctx *ctx, const std::vector<T> &tab, T **d)
{
    if (*d) wgs_pool_free(ctx, *d);
    *d = nullptr;
    if (tab.empty()) return 0;
    HIP_TRY(wgs_pool_malloc(ctx, d, sizeof(T) * tab.size()));
    HIP_TRY(hipMemcpy(*d, tab.data(), sizeof(T) * tab.size(), hipMemcpyHostToDevice));
    return 0;
}

// d_acol[k] = column k of the frequency set; `host` holds the pointers until the caller has synchronised `stream` (nullptr: a blocking copy)
static hipError_t upload_columns(const wgs_afset *a, std::vector<const float *> &host, const float **d_acol, hipStream_t stream)
{
    host.resize(a->K);
    for (int k = 0; k < a->K; ++k) host[k] = a->buf + (size_t)k * a->m;
    if (!stream) return hipMemcpy(d_acol, host.data(), sizeof(float *) * a->K, hipMemcpyHostToDevice);
    return hipMemcpyAsync(d_acol, host.data(), sizeof(float *) * a->K, hipMemcpyHostToDevice, stream);
}

// The buffers a wgs_score allocates when first needed and keeps
template <class T>
static hipError_t grow_once(wgs_score *sc, T **p, size_t bytes) { return *p ? hipSuccess : wgs_pool_malloc(sc->b->ctx, p, bytes); }

// KB = populations per register batch: the batch size with the fewest passes over K, then the least padding.
// Every pass re-reads the block's GLs, so K <= 10 is ONE pass (HBM traffic = algorithmic bytes) and K = 20 two;
// KB = 9, 10 run one pair per wave at 2 waves/SIMD (measured equal to two passes of 5 in exact mode -- the kernel is
// bound by FP64 issue either way -- and 11 % faster in float32 mode).
static int pick_kb(int K, int kb_max = 10)
{
    int best = 4, best_cost = 1 << 30;
    for (int kb = 4; kb <= kb_max; ++kb) {
        const int passes = (K + kb - 1) / kb;
        const int cost = passes * 1000 + passes * kb - K;
        if (cost < best_cost) best_cost = cost, best = kb;
    }
    return best;
}

/* The shape of the plan -- register batches and pairs per wave, which the slab tables are built for: wgs_score_create and every
 * launch take it from here.  The chain kernel (and the WGSASSIGN_PARTS=fast cross-check kernel) stays with batches of at most 8
 * populations (9 and 10 would spill). */
static ScorePlan score_plan_shape(int K, bool per_ind)
{
    ScorePlan p;
    p.kb = pick_kb(K);
    p.np = sweep_pairs(p.kb, per_ind);
    p.chain_kb = pick_kb(K, 8);
    p.chain_np = chain_pairs(p.chain_kb, per_ind);
    return p;
}

// The block-parallel chains take P partitions while their tables fit 64 KiB of LDS and a chain's index 31 bits; else the literal chains
static bool chains_block_parallel(const ScorePlan &p, int64_t cells, int32_t P)
{
    return chain_cand_lds_bytes(p.chain_kb, p.chain_np, P) <= 64 * 1024 && cells * P < (1ll << 31);
}

// The environment switches of scoring, read once per wgs_score_sums (tests and tools/probe_score_parts.py change them between calls)
struct ScoreSwitches {
    const char *env_table = getenv("WGS_SCORE_CODED_TABLE"), *env_parts = getenv("WGS_SCORE_CODED_PARTS");
    char coded_table = env_table ? env_table[0] : 0;        // = f | d: float / float64 rows of the 16-SNP table whatever KB (experiments)
    int coded_parts = env_parts ? atoi(env_parts) : 0;      // = 1 .. 16: workgroups per block of the coded sweep (experiments)
};

/* Slab table for NP pairs per wave, restricted to the individuals [row_lo, row_hi). */
static int build_slab_table(wgs_score *sc, int np, int which)
{
    std::vector<ScoreSlab> tab;
    int pg = 0;
    for_scored_slabs(sc->b, sc->row_lo, sc->row_hi, [&](int, const Slab &s, int lo, int hi) {
        const int pair0 = lo / 2, npg = ((hi - 1) / 2 - pair0 + 1 + np - 1) / np;
        tab.push_back({s.base, s.d_members, s.npairs, s.ncols, pair0, npg, pg, lo, hi});
        pg += npg;
    });
    sc->n_slabs[which] = (int)tab.size();
    sc->total_pg[which] = pg;
    return upload_table(sc->b->ctx, tab, &sc->d_slabs[which]);
}

/* The same for the sweep through the class codes. */
static int build_coded_table(wgs_score *sc, const wgs_codes *codes)
{
    std::vector<CodedSlab> tab;
    int quad0 = 0;
    for_scored_slabs(sc->b, sc->row_lo, sc->row_hi, [&](int g, const Slab &s, int lo, int hi) {
        const SlabCodes &c = codes->slabs[g];
        tab.push_back({c.codes, s.d_members, s.base, c.nquads, s.ncols, quad0, lo, hi, s.npairs});
        quad0 += c.nquads;
    });
    sc->n_coded = (int)tab.size();
    sc->coded_quads = quad0;
    if (upload_table(sc->b->ctx, tab, &sc->d_coded)) return 1;
    sc->coded_generation = codes->generation;
    return 0;
}

/* The plan of one wgs_score_sums: through the class codes or over the float32 slabs and, for the coded sweep, its table and how many
 * workgroups share a block.  May build the codes and, for a new build of them, their slab table (its quads size the grid);
 * enqueues no sweep. */
static int score_plan_sums(wgs_score *sc, const ScoreSwitches &sw, ScorePlan *plan)
{
    wgs_ctx *ctx = sc->b->ctx;
    ScorePlan &p = *plan = score_plan_shape(sc->K, sc->per_ind);
    // shared columns + a codable matrix: the sweep through the class codes (same S, bit for bit)
    // (built for this sweep only when what it saves exceeds the encode pass: codes.hip: wgs_codes_pay_for_scoring)
    wgs_codes *codes = sc->per_ind ? nullptr : wgs_beagle_codes(sc->b, false);
    if (!codes && !sc->per_ind && wgs_codes_pay_for_scoring(sc->b, sc->K)) codes = wgs_beagle_codes(sc->b, true, false, true);
    if (!codes) return 0;
    // float table rows where they need (almost) no padding to 16 bytes, float64 rows (no conversion in phase 2) elsewhere
    // (the 8- and 4-SNP tables exist with float64 rows only)
    const bool wide = codes->score_batch < 16 || sw.coded_table == 'd' || (sw.coded_table != 'f' && ((p.kb + 3) & ~3) - p.kb > 1);
    const size_t lds = score_coded_lds_bytes(codes->rows_batch, p.kb, wide ? 8 : 4);
    if (lds > 64 * 1024) return 0;             // class table too large for LDS
    // (keyed on the build, not on the object's address: a rebuilt wgs_codes may reuse it)
    if (sc->coded_generation != codes->generation && build_coded_table(sc, codes)) return 1;
    p.codes = codes;
    p.score_batch = codes->score_batch;
    p.elem_bytes = wide ? 8 : 4;
    p.lds = lds;
    p.total_quads = sc->coded_quads;
    if (sc->b->m <= 0 || p.total_quads <= 0 || sc->K <= 0 || sc->nblocks <= 0) return 0;     // (nothing to sweep)
    const unsigned ygroups = (unsigned)((p.total_quads + 255) / 256);
    // A block's 64 tiles go to `parts` workgroups: enough of them to fill the chip (short matrices), and -- the workgroups all take
    // the same time -- a count that does not leave the last round of workgroups mostly empty: 2442 blocks on 768 places (3 per CU by
    // registers, fewer when the table is large) are 3.18 rounds, i.e. a fifth of the chip-time idle; in halves 6.36 of 7, in quarters
    // 12.7 of 13.
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(3, (160 * 1024) / std::max<size_t>(lds, 1)));
    const double places = (double)std::max(1, ctx->cus) * per_cu;
    // Any count from 1 to 16 whose runs of ceil(64 / parts) tiles are all non-empty (round 5, late: the powers of two alone left a
    // shard of 1.25M SNPs -- 306 blocks -- at 6.4 rounds of 7 with 16 parts; 5 parts are 1.99 rounds of 2).  The workgroups all take
    // about the same time, a run's tiles plus what a workgroup costs before its first one (the log table, the first batch's trips to
    // memory: about a tile's worth), so the split with the fewest rounds x (tiles per run + 1) wins -- tools/probe_score_parts.py
    // times every split: 5 at 1.25M SNPs (1.44 ms; 16: 1.59), 10 at 300 k (0.45 ms; 16: 0.46, 4: 0.73), 3-5 or 12 at 10M (within 2 %).
    auto usable = [](int q) { return (q - 1) * ((WGS_BLOCK_TILES + q - 1) / q) < WGS_BLOCK_TILES; };
    double best_cost = 0.0;
    for (int q = 1; q <= 16; ++q) {
        if (!usable(q)) continue;
        const double rounds = ceil((double)sc->nblocks * ygroups * q / places);
        const double cost = rounds * (double)((WGS_BLOCK_TILES + q - 1) / q + 1);
        if (q == 1 || cost < best_cost - 1e-9) p.parts = q, best_cost = cost;
    }
    if (sw.coded_parts >= 1 && sw.coded_parts <= 16 && usable(sw.coded_parts)) p.parts = sw.coded_parts;
    return 0;
}

extern "C" {

/* ------------------------------------------------------------------ assignment / scoring */

int wgs_assign_last_ms(wgs_ctx *ctx, float *ms)
{
    WGS_REQUIRE(ctx && ms, "null argument");
    if (ctx->assign_ms_pending) {
        if (ctx->allocs_in_flight.load() > 0) {              // the query would wait for that hipMalloc: not known yet (ask again later)
            *ms = -1.0f;
            return 0;
        }
        HIP_TRY(hipSetDevice(ctx->device));
        if (hipEventElapsedTime(&ctx->last_assign_ms, ctx->ev0, ctx->ev1) != hipSuccess) ctx->last_assign_ms = 0.0f;
        (void)hipGetLastError();
        ctx->assign_ms_pending = false;
    }
    *ms = ctx->last_assign_ms;
    return 0;
}

void wgs_score_destroy(wgs_score *sc)
{
    if (!sc || !wgs_live_remove(sc)) return;          // (destroyed already, e.g. together with its matrix or frequency set)
    (void)hipSetDevice(sc->b->ctx->device);
    (void)hipStreamSynchronize(sc->b->ctx->stream);
    void *bufs[] = {sc->d_acol, sc->d_colptr, sc->d_slabs[0], sc->d_slabs[1] == sc->d_slabs[0] ? nullptr : sc->d_slabs[1], sc->d_S,
                    sc->d_out, sc->d_start, sc->d_run, sc->d_coded, sc->d_cand, sc->d_carry, sc->d_parts, sc->d_nserial, sc->d_chunks};
    for (void *p : bufs)
        if (p) wgs_pool_free(sc->b->ctx, p);
    delete sc;
}

int wgs_score_create(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int32_t row_lo, int32_t row_hi, wgs_score **out)
{
    WGS_REQUIRE(b && a && out, "null argument");
    WGS_REQUIRE(a->m == b->m, "allele frequencies cover %lld SNPs, the Beagle shard %lld", (long long)a->m, (long long)b->m);
    WGS_REQUIRE(row_lo >= 0 && row_lo <= row_hi && row_hi <= b->n, "individual range [%d, %d) outside 0..%lld", row_lo, row_hi,
                (long long)b->n);
    wgs_ctx *ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    wgs_score *sc = new wgs_score();
    wgs_live_add(sc, WGS_LIVE_SCORE, b, a);
    auto guard = on_failure([&] { wgs_score_destroy(sc); });
    sc->b = b;
    sc->a = a;
    sc->K = a->K;
    sc->n = b->n;
    sc->cells = b->n * (int64_t)a->K;
    sc->row_lo = row_lo;
    sc->row_hi = row_hi;
    sc->per_ind = colptr != nullptr;
    sc->nblocks = (int32_t)((wgs_ntiles(b->m) + WGS_BLOCK_TILES - 1) / WGS_BLOCK_TILES);
    HIP_TRY(wgs_pool_malloc(ctx, &sc->d_acol, sizeof(float *) * a->K));
    std::vector<const float *> acol;
    HIP_TRY(upload_columns(a, acol, sc->d_acol, nullptr));
    if (colptr) {
        HIP_TRY(wgs_pool_malloc(ctx, &sc->d_colptr, sizeof(float *) * sc->cells));
        HIP_TRY(hipMemcpy(sc->d_colptr, colptr, sizeof(float *) * sc->cells, hipMemcpyHostToDevice));
    }
    sc->plan = score_plan_shape(a->K, sc->per_ind);
    if (build_slab_table(sc, sc->plan.np, 0)) return 1;
    if (sc->plan.chain_np == sc->plan.np) {
        sc->d_slabs[1] = sc->d_slabs[0];
        sc->n_slabs[1] = sc->n_slabs[0];
        sc->total_pg[1] = sc->total_pg[0];
    } else if (build_slab_table(sc, sc->plan.chain_np, 1)) {
        return 1;
    }
    if (wgs_pool_malloc(ctx, &sc->d_S, sizeof(double) * (size_t)sc->nblocks * sc->cells) != hipSuccess) {
        wgs_set_error("hipMalloc of %zu bytes for the block sums failed", sizeof(double) * (size_t)sc->nblocks * sc->cells);
        return 1;
    }
    HIP_TRY(wgs_pool_malloc(ctx, &sc->d_out, sizeof(double) * sc->cells));
    guard.dismiss();
    *out = sc;
    return 0;
}

static ScoreArgs score_args(const wgs_score *sc, int which)
{
    ScoreArgs A = {};              // (no start, no cand: wgs_score_chains_prepare sets them)
    A.slabs = sc->d_slabs[which];
    A.n_slabs = sc->n_slabs[which];
    A.total_pg = sc->total_pg[which];
    A.colptr = sc->d_colptr;
    A.acol = sc->d_acol;
    A.m = sc->b->m;
    A.site0 = sc->b->site0;
    A.cells = sc->cells;
    A.K = sc->K;
    A.P = 1;
    A.period = 1;
    A.nblocks = sc->nblocks;
    A.S = sc->d_S;
    return A;
}

// The sweep of the plan into sc->d_S (zeroed): one kernel, or the coded kernel in parts and their sum
static int score_enqueue_sweep(wgs_score *sc, const ScorePlan &p, int mode)
{
    wgs_ctx *ctx = sc->b->ctx;
    if (!p.codes) return launch_score_sweep(ctx, score_args(sc, 0), p.kb, p.np, mode);
    const int64_t total = (int64_t)sc->nblocks * sc->cells;
    double *S = sc->d_S;
    if (p.combine()) {
        void *ws = nullptr;
        if (wgs_ctx_workspace(ctx, sizeof(double) * (size_t)total * p.parts, &ws)) return 1;
        HIP_TRY(hipMemsetAsync(ws, 0, sizeof(double) * (size_t)total * p.parts, ctx->stream));   // rows outside the scored range stay 0
        S = reinterpret_cast<double *>(ws);
    }
    if (launch_score_coded(ctx, p, sc->d_coded, sc->n_coded, sc->d_acol, sc->b->m, sc->cells, sc->K, sc->nblocks, S, mode)) return 1;
    return p.combine() ? launch_combine_parts(ctx, S, sc->d_S, total, p.parts) : 0;
}

// Plans and enqueues one sweep of the scored individuals and the per-chunk sums behind it (sc->d_out: the sums of this matrix alone,
// sc->d_chunks: what a running total continues over); nothing is read back and nothing waits.
static int score_sums_enqueue(wgs_score *sc, int mode)
{
    wgs_ctx *ctx = sc->b->ctx;
    if (score_plan_sums(sc, ScoreSwitches(), &sc->plan)) return 1;
    HIP_TRY(hipMemsetAsync(sc->d_S, 0, sizeof(double) * (size_t)sc->nblocks * sc->cells, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    if (score_enqueue_sweep(sc, sc->plan, mode)) return 1;
    HIP_TRY(grow_once(sc, &sc->d_chunks, sizeof(double) * (size_t)((sc->nblocks + 1) / 2) * sc->cells));
    if (launch_block_prefix(ctx, sc->d_S, sc->nblocks, sc->cells, sc->d_out, 1, sc->d_chunks)) return 1;
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    return 0;
}

// np.sum's running total continued over the chunk sums of the last sweep: d_out = ((d_carry + C0) + C1) + ... (d_carry == nullptr:
// from zero).  What wgs_score_total_from hands from SNP shard to SNP shard and wgs_score_stream_push from window to window.
static int score_total_enqueue(wgs_score *sc, const double *d_carry, double *d_out)
{
    return launch_chunk_total(sc->b->ctx, sc->d_chunks, (sc->nblocks + 1) / 2, sc->cells, d_carry, d_out);
}

/* All n x K sums of glassy.py:31-42 / 92-105 for the scored individuals: out[i*K + k] (host, overwritten;
 * rows outside the scored range are 0) = the float64 sum over this shard's SNPs of the float32 per-site
 * values, formed in a fixed order (per lane over the tiles of a block, a fixed shuffle tree over lanes,
 * blocks in order): the same bits on every run. */
int wgs_score_sums(wgs_score *sc, int mode, double *out)
{
    WGS_REQUIRE(sc && out, "null argument");
    WGS_REQUIRE(mode == WGS_MODE_EXACT || mode == WGS_MODE_FAST, "unknown mode %d", mode);
    wgs_ctx *ctx = sc->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (score_sums_enqueue(sc, mode)) return 1;
    HIP_TRY(hipMemcpyAsync(out, sc->d_out, sizeof(double) * sc->cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->assign_ms_pending = true;
    sc->have_prefix = (mode == WGS_MODE_EXACT);
    return 0;
}

/* Test hook (include/wgsassign_hip_debug.h): the plan of the last wgs_score_sums, as eight numbers. */
int wgs_debug_score_plan(wgs_score *sc, int32_t info[8])
{
    WGS_REQUIRE(sc && info, "null argument");
    const ScorePlan &p = sc->plan;
    const int32_t v[8] = {p.codes ? 1 : 0, p.kb, p.np, p.chain_kb, p.chain_np, p.score_batch, p.elem_bytes, p.parts};
    std::copy(v, v + 8, info);
    return 0;
}

/* Test hook (include/wgsassign_hip_debug.h): the sums of the last wgs_score_sums per CHUNK of 8192 sites (two blocks; the addends of
 * np.sum's running total, what wgs_score_total_from folds): out[c * cells + i * K + k], ceil(nblocks / 2) x cells float64.  Lets a
 * test hold a full-size sweep to the oracle at any subset of the chunks: every float64 partial sum inside a chunk is exact. */
int wgs_debug_score_chunks(wgs_score *sc, double *out, int64_t *nchunks)
{
    WGS_REQUIRE(sc && nchunks, "null argument");
    WGS_REQUIRE(sc->d_chunks, "wgs_debug_score_chunks needs wgs_score_sums first");
    *nchunks = (sc->nblocks + 1) / 2;
    if (!out) return 0;
    wgs_ctx *ctx = sc->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out, sc->d_chunks, sizeof(double) * (size_t)*nchunks * sc->cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

/* Test hooks (include/wgsassign_hip_debug.h): the three kernels that add float64 block sums, each launched once on arrays made up
 * by the caller -- uploaded, one launch_* of the product path, downloaded.  `in` (n_in doubles, may be NULL) goes to the front of a
 * device buffer of n_all doubles, which *d receives; the rest of it is written by the kernel before it is read. */
static int debug_sums_upload(wgs_ctx *ctx, const double *in, size_t n_in, size_t n_all, double **d)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(wgs_malloc(d, sizeof(double) * std::max<size_t>(n_all, 1)));
    if (in && n_in && hipMemcpyAsync(*d, in, sizeof(double) * n_in, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        (void)hipFree(*d);
        wgs_set_error("block sums: upload failed");
        return 1;
    }
    return 0;
}

static int debug_sums_finish(wgs_ctx *ctx, double *d, int rc)
{
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        wgs_set_error("block sums: device operation failed");
        rc = 1;
    }
    (void)hipFree(d);
    return rc;
}

int wgs_debug_block_prefix(wgs_ctx *ctx, double *S, int32_t nblocks, int64_t cells, int keep_prefix, double *out, double *chunks)
{
    WGS_REQUIRE(ctx && out && nblocks >= 0 && cells > 0 && (S || nblocks == 0), "bad argument");
    const size_t nS = (size_t)nblocks * cells, nC = (size_t)((nblocks + 1) / 2) * cells;
    double *d = nullptr;                                   // S | out | chunks
    if (debug_sums_upload(ctx, S, nS, nS + cells + nC, &d)) return 1;
    int rc = launch_block_prefix(ctx, d, nblocks, cells, d + nS, keep_prefix, chunks ? d + nS + cells : nullptr);
    if (!rc && ((nS && hipMemcpyAsync(S, d, sizeof(double) * nS, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
                hipMemcpyAsync(out, d + nS, sizeof(double) * cells, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                (chunks && nC && hipMemcpyAsync(chunks, d + nS + cells, sizeof(double) * nC, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))) {
        wgs_set_error("block prefix: download failed");
        rc = 1;
    }
    return debug_sums_finish(ctx, d, rc);
}

int wgs_debug_chunk_total(wgs_ctx *ctx, const double *chunks, int32_t nchunks, int64_t cells, const double *carry, double *out)
{
    WGS_REQUIRE(ctx && out && nchunks >= 0 && cells > 0 && (chunks || nchunks == 0), "bad argument");
    const size_t nC = (size_t)nchunks * cells;
    double *d = nullptr;                                   // chunks | out | carry
    if (debug_sums_upload(ctx, chunks, nC, nC + 2 * cells, &d)) return 1;
    int rc = 0;
    if (carry && hipMemcpyAsync(d + nC + cells, carry, sizeof(double) * cells, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        wgs_set_error("chunk total: upload failed");
        rc = 1;
    }
    if (!rc) rc = launch_chunk_total(ctx, d, nchunks, cells, carry ? d + nC + cells : nullptr, d + nC);
    if (!rc && hipMemcpyAsync(out, d + nC, sizeof(double) * cells, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
        wgs_set_error("chunk total: download failed");
        rc = 1;
    }
    return debug_sums_finish(ctx, d, rc);
}

int wgs_debug_combine_parts(wgs_ctx *ctx, const double *Sp, int64_t total, int32_t parts, double *S)
{
    WGS_REQUIRE(ctx && Sp && S && total > 0 && parts >= 1, "bad argument");
    const size_t nP = (size_t)total * parts;
    double *d = nullptr;                                   // Sp | S
    if (debug_sums_upload(ctx, Sp, nP, nP + total, &d)) return 1;
    int rc = launch_combine_parts(ctx, d, d + nP, total, parts);
    if (!rc && hipMemcpyAsync(S, d + nP, sizeof(double) * total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
        wgs_set_error("combine parts: download failed");
        rc = 1;
    }
    return debug_sums_finish(ctx, d, rc);
}

/* The same sums continued from the SNP shards before this one: out[i*K + k] = (((carry_in + C0) + C1) + ...) over this
 * shard's 8192-site chunk sums C (kept by wgs_score_sums), i.e. np.sum(vec, dtype=float) of glassy.py:38 carried on in
 * NumPy's own order when every shard starts at a multiple of 8192 sites (comm.shard_range sees to that).  carry_in (host,
 * n*K doubles, NULL = zeros) is the value returned for the preceding shard; needs wgs_score_sums first. */
int wgs_score_total_from(wgs_score *sc, const double *carry_in, double *out)
{
    WGS_REQUIRE(sc && out, "null argument");
    WGS_REQUIRE(sc->d_chunks, "wgs_score_total_from needs wgs_score_sums first");
    wgs_ctx *ctx = sc->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(grow_once(sc, &sc->d_start, sizeof(double) * sc->cells));
    if (carry_in) HIP_TRY(hipMemcpyAsync(sc->d_start, carry_in, sizeof(double) * sc->cells, hipMemcpyHostToDevice, ctx->stream));
    if (score_total_enqueue(sc, carry_in ? sc->d_start : nullptr, sc->d_out)) return 1;
    HIP_TRY(hipMemcpyAsync(out, sc->d_out, sizeof(double) * sc->cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

/* The n x K totals over ALL SNP shards in NumPy's order, one call: np.sum's running float64 total is relayed from shard to shard
 * (common.h: wgs_relay) -- rank r continues it over its chunk sums (chunk_total_kernel) from what rank r - 1 left.
 * totals_out (host, n*K) receives the totals on every rank; before_out (host, n*K, may be NULL) the total over the shards
 * BEFORE this one (what wgs_score_chains_prepare wants as `start`).  comm == NULL or one rank: the local sums.
 * Needs wgs_score_sums first. */
int wgs_score_totals_all(wgs_score *sc, wgs_comm *comm, double *totals_out, double *before_out)
{
    WGS_REQUIRE(sc && totals_out, "null argument");
    WGS_REQUIRE(sc->d_chunks, "wgs_score_totals_all needs wgs_score_sums first");
    wgs_ctx *ctx = sc->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * sc->cells;
    HIP_TRY(grow_once(sc, &sc->d_start, bytes));
    HIP_TRY(grow_once(sc, &sc->d_run, wgs_relay_bytes(bytes)));
    HIP_TRY(hipMemsetAsync(sc->d_start, 0, bytes, ctx->stream));
    const int32_t generation = comm ? wgs_comm_next_generation(comm) : 0;
    if (wgs_relay(
            comm, sc->d_run, bytes,
            [&](int r) { return wgs_coll_tag{WGS_OP_SCORE_TOTALS, generation, r, (int32_t)(sc->row_hi - sc->row_lo), r, 0}; },
            [&](bool continued) -> int {
                if (continued) HIP_TRY(hipMemcpyAsync(sc->d_start, sc->d_run, bytes, hipMemcpyDeviceToDevice, ctx->stream));   // what precedes this shard
                return launch_chunk_total(ctx, sc->d_chunks, (sc->nblocks + 1) / 2, sc->cells, continued ? sc->d_start : nullptr, sc->d_run);
            }))
        return 1;
    HIP_TRY(hipMemcpyAsync(totals_out, sc->d_run, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (before_out) HIP_TRY(hipMemcpyAsync(before_out, sc->d_start, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return wgs_comm_check(comm);
}

/* ---- windowed scoring: one GPU walks the sites of a file window by window.  What the relay above does
 * across ranks -- np.sum's running float64 total continued from one site range to the next over the range's 8192-site chunk sums --
 * happens here in time: the total stays in device memory between the pushes (streams.h: RunningPair) and crosses to the host once,
 * in wgs_score_stream_finish. */
struct wgs_score_stream : StreamCursor {
    int64_t n = 0, cells = 0;
    int32_t K = 0;
    RunningPair<double> run;          // the n x K totals over the sites pushed so far
};

void wgs_score_stream_destroy(wgs_score_stream *st)
{
    if (!stream_retire(st)) return;
    st->run.release();
    delete st;
}

int wgs_score_stream_create(wgs_ctx *ctx, int64_t n, int32_t K, int64_t m_total, wgs_score_stream **out)
{
    WGS_REQUIRE(ctx && out, "null argument");
    WGS_REQUIRE(n > 0 && K > 0 && m_total > 0, "a score stream needs individuals, populations and sites (%lld x %d over %lld sites)",
                (long long)n, K, (long long)m_total);
    HIP_TRY(hipSetDevice(ctx->device));
    wgs_score_stream *st = stream_new<wgs_score_stream>(ctx, m_total, WGS_LIVE_SCORE_STREAM);
    auto guard = on_failure([&] { wgs_score_stream_destroy(st); });
    st->n = n;
    st->K = K;
    st->cells = n * (int64_t)K;
    HIP_TRY(st->run.allocate((size_t)st->cells));
    guard.dismiss();
    *out = st;
    return 0;
}

/* One window, under the window rule (stream_checks.h): a window that breaks it, or has another n or K, is refused before a kernel is
 * launched.  The window is swept by the path wgs_score_sums takes; its chunk sums are folded onto the running total by the code behind
 * wgs_score_total_from.  Returns when the device is done with the window -- its matrix and frequencies may be refilled -- but reads
 * nothing back.  wgs_assign_last_ms: this window's sweep. */
int wgs_score_stream_push(wgs_score_stream *st, wgs_beagle *window, wgs_afset *window_af, int mode)
{
    WGS_REQUIRE(st && window && window_af, "null argument");
    WGS_REQUIRE(mode == WGS_MODE_EXACT || mode == WGS_MODE_FAST, "unknown mode %d", mode);
    WGS_REQUIRE(window->ctx == st->ctx && window_af->ctx == st->ctx, "the window belongs to another context than the score stream");
    STREAM_TRY(score_stream_shape_refusal(window->n, window_af->K, window_af->m, window->m, st->n, st->K, why, sizeof why) ||
               stream_window_refusal("score stream", window->site0, window->m, st->pushed, st->m_total, WGS_WINDOW_ALIGN, why, sizeof why));
    wgs_ctx *ctx = st->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    wgs_score *sc = nullptr;
    auto guard = on_failure([&] { wgs_score_destroy(sc); });
    if (int rc = wgs_score_create(window, window_af, nullptr, 0, (int32_t)window->n, &sc)) return rc;
    if (score_sums_enqueue(sc, mode)) return 1;
    if (score_total_enqueue(sc, st->run.before(st->pushed > 0), st->run.next())) return 1;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    wgs_score_destroy(sc);
    ctx->assign_ms_pending = true;
    st->run.flip();
    st->pushed += window->m;
    return 0;
}

int wgs_score_stream_finish(wgs_score_stream *st, double *out_nK)
{
    WGS_REQUIRE(st && out_nK, "null argument");
    STREAM_TRY(stream_all_pushed_refusal(st->pushed, st->m_total, why, sizeof why));
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(hipMemcpyAsync(out_nK, st->run.current(), sizeof(double) * (size_t)st->cells, hipMemcpyDeviceToHost, st->ctx->stream));
    HIP_TRY(hipStreamSynchronize(st->ctx->stream));
    return 0;
}

/* Block functions of the exact partition chains (utils.py:147-149) for P partitions; needs the block
 * sums of wgs_score_sums(WGS_MODE_EXACT).  start (host, n*K doubles, may be NULL) = the float64 sums over
 * the SNP shards that precede this one (its partitions are predicted to hold equal shares).  rc 2 when P is
 * too large for the block-parallel kernel (use wgs_assign_parts_exact's literal chains then). */
// The block functions of wgs_score_chains_prepare, enqueued: `start` (n*K float64, may be NULL) is copied from the host or from the device
// (start_on_device: a running total that never left it, wgs_loo_stream_push).  The caller waits for the stream before `start` changes.
static int chains_prepare_enqueue(wgs_score *sc, int32_t P, const double *start, bool start_on_device)
{
    wgs_ctx *ctx = sc->b->ctx;
    const size_t chains = (size_t)sc->cells * P;
    if (sc->P != P) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (void *p : {(void *)sc->d_cand, (void *)sc->d_carry, (void *)sc->d_parts})
            if (p) wgs_pool_free(ctx, p);
        sc->d_cand = nullptr;
        sc->d_carry = sc->d_parts = nullptr;
        sc->P = 0;
        if (wgs_pool_malloc(ctx, &sc->d_cand, sizeof(uint32_t) * chains * sc->nblocks) != hipSuccess) {
            wgs_set_error("hipMalloc of %zu bytes for the partition-chain block functions failed", sizeof(uint32_t) * chains * sc->nblocks);
            return 1;
        }
        HIP_TRY(wgs_pool_malloc(ctx, &sc->d_carry, sizeof(float) * chains));
        HIP_TRY(wgs_pool_malloc(ctx, &sc->d_parts, wgs_relay_bytes(sizeof(float) * chains)));
        HIP_TRY(grow_once(sc, &sc->d_nserial, sizeof(int32_t)));
        HIP_TRY(grow_once(sc, &sc->d_start, sizeof(double) * sc->cells));
        sc->P = P;
    }
    HIP_TRY(hipMemsetAsync(sc->d_cand, 0, sizeof(uint32_t) * chains * sc->nblocks, ctx->stream));
    if (start)
        HIP_TRY(hipMemcpyAsync(sc->d_start, start, sizeof(double) * sc->cells, start_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               ctx->stream));
    ScoreArgs A = score_args(sc, 1);
    A.P = P;
    int g = 64, r = P;                       // gcd(64, P)
    while (r) {
        const int t = g % r;
        g = r;
        r = t;
    }
    A.period = P / g;
    A.start = start ? sc->d_start : nullptr;
    A.cand = sc->d_cand;
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    if (launch_chain_cand(ctx, A, sc->plan.chain_kb, sc->plan.chain_np)) return 1;
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    return 0;
}

int wgs_score_chains_prepare(wgs_score *sc, int32_t P, const double *start)
{
    WGS_REQUIRE(sc, "null argument");
    WGS_REQUIRE(P >= 1, "partition count must be >= 1");
    WGS_REQUIRE(sc->have_prefix, "wgs_score_chains_prepare needs wgs_score_sums(WGS_MODE_EXACT) first");
    WGS_REQUIRE(chains_block_parallel(sc->plan, sc->cells, P), "too many partitions (%d) for the block-parallel chains", P);
    wgs_ctx *ctx = sc->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (chains_prepare_enqueue(sc, P, start, false)) return 1;
    HIP_TRY(hipStreamSynchronize(ctx->stream));       // `start` (host) has been consumed
    ctx->assign_ms_pending = true;
    return 0;
}

/* Walk the chains of this shard: carry_in (host float32 [n*P*K], NULL = zeros) is the running value after
 * the preceding shards, parts_out (host float32 [n*P*K], index (i*P + p)*K + k) the value after this one;
 * rows of individuals outside the scored range are 0. */
static int chains_walk_enqueue(wgs_score *sc, bool with_carry)
{
    wgs_ctx *ctx = sc->b->ctx;
    const size_t chains = (size_t)sc->cells * sc->P;
    HIP_TRY(hipMemsetAsync(sc->d_parts, 0, sizeof(float) * chains, ctx->stream));
    HIP_TRY(hipMemsetAsync(sc->d_nserial, 0, sizeof(int32_t), ctx->stream));
    WalkArgs W;
    W.cand = sc->d_cand;
    W.carry = with_carry ? sc->d_carry : nullptr;
    W.parts = sc->d_parts;
    W.group_of = sc->b->d_group_of;
    W.col_of = sc->b->d_col_of;
    W.npairs = sc->b->d_npairs;
    W.base = sc->b->d_base;
    W.colptr = sc->d_colptr;
    W.acol = sc->d_acol;
    W.m = sc->b->m;
    W.site0 = sc->b->site0;
    W.n = (int32_t)sc->n;
    W.K = sc->K;
    W.P = sc->P;
    W.nblocks = sc->nblocks;
    W.row_lo = sc->row_lo;
    W.row_hi = sc->row_hi;
    W.n_serial = sc->d_nserial;
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    if (launch_chain_walk(ctx, W)) return 1;
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    return 0;
}

int wgs_score_chains_walk(wgs_score *sc, const float *carry_in, float *parts_out)
{
    WGS_REQUIRE(sc && parts_out, "null argument");
    WGS_REQUIRE(sc->P >= 1 && sc->d_cand, "wgs_score_chains_walk needs wgs_score_chains_prepare first");
    wgs_ctx *ctx = sc->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t chains = (size_t)sc->cells * sc->P;
    if (carry_in) HIP_TRY(hipMemcpyAsync(sc->d_carry, carry_in, sizeof(float) * chains, hipMemcpyHostToDevice, ctx->stream));
    if (chains_walk_enqueue(sc, carry_in != nullptr)) return 1;
    HIP_TRY(hipMemcpyAsync(parts_out, sc->d_parts, sizeof(float) * chains, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&sc->last_serial_blocks, sc->d_nserial, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->assign_ms_pending = true;
    return 0;
}

/* The chains of ALL SNP shards, one call: the float32 values are relayed from shard to shard (common.h: wgs_relay), rank r walking
 * its blocks on from them; parts_out (host) receives the values after the last shard on every rank.  Every rank has prepared its
 * block functions before (in parallel). */
int wgs_score_chains_walk_all(wgs_score *sc, wgs_comm *comm, float *parts_out)
{
    WGS_REQUIRE(sc && parts_out, "null argument");
    WGS_REQUIRE(sc->P >= 1 && sc->d_cand, "wgs_score_chains_walk_all needs wgs_score_chains_prepare first");
    wgs_ctx *ctx = sc->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(float) * (size_t)sc->cells * sc->P;
    const int32_t generation = comm ? wgs_comm_next_generation(comm) : 0;
    if (wgs_relay(
            comm, sc->d_parts, bytes, [&](int r) { return wgs_coll_tag{WGS_OP_PART_CHAINS, generation, r, sc->P, r, 0}; },
            [&](bool continued) -> int {
                if (continued) HIP_TRY(hipMemcpyAsync(sc->d_carry, sc->d_parts, bytes, hipMemcpyDeviceToDevice, ctx->stream));
                if (chains_walk_enqueue(sc, continued)) return 1;
                HIP_TRY(hipMemcpyAsync(&sc->last_serial_blocks, sc->d_nserial, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
                return 0;
            }))
        return 1;
    HIP_TRY(hipMemcpyAsync(parts_out, sc->d_parts, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->assign_ms_pending = true;
    return wgs_comm_check(comm);
}

/* Test hook: blocks that took the literal serial loop in the last wgs_score_chains_walk, and the number of
 * (chain, block) pairs walked. */
int wgs_score_last_serial_blocks(wgs_score *sc, int64_t *total_blocks)
{
    if (!sc) return -1;
    if (total_blocks) *total_blocks = (int64_t)(sc->row_hi - sc->row_lo) * sc->K * sc->P * sc->nblocks;
    return sc->last_serial_blocks;
}

int wgs_assign(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int mode, double *out)
{
    WGS_REQUIRE(b && a && out, "null argument");
    WGS_REQUIRE(a->m == b->m, "allele frequencies cover %lld SNPs, the Beagle shard %lld", (long long)a->m, (long long)b->m);
    wgs_ctx *ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t cells = (size_t)b->n * a->K;
    ctx->last_assign_ms = 0.0f;
    ctx->assign_ms_pending = false;
    std::vector<double> h(cells);
    // one launch over all population slabs, reproducible sums (wgs_score_sums)
    wgs_score *sc = nullptr;
    int rc = wgs_score_create(b, a, colptr, 0, (int32_t)b->n, &sc);
    if (!rc) rc = wgs_score_sums(sc, mode, h.data());
    wgs_score_destroy(sc);
    if (rc) return rc;
    for (size_t c = 0; c < cells; ++c) out[c] += h[c];
    return 0;
}

/* Cross-check only (tests, tools/check_fast_mode.py): FLOAT64 partition sums (labels = global site index % P) from the
 * round-1 kernel that maps lanes to pairs of individuals and combines tile ranges with float64 atomics -- within
 * ~1e-5 of the reference's serial float32 partition sums and not reproducible run to run.  The product path is
 * wgs_assign_parts_exact / wgs_score_chains_*.  out [n*K] and parts [n*P*K] are accumulated into. */
int wgs_debug_assign_parts_f64(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int32_t P, int mode, double *out, double *parts)
{
    WGS_REQUIRE(b && a && out && parts, "null argument");
    WGS_REQUIRE(a->m == b->m, "allele frequencies cover %lld SNPs, the Beagle shard %lld", (long long)a->m, (long long)b->m);
    WGS_REQUIRE(P >= 1, "partition count must be >= 1");
    wgs_ctx *ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const int K = a->K;
    const int64_t n = b->n;
    const size_t cells = (size_t)n * P * K;
    ctx->last_assign_ms = 0.0f;
    ctx->assign_ms_pending = false;
    std::vector<double> h(cells);
    // one grow-only workspace: [cells doubles | K shared pointers | n*K per-individual pointers]
    const size_t off_acol = (sizeof(double) * cells + 255) & ~(size_t)255;
    const size_t off_colptr = (off_acol + sizeof(float *) * K + 255) & ~(size_t)255;
    const size_t total = off_colptr + (colptr ? sizeof(float *) * n * K : 0);
    void *ws = nullptr;
    if (wgs_ctx_workspace(ctx, total, &ws)) return 1;
    double *d_out = reinterpret_cast<double *>(ws);
    const float **d_acol = reinterpret_cast<const float **>(reinterpret_cast<char *>(ws) + off_acol);
    const float **d_colptr = colptr ? reinterpret_cast<const float **>(reinterpret_cast<char *>(ws) + off_colptr) : nullptr;
    std::vector<const float *> acol;
    HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(double) * cells, ctx->stream));
    HIP_TRY(upload_columns(a, acol, d_acol, ctx->stream));
    if (colptr) HIP_TRY(hipMemcpyAsync(d_colptr, colptr, sizeof(float *) * n * K, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));      // acol has been consumed
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    const int kb = score_plan_shape(K, colptr != nullptr).chain_kb;
    int rc = 0;
    for_scored_slabs(b, 0, n, [&](int, const Slab &s, int, int) {
        const AssignArgs args = {s.base, s.d_members, d_colptr, d_acol, d_out, b->m, b->site0, s.npairs, s.ncols, K, P, 0};
        if (!rc) rc = launch_assign(ctx, args, kb, mode);
    });
    if (rc) return 1;
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h.data(), d_out, sizeof(double) * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->assign_ms_pending = true;
    for (size_t c = 0; c < cells; ++c) parts[c] += h[c];
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int p = 0; p < P; ++p) t += h[((size_t)i * P + p) * K + k];
            out[(size_t)i * K + k] += t;
        }
    return 0;
}

/* ---- glassy.loo -- glassy.py:47-112 -- in one call ---------------------------------------------------
 * For every individual i (file order): re-fit its population without it (emMAF.py:15-27 via wgs_em_fit, all
 * individuals of a batch at once), clamp with n_pop - 1 (glassy.py:80-85), OVERWRITE the population's column
 * (glassy.py:87-89: never restored, so every other column is the re-fit of the most recent earlier individual
 * of that population), score i against all K columns (float64 sums of the float32 per-site values,
 * glassy.py:92-105) and, if asked, accumulate the serial float32 partition sums (utils.py:147-149).
 *   b       the matrix the frequencies are estimated from (population slabs = columns of `a`);
 *   scored  the matrix that is scored (NULL = b; the downsampled matrix of --loo_downsampled_beagle);
 *   a       in: the full-population estimates; out: each population's LAST re-fit (glassy.py:89);
 *   batch   re-fits per EM batch, 0 = what fits the free device memory (agreed across ranks);
 *   ll_out  host float64 [n*K] (overwritten); parts_out host float32 [n*P*K] or NULL; iters_out [n]. */
static double g_loo_stats[7];      // of the last wgs_loo of this process: see wgs_loo_stats

static double wall_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

/* Phases of the last wgs_loo: stats[0..5] = seconds in the EM re-fits (wgs_em_fit incl. its exact chains), in the
 * scoring sweeps (+ their cross-rank totals), in the exact partition chains; EM sweep kernel ms; EM batches; chain
 * resolutions of the re-fits; EM iterations enqueued (= all-reduces of the convergence sums across SNP shards). */
int wgs_loo_stats(double *stats)
{
    WGS_REQUIRE(stats, "null argument");
    for (int i = 0; i < 7; ++i) stats[i] = g_loo_stats[i];
    return 0;
}

int wgs_loo(wgs_beagle *b, wgs_beagle *scored, wgs_afset *a, int32_t max_iter, double tole, int64_t m_total, wgs_comm *comm,
            int32_t P, int32_t batch, int em_mode, int score_mode, double *ll_out, float *parts_out, int32_t *iters_out)
{
    for (double &x : g_loo_stats) x = 0.0;
    WGS_REQUIRE(b && a && ll_out && iters_out, "null argument");
    if (!scored) scored = b;
    WGS_REQUIRE(scored->n == b->n && scored->m == b->m && scored->n_groups == b->n_groups && scored->group_of == b->group_of,
                "the scored matrix must have the shape and population slabs of the fitted one");
    WGS_REQUIRE(a->m == b->m && a->K == b->n_groups, "allele frequencies (%lld x %d) do not match the population slabs (%lld x %d)",
                (long long)a->m, a->K, (long long)b->m, b->n_groups);
    WGS_REQUIRE(P >= 1, "partition count must be >= 1");
    wgs_ctx *ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t n = b->n;
    const int K = a->K;
    const size_t cells = (size_t)n * K;
    int world = 1, rank = 0;
    if (comm) wgs_comm_rank(comm, &rank, &world);
    if (batch <= 0) {      // 2 float32 vectors + per-tile partial sums per fit: ~8.2 bytes per SNP and fit
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const double per_fit = (double)b->m * 8.2 + 4096.0;
        batch = (int32_t)std::max<double>(1.0, std::min<double>((double)n, 0.8 * (double)free_b / per_fit));
    }
    batch = (int32_t)std::min<int64_t>(n, batch);
    if (world > 1) {       // every rank must run the same batches: the minimum over ranks
        std::vector<double> slots(world, 0.0);
        slots[rank] = (double)batch;
        const wgs_coll_tag tag = {WGS_OP_LOO_BATCH, wgs_comm_next_generation(comm), 0, (int32_t)n, P, batch};
        if (wgs_comm_allreduce_host_tagged(comm, slots.data(), world, &tag, nullptr)) return 1;
        batch = (int32_t)*std::min_element(slots.begin(), slots.end());
    }
    std::vector<int32_t> counts(K, 0);
    for (int64_t i = 0; i < n; ++i) ++counts[b->group_of[i]];
    std::fill(ll_out, ll_out + cells, 0.0);
    if (parts_out) std::fill(parts_out, parts_out + cells * P, 0.0f);
    std::vector<const float *> colptr(cells), cur(K);
    std::vector<double> sums(cells), start(cells);
    std::vector<float> parts;
    for (int64_t i0 = 0; i0 < n; i0 += batch) {
        const int64_t i1 = std::min<int64_t>(n, i0 + batch);
        const int nb = (int)(i1 - i0);
        std::vector<int32_t> grp(nb), skip(nb);
        for (int x = 0; x < nb; ++x) grp[x] = b->group_of[i0 + x], skip[x] = (int32_t)(i0 + x);
        wgs_em *em = nullptr;
        wgs_score *sc = nullptr;
        auto guard = on_failure([&] { wgs_score_destroy(sc); wgs_em_destroy(em); });
        double t_phase = wall_s();
        int rc = wgs_em_create(b, nb, grp.data(), skip.data(), em_mode, &em);
        if (rc) return rc;
        if ((rc = wgs_em_fit(em, max_iter, tole, m_total, comm, 0.0, iters_out + i0))) return rc;
        {
            int32_t it = 0, cb = 0;
            double sec = 0.0, sweep_ms = 0.0;
            wgs_em_fit_stats(em, &it, &cb, &sec, &sweep_ms);
            if (sweep_ms < 0) sweep_ms = 0.0;                // (not known while the codes' memory is being allocated)
            g_loo_stats[0] += wall_s() - t_phase;
            g_loo_stats[3] += sweep_ms;
            g_loo_stats[4] += 1.0;
            g_loo_stats[5] += cb;
            g_loo_stats[6] += it;
        }
        t_phase = wall_s();
        for (int x = 0; x < nb; ++x) {
            const int npop = counts[grp[x]] - 1;
            const double lo = 1.0 / (2.0 * (npop + 1));
            if ((rc = wgs_em_clamp(em, x, (float)lo, (float)(1.0 - lo)))) return rc;
        }
        // glassy.py:87-105: individual i's own re-fit, else the most recent earlier re-fit, else the column of `a`
        for (int k = 0; k < K; ++k) cur[k] = a->buf + (size_t)k * a->m;
        for (int64_t i = 0; i < n; ++i)
            for (int k = 0; k < K; ++k) colptr[(size_t)i * K + k] = cur[k];
        for (int64_t i = i0; i < i1; ++i) {
            cur[b->group_of[i]] = wgs_em_f_dev(em, (int32_t)(i - i0));
            for (int k = 0; k < K; ++k) colptr[(size_t)i * K + k] = cur[k];
        }
        if ((rc = wgs_score_create(scored, a, colptr.data(), (int32_t)i0, (int32_t)i1, &sc))) return rc;
        if ((rc = wgs_score_sums(sc, parts_out ? WGS_MODE_EXACT : score_mode, sums.data()))) return rc;
        if (world > 1) {
            // np.sum's running float64 total handed from shard to shard in SNP order on the stream (`world` broadcasts,
            // one readback); `start` = what precedes this shard, for the chain prediction
            if ((rc = wgs_score_totals_all(sc, comm, sums.data(), start.data()))) return rc;
        }
        for (size_t c = (size_t)i0 * K; c < (size_t)i1 * K; ++c) ll_out[c] = sums[c];
        g_loo_stats[1] += wall_s() - t_phase;
        t_phase = wall_s();
        if (parts_out) {
            if ((rc = wgs_score_chains_prepare(sc, P, world > 1 && rank > 0 ? start.data() : nullptr))) return rc;
            parts.assign(cells * P, 0.0f);
            // every rank has its block functions; the walks follow each other with the float32 carries (`world` broadcasts)
            if ((rc = wgs_score_chains_walk_all(sc, comm, parts.data()))) return rc;
            for (size_t c = (size_t)i0 * P * K; c < (size_t)i1 * P * K; ++c) parts_out[c] = parts[c];
            g_loo_stats[2] += wall_s() - t_phase;
        }
        // the last re-fit of each population in this batch becomes the current column
        std::vector<int32_t> last(K, -1);
        for (int x = 0; x < nb; ++x) last[grp[x]] = x;
        for (int k = 0; k < K; ++k)
            if (last[k] >= 0 && (rc = wgs_afset_set_column_from_em(a, k, em, last[k]))) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        guard.dismiss();
        wgs_score_destroy(sc);
        wgs_em_destroy(em);
    }
    return wgs_comm_check(comm);
}

static int parts_exact_literal(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int32_t P, const float *carry_in,
                               float *parts_out);

/* Exact partition sums: utils.partition_loglikes (utils.py:129-151) for every (individual,
 * population) -- serial float32 accumulation per partition in site order, continued from
 * carry_in (float32 [n*P*K], NULL = zeros: first shard) into parts_out (float32 [n*P*K]).
 * literal != 0 forces the one-lane-per-chain kernel (the cross-check of the block-parallel chains). */
int wgs_assign_parts_exact(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int32_t P, const float *carry_in,
                           float *parts_out)
{
    WGS_REQUIRE(b && a && parts_out, "null argument");
    WGS_REQUIRE(a->m == b->m, "allele frequencies cover %lld SNPs, the Beagle shard %lld", (long long)a->m, (long long)b->m);
    WGS_REQUIRE(P >= 1, "partition count must be >= 1");
    if (!chains_block_parallel(score_plan_shape(a->K, colptr != nullptr), b->n * (int64_t)a->K, P))
        return parts_exact_literal(b, a, colptr, P, carry_in, parts_out);
    const size_t cells = (size_t)b->n * a->K;
    std::vector<double> sums(cells), start;
    if (carry_in) {           // the preceding shards' float64 sums are not known here: their float32 chains stand in
        start.assign(cells, 0.0);
        for (int64_t i = 0; i < b->n; ++i)
            for (int p = 0; p < P; ++p)
                for (int k = 0; k < a->K; ++k) start[(size_t)i * a->K + k] += (double)carry_in[((size_t)i * P + p) * a->K + k];
    }
    wgs_score *sc = nullptr;
    int rc = wgs_score_create(b, a, colptr, 0, (int32_t)b->n, &sc);
    if (!rc) rc = wgs_score_sums(sc, WGS_MODE_EXACT, sums.data());
    if (!rc) rc = wgs_score_chains_prepare(sc, P, carry_in ? start.data() : nullptr);
    if (!rc) rc = wgs_score_chains_walk(sc, carry_in, parts_out);
    wgs_score_destroy(sc);
    return rc;
}

int wgs_debug_parts_exact_literal(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int32_t P, const float *carry_in,
                                  float *parts_out)
{
    WGS_REQUIRE(b && a && parts_out, "null argument");
    WGS_REQUIRE(a->m == b->m, "allele frequencies cover %lld SNPs, the Beagle shard %lld", (long long)a->m, (long long)b->m);
    WGS_REQUIRE(P >= 1, "partition count must be >= 1");
    return parts_exact_literal(b, a, colptr, P, carry_in, parts_out);
}

static int parts_exact_literal(wgs_beagle *b, wgs_afset *a, const float *const *colptr, int32_t P, const float *carry_in,
                               float *parts_out)
{
    wgs_ctx *ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const int K = a->K;
    const int64_t n = b->n;
    const size_t cells = (size_t)n * P * K;
    const size_t off_carry = (sizeof(float) * cells + 255) & ~(size_t)255;
    const size_t off_acol = (off_carry + sizeof(float) * cells + 255) & ~(size_t)255;
    const size_t off_slabs = (off_acol + sizeof(float *) * K + 255) & ~(size_t)255;
    const size_t off_colptr = (off_slabs + sizeof(PartsSlab) * b->n_groups + 255) & ~(size_t)255;
    const size_t total = off_colptr + (colptr ? sizeof(float *) * n * K : 0);
    void *ws = nullptr;
    if (wgs_ctx_workspace(ctx, total, &ws)) return 1;
    char *base = reinterpret_cast<char *>(ws);
    float *d_parts = reinterpret_cast<float *>(base);
    float *d_carry = carry_in ? reinterpret_cast<float *>(base + off_carry) : nullptr;
    PartsSlab *d_slabs = reinterpret_cast<PartsSlab *>(base + off_slabs);
    const float **d_acol = reinterpret_cast<const float **>(base + off_acol);
    const float **d_colptr = colptr ? reinterpret_cast<const float **>(base + off_colptr) : nullptr;
    HIP_TRY(hipMemsetAsync(d_parts, 0, sizeof(float) * cells, ctx->stream));
    if (carry_in) HIP_TRY(hipMemcpyAsync(d_carry, carry_in, sizeof(float) * cells, hipMemcpyHostToDevice, ctx->stream));
    std::vector<const float *> acol;
    HIP_TRY(upload_columns(a, acol, d_acol, ctx->stream));
    if (colptr) HIP_TRY(hipMemcpyAsync(d_colptr, colptr, sizeof(float *) * n * K, hipMemcpyHostToDevice, ctx->stream));
    std::vector<PartsSlab> slabs;
    int blocks = 0;
    for_scored_slabs(b, 0, n, [&](int, const Slab &s, int, int) {
        slabs.push_back({s.base, s.d_members, s.npairs, s.ncols, blocks});
        blocks += (s.ncols + 63) / 64;
    });
    HIP_TRY(hipMemcpyAsync(d_slabs, slabs.data(), sizeof(PartsSlab) * slabs.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    AssignArgs args = {};          // (the fields common to all slabs)
    args.colptr = d_colptr;
    args.acol = d_acol;
    args.m = b->m;
    args.site0 = b->site0;
    args.K = K;
    args.P = P;
    if (launch_parts_exact(ctx, args, d_slabs, (int)slabs.size(), blocks, d_carry, d_parts)) return 1;
    HIP_TRY(hipMemcpyAsync(parts_out, d_parts, sizeof(float) * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

/* ---- the leave-one-out run in site windows ("leave-one-out in windows").  What wgs_loo does on one resident
 * matrix after its re-fits -- the column table of glassy.py:87-105, the per-individual sweep, np.sum's float64 totals, the serial float32
 * partition sums -- happens here window by window, on the window's batch of n re-fits that the last round of a windowed fit left
 * clamped on the device (wgs_em_stream_push_keep).  Between the pushes the stream keeps the n x K running totals (as wgs_score_stream
 * does) and the n x P x K float32 partition carries on the device; a window continues both exactly as the
 * SNP shard of a rank > 0 continues them in wgs_loo: the totals over its 8192-site chunk sums, the chains from the carries with the
 * totals before the window as `start`.  wgs_loo_stream_finish is the one read-back. */
struct wgs_loo_stream : StreamCursor {
    int64_t n = 0, cells = 0;
    int32_t K = 0, P = 0;               // P == 0: no partition sums
    RunningPair<double> run;            // the n x K totals over the sites pushed so far
    float *d_carry = nullptr;           // [n * P * K] the partition sums over the sites pushed so far
    std::vector<float> h_carry, h_parts;    // the literal chains (P too large for the block-parallel ones) take and give host arrays
};

void wgs_loo_stream_destroy(wgs_loo_stream *st)
{
    if (!stream_retire(st)) return;
    st->run.release();
    if (st->d_carry) (void)hipFree(st->d_carry);
    delete st;
}

int wgs_loo_stream_create(wgs_ctx *ctx, int64_t n, int32_t K, int64_t m_total, int32_t P, wgs_loo_stream **out)
{
    WGS_REQUIRE(ctx && out, "null argument");
    WGS_REQUIRE(n > 0 && K > 0 && m_total > 0, "a leave-one-out stream needs individuals, populations and sites (%lld x %d over %lld sites)",
                (long long)n, K, (long long)m_total);
    WGS_REQUIRE(P >= 0, "partition count must be >= 0 (0: no partition sums)");
    WGS_REQUIRE(n * (int64_t)K * std::max(1, P) < (1ll << 31), "%lld individuals x %d populations x %d partitions are too many for one stream",
                (long long)n, K, P);
    HIP_TRY(hipSetDevice(ctx->device));
    wgs_loo_stream *st = stream_new<wgs_loo_stream>(ctx, m_total, WGS_LIVE_LOO_STREAM);
    auto guard = on_failure([&] { wgs_loo_stream_destroy(st); });
    st->n = n;
    st->K = K;
    st->P = P;
    st->cells = n * (int64_t)K;
    HIP_TRY(st->run.allocate((size_t)st->cells));
    if (P > 0) HIP_TRY(wgs_malloc(&st->d_carry, sizeof(float) * (size_t)st->cells * P));
    guard.dismiss();
    *out = st;
    return 0;
}

/* One window: `window_em` is the batch of n re-fits made from the window's matrix (fit i: the population of individual i without i),
 * every fit at its stopping iteration and clamped; window_af the window's rows of the full-population frequencies.  Individual i is
 * scored against its own re-fit and, for every other population, the re-fit of the most recent earlier individual of that population,
 * else the column of window_af (glassy.py:87-105).  mode: the arithmetic of the sweep when no partition sums are kept (with them it is
 * exact).  A wrong first site, a misaligned or ragged middle window, an overrun, another n or K, a batch that is not the n re-fits:
 * rc 2 and a message, nothing launched.  Returns when the device is done with the window; nothing is read back. */
int wgs_loo_stream_push(wgs_loo_stream *st, wgs_em *window_em, wgs_afset *window_af, int mode)
{
    WGS_REQUIRE(st && window_em && window_af, "null argument");
    return wgs_loo_stream_push_scored(st, window_em, window_em->b, window_af, mode);
}

/* wgs_loo_stream_push with the matrix that is SCORED given apart from the one the re-fits were made from (--loo_downsampled_beagle in
 * site windows: `scored_window` is the downsampled file's window of the same kept sites; wgs_loo's `scored`).  The column table still
 * comes from window_em and window_af; the sweep, the chunk sums and the partition chains read scored_window.  A scored window of another
 * context, with another n, m, site0 or n_groups, or with another group_of than the fitted window's: rc 2 and a message, nothing
 * launched, the stream as it was.  scored_window == the matrix of window_em is wgs_loo_stream_push. */
int wgs_loo_stream_push_scored(wgs_loo_stream *st, wgs_em *window_em, wgs_beagle *scored_window, wgs_afset *window_af, int mode)
{
    WGS_REQUIRE(st && window_em && scored_window && window_af, "null argument");
    WGS_REQUIRE(mode == WGS_MODE_EXACT || mode == WGS_MODE_FAST, "unknown mode %d", mode);
    wgs_beagle *window = window_em->b;
    WGS_REQUIRE(window->ctx == st->ctx && window_af->ctx == st->ctx, "the window belongs to another context than the leave-one-out stream");
    WGS_REQUIRE(scored_window->ctx == st->ctx, "the scored window belongs to another context than the leave-one-out stream");
    STREAM_TRY(loo_stream_shape_refusal(window->n, window->n_groups, window_em->n_fits, window_af->K, window_af->m, window->m, st->n, st->K, why,
                                        sizeof why) ||
               loo_stream_fits_refusal(st->n, window_em->group.data(), window_em->skip_local.data(), window->group_of.data(), why, sizeof why) ||
               stream_window_refusal("leave-one-out stream", window->site0, window->m, st->pushed, st->m_total, WGS_WINDOW_ALIGN, why, sizeof why) ||
               (scored_window != window &&
                loo_stream_scored_refusal(scored_window->n, scored_window->m, scored_window->site0, scored_window->n_groups,
                                          scored_window->group_of.data(), window->n, window->m, window->site0, window->n_groups,
                                          window->group_of.data(), why, sizeof why)));
    wgs_ctx *ctx = st->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t n = st->n;
    const int K = st->K, P = st->P;
    const size_t cells = (size_t)st->cells;
    // glassy.py:87-105: individual i's own re-fit, else the most recent earlier re-fit, else the column of window_af
    std::vector<const float *> colptr(cells), cur(K);
    for (int k = 0; k < K; ++k) cur[k] = window_af->buf + (size_t)k * window_af->m;
    for (int64_t i = 0; i < n; ++i) {
        cur[window->group_of[i]] = wgs_em_f_dev(window_em, (int32_t)i);
        for (int k = 0; k < K; ++k) colptr[(size_t)i * K + k] = cur[k];
    }
    wgs_score *sc = nullptr;
    auto guard = on_failure([&] { wgs_score_destroy(sc); });
    if (int rc = wgs_score_create(scored_window, window_af, colptr.data(), 0, (int32_t)n, &sc)) return rc;
    if (score_sums_enqueue(sc, P > 0 ? WGS_MODE_EXACT : mode)) return 1;
    sc->have_prefix = P > 0;
    const double *before = st->run.before(st->pushed > 0);                  // the totals over the windows before this one
    if (score_total_enqueue(sc, before, st->run.next())) return 1;
    const size_t chains = cells * (size_t)std::max(1, P);
    if (P > 0 && P <= WGS_MAX_BLOCK_PARALLEL_PARTS && chains_block_parallel(sc->plan, sc->cells, P)) {
        if (chains_prepare_enqueue(sc, P, before, true)) return 1;
        if (before) HIP_TRY(hipMemcpyAsync(sc->d_carry, st->d_carry, sizeof(float) * chains, hipMemcpyDeviceToDevice, ctx->stream));
        if (chains_walk_enqueue(sc, before != nullptr)) return 1;
        HIP_TRY(hipMemcpyAsync(st->d_carry, sc->d_parts, sizeof(float) * chains, hipMemcpyDeviceToDevice, ctx->stream));
    } else if (P > 0) {
        // many short chains: the literal one-lane chains, which take the carry and give the sums as host arrays (n * P * K floats)
        st->h_parts.assign(chains, 0.0f);
        if (before) {
            st->h_carry.resize(chains);
            HIP_TRY(hipMemcpyAsync(st->h_carry.data(), st->d_carry, sizeof(float) * chains, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (int rc = parts_exact_literal(scored_window, window_af, colptr.data(), P, before ? st->h_carry.data() : nullptr, st->h_parts.data())) return rc;
        HIP_TRY(hipMemcpyAsync(st->d_carry, st->h_parts.data(), sizeof(float) * chains, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    wgs_score_destroy(sc);
    ctx->assign_ms_pending = true;
    st->run.flip();
    st->pushed += window->m;
    return 0;
}

/* The one read-back: ll_out (host, n*K float64, overwritten) the totals, parts_out (host, n*P*K float32, index (i*P + p)*K + k; NULL
 * when the stream keeps no partition sums) the partition sums.  rc 2 before all m_total sites were pushed. */
int wgs_loo_stream_finish(wgs_loo_stream *st, double *ll_out, float *parts_out)
{
    WGS_REQUIRE(st && ll_out, "null argument");
    STREAM_TRY(stream_all_pushed_refusal(st->pushed, st->m_total, why, sizeof why));
    WGS_REQUIRE(!parts_out || st->P > 0, "the leave-one-out stream keeps no partition sums");
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(hipMemcpyAsync(ll_out, st->run.current(), sizeof(double) * (size_t)st->cells, hipMemcpyDeviceToHost, st->ctx->stream));
    if (parts_out)
        HIP_TRY(hipMemcpyAsync(parts_out, st->d_carry, sizeof(float) * (size_t)st->cells * st->P, hipMemcpyDeviceToHost, st->ctx->stream));
    HIP_TRY(hipStreamSynchronize(st->ctx->stream));
    return 0;
}

}   // extern "C"
