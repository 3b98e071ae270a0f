// C ABI of the z-score options (include/wgsassign_hip.h, "z-scores"): depth table, depth-class sweep, kept-site sets, per-site
// statistic, and the leave-one-out fit whose convergence test runs over a site subset.  Kernels: zscore_kernels.hip.
#include <math.h>
#include <string.h>

#include "em_state.h"
#include "zscore.h"

// Device buffers of one call, released when it returns whichever way.
struct ZBufs {
    std::vector<void *> p;
    ~ZBufs() { for (void *q : p) (void)hipFree(q); }
    template <typename T>
    hipError_t get(T **out, size_t bytes)
    {
        const hipError_t e = wgs_malloc(out, bytes ? bytes : 1);
        if (e == hipSuccess) p.push_back(*out);
        return e;
    }
};

int zs_fill_inds(wgs_beagle *b, int32_t i0, int32_t count, std::vector<ZInd> &out)
{
    WGS_REQUIRE(i0 >= 0 && count > 0 && (int64_t)i0 + count <= b->n, "individuals [%d, %d) outside 0..%lld", i0, i0 + count, (long long)b->n);
    out.resize(count);
    for (int j = 0; j < count; ++j) {
        const Slab &s = b->slabs[b->group_of[i0 + j]];
        const int col = b->col_of[i0 + j];
        out[j] = ZInd{s.base, s.npairs, col >> 1, col & 1, i0 + j};
    }
    return 0;
}

extern "C" {

static int depth_create(wgs_ctx *ctx, wgs_beagle *b, int64_t m, int64_t n, wgs_depth **out)
{
    WGS_REQUIRE(m > 0 && m < (int64_t)1 << 31, "the depth table needs between 1 and 2^31 - 1 sites");
    WGS_REQUIRE(n > 0 && n < (int64_t)1 << 24, "the depth table needs between 1 and 2^24 - 1 individuals");
    HIP_TRY(hipSetDevice(ctx->device));
    wgs_depth *d = new wgs_depth();
    wgs_live_add(d, WGS_LIVE_DEPTH, b ? (void *)b : (void *)ctx);
    auto guard = on_failure([&] { wgs_depth_destroy(d); });
    d->b = b;
    d->ctx = ctx;
    d->m = m;
    d->n = n;
    d->mpad = wgs_ntiles(m) * 64;
    const size_t bytes = (size_t)n * d->mpad * sizeof(uchar2);
    if (wgs_malloc(&d->table, bytes) != hipSuccess) {
        wgs_set_error("hipMalloc of %zu bytes for the allele-depth table failed", bytes);
        return 1;
    }
    HIP_TRY(wgs_malloc(&d->d_bad, sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(d->table, 0, bytes, ctx->stream));
    HIP_TRY(hipMemsetAsync(d->d_bad, 0, sizeof(int32_t), ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    *out = d;
    return 0;
}

int wgs_depth_create(wgs_beagle *b, wgs_depth **out)
{
    WGS_REQUIRE(b && out, "null argument");
    return depth_create(b->ctx, b, b->m, b->n, out);
}

int wgs_depth_create_shape(wgs_ctx *ctx, int64_t m, int64_t n, wgs_depth **out)
{
    WGS_REQUIRE(ctx && out, "null argument");
    return depth_create(ctx, nullptr, m, n, out);
}

void wgs_depth_destroy(wgs_depth *d)
{
    if (!d || !wgs_live_remove(d)) return;
    wgs_live_destroy_children(d);             // kept-site sets made from this table go first
    (void)hipSetDevice(d->ctx->device);
    if (d->table) (void)hipFree(d->table);
    if (d->d_bad) (void)hipFree(d->d_bad);
    delete d;
}

int wgs_depth_upload_rows(wgs_depth *d, const int32_t *AD_rows, int64_t row0, int64_t nrows)
{
    WGS_REQUIRE(d && AD_rows, "null argument");
    const wgs_depth *b = d;                                  // (the table's own shape: it may have no matrix)
    WGS_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= b->m, "row range [%lld, %lld) outside 0..%lld", (long long)row0,
                (long long)(row0 + nrows), (long long)b->m);
    WGS_REQUIRE(nrows * b->n < (int64_t)1 << 38, "too many rows in one upload");
    if (nrows == 0) return 0;
    wgs_ctx *ctx = d->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    ZBufs bufs;
    int32_t *d_rows = nullptr;
    const size_t bytes = (size_t)nrows * 2 * b->n * sizeof(int32_t);
    HIP_TRY(bufs.get(&d_rows, bytes));
    HIP_TRY(hipMemcpyAsync(d_rows, AD_rows, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (launch_zdepth_scatter(ctx, d_rows, nrows, b->n, row0, d->mpad, d->table, d->d_bad)) return 1;
    int32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d->d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (bad) {
        HIP_TRY(hipMemset(d->d_bad, 0, sizeof(int32_t)));
        wgs_set_error("allele depths outside 0..255 do not fit the device table");
        return 2;
    }
    return 0;
}

int wgs_depth_download_rows(wgs_depth *d, int32_t *AD_rows, int64_t row0, int64_t nrows)
{
    WGS_REQUIRE(d && AD_rows, "null argument");
    WGS_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= d->m, "row range [%lld, %lld) outside 0..%lld", (long long)row0,
                (long long)(row0 + nrows), (long long)d->m);
    WGS_REQUIRE(nrows * d->n < (int64_t)1 << 38, "too many rows in one download");
    if (nrows == 0) return 0;
    wgs_ctx *ctx = d->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    ZBufs bufs;
    int32_t *d_rows = nullptr;
    const size_t bytes = (size_t)nrows * 2 * d->n * sizeof(int32_t);
    HIP_TRY(bufs.get(&d_rows, bytes));
    if (launch_zdepth_gather(ctx, d->table, nrows, d->n, row0, d->mpad, d_rows)) return 1;
    HIP_TRY(hipMemcpyAsync(AD_rows, d_rows, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int wgs_zscore_classes_sharded(wgs_depth *d, int32_t i0, int32_t count, wgs_comm *comm, int32_t *counts_out, float *sums_out,
                               int64_t *first_out, int32_t *over_out)
{
    WGS_REQUIRE(d && counts_out && sums_out && first_out && over_out, "null argument");
    WGS_REQUIRE(d->b, "the depth table was created without a matrix (wgs_depth_create_shape)");
    wgs_beagle *b = d->b;
    wgs_ctx *ctx = b->ctx;
    int world = 1, rank = 0;
    if (comm) wgs_comm_rank(comm, &rank, &world);
    std::vector<ZInd> inds;
    if (int rc = zs_fill_inds(b, i0, count, inds)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int32_t generation = comm ? wgs_comm_next_generation(comm) : 0;
    ZBufs bufs;
    ZInd *d_inds = nullptr;
    int32_t *cnt = nullptr, *first = nullptr, *over = nullptr;
    float *sums = nullptr;
    const size_t cells = (size_t)count * 256;
    HIP_TRY(bufs.get(&d_inds, sizeof(ZInd) * count));
    HIP_TRY(bufs.get(&cnt, sizeof(int32_t) * cells));
    HIP_TRY(bufs.get(&first, sizeof(int32_t) * cells));
    HIP_TRY(bufs.get(&sums, wgs_relay_bytes(sizeof(float) * 3 * cells)));
    HIP_TRY(bufs.get(&over, sizeof(int32_t) * count));
    HIP_TRY(hipMemcpyAsync(d_inds, inds.data(), sizeof(ZInd) * count, hipMemcpyHostToDevice, ctx->stream));
    // the running class sums cross the shards (common.h: wgs_relay); a class that a shard does not have is handed on untouched
    if (wgs_relay(
            comm, sums, sizeof(float) * 3 * cells, [&](int r) { return wgs_coll_tag{WGS_OP_Z_CLASS, generation, r, i0, 0, 0}; },
            [&](bool continued) { return launch_zclass(ctx, d_inds, count, d->table, b->m, d->mpad, cnt, sums, first, over, continued); }))
        return 1;
    std::vector<int32_t> h_cnt(cells), h_first(cells), h_over(count);
    std::vector<float> h_sums(3 * cells);
    HIP_TRY(hipMemcpyAsync(h_cnt.data(), cnt, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_first.data(), first, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_sums.data(), sums, sizeof(float) * 3 * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_over.data(), over, sizeof(int32_t) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (wgs_comm_check(comm)) return 1;               // (a receiver's view of the senders' rows)
    // counts add; a first site is the smallest global number among the shards that have the class; `over` stays per rank.  One sum
    // all-reduce gathers all three: every rank fills its own row of [world][first + 1 | over] (0: none) behind the counts.
    const size_t nk = (size_t)count * WGS_Z_NKEYS, row = nk + count;
    std::vector<double> wire(nk + (size_t)world * row, 0.0);
    for (int j = 0; j < count; ++j) {
        for (int k = 0; k < WGS_Z_NKEYS; ++k) {
            const size_t e = (size_t)j * WGS_Z_NKEYS + k, o = (size_t)j * 256 + k;
            wire[e] = (double)h_cnt[o];
            wire[nk + (size_t)rank * row + e] = h_first[o] < 0 ? 0.0 : (double)(b->site0 + h_first[o] + 1);
        }
        wire[nk + (size_t)rank * row + nk + j] = (double)h_over[j];
    }
    if (world > 1) {
        const wgs_coll_tag tag = {WGS_OP_Z_CLASS, generation, world, i0, count, 0};
        if (wgs_comm_allreduce_host_tagged(comm, wire.data(), (int64_t)wire.size(), &tag, nullptr)) return 1;
    }
    for (int j = 0; j < count; ++j) {
        for (int k = 0; k < WGS_Z_NKEYS; ++k) {
            const size_t e = (size_t)j * WGS_Z_NKEYS + k;
            counts_out[e] = (int32_t)wire[e];
            int64_t f = -1;
            for (int r = 0; r < world; ++r) {
                const int64_t g = (int64_t)wire[nk + (size_t)r * row + e] - 1;
                if (g >= 0 && (f < 0 || g < f)) f = g;
            }
            first_out[e] = f;
        }
        memcpy(sums_out + (size_t)j * WGS_Z_NKEYS * 3, h_sums.data() + (size_t)j * 256 * 3, sizeof(float) * 3 * WGS_Z_NKEYS);
        for (int r = 0; r < world; ++r) over_out[(size_t)r * count + j] = (int32_t)wire[nk + (size_t)r * row + nk + j];
    }
    return 0;
}

// One shard: the same body without a communicator -- one launch of zclass_kernel<false>, no collective; first sites stay local numbers.
int wgs_zscore_classes(wgs_depth *d, int32_t i0, int32_t count, int32_t *counts_out, float *sums_out, int32_t *first_out, int32_t *over_out)
{
    WGS_REQUIRE(d && counts_out && sums_out && first_out && over_out, "null argument");
    WGS_REQUIRE(d->b, "the depth table was created without a matrix (wgs_depth_create_shape)");
    WGS_REQUIRE(count > 0, "individuals [%d, %d) outside 0..%lld", i0, i0 + count, (long long)d->b->n);
    std::vector<int64_t> first((size_t)count * WGS_Z_NKEYS);
    if (int rc = wgs_zscore_classes_sharded(d, i0, count, nullptr, counts_out, sums_out, first.data(), over_out)) return rc;
    for (size_t e = 0; e < first.size(); ++e) first_out[e] = first[e] < 0 ? -1 : (int32_t)(first[e] - d->b->site0);
    return 0;
}

int wgs_zscore_max_depth(void) { return WGS_Z_MAXD; }

int wgs_zscore_deep_sites(wgs_depth *d, int32_t i0, int32_t count, const int32_t *over, int32_t *site_out, int32_t *depth_out, float *g_out)
{
    WGS_REQUIRE(d && over && site_out && depth_out && g_out, "null argument");
    WGS_REQUIRE(d->b, "the depth table was created without a matrix (wgs_depth_create_shape)");
    wgs_beagle *b = d->b;
    wgs_ctx *ctx = b->ctx;
    std::vector<ZInd> inds;
    if (int rc = zs_fill_inds(b, i0, count, inds)) return rc;
    std::vector<int64_t> obase(count);
    int64_t all = 0;
    for (int j = 0; j < count; ++j) {
        WGS_REQUIRE(over[j] >= 0, "individual %d: a negative number of deep sites", i0 + j);
        obase[j] = all;
        all += over[j];
    }
    if (all == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    ZBufs bufs;
    ZInd *d_inds = nullptr;
    unsigned long long *words = nullptr;
    uint32_t *off = nullptr;
    int64_t *d_total = nullptr, *d_obase = nullptr;
    int32_t *d_site = nullptr, *d_ad = nullptr;
    float *d_g = nullptr;
    const size_t nt = (size_t)wgs_ntiles(b->m);
    HIP_TRY(bufs.get(&d_inds, sizeof(ZInd) * count));
    HIP_TRY(bufs.get(&words, sizeof(unsigned long long) * count * nt));
    HIP_TRY(bufs.get(&off, sizeof(uint32_t) * count * nt));
    HIP_TRY(bufs.get(&d_total, sizeof(int64_t) * count));
    HIP_TRY(bufs.get(&d_obase, sizeof(int64_t) * count));
    HIP_TRY(bufs.get(&d_site, sizeof(int32_t) * all));
    HIP_TRY(bufs.get(&d_ad, sizeof(int32_t) * 2 * all));
    HIP_TRY(bufs.get(&d_g, sizeof(float) * 2 * all));
    HIP_TRY(hipMemcpyAsync(d_inds, inds.data(), sizeof(ZInd) * count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_obase, obase.data(), sizeof(int64_t) * count, hipMemcpyHostToDevice, ctx->stream));
    if (launch_zdeep_flag(ctx, d_inds, count, d->table, b->m, d->mpad, words, off, d_total)) return 1;
    std::vector<int64_t> total(count);
    HIP_TRY(hipMemcpyAsync(total.data(), d_total, sizeof(int64_t) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < count; ++j)         // the gather writes total[j] entries behind obase[j]: the caller's sizes must be the table's
        WGS_REQUIRE(total[j] == over[j], "individual %d has %lld sites deeper than %d reads, the caller expects %d", i0 + j,
                    (long long)total[j], WGS_Z_MAXD, over[j]);
    if (launch_zdeep_gather(ctx, d_inds, count, d->table, b->m, d->mpad, words, off, d_obase, d_site, d_ad, d_g)) return 1;
    HIP_TRY(hipMemcpyAsync(site_out, d_site, sizeof(int32_t) * all, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(depth_out, d_ad, sizeof(int32_t) * 2 * all, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(g_out, d_g, sizeof(float) * 2 * all, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

void wgs_zkeep_destroy(wgs_zkeep *zk)
{
    if (!zk || !wgs_live_remove(zk)) return;
    (void)hipSetDevice(zk->b->ctx->device);
    for (void *p : {(void *)zk->d_inds, (void *)zk->mask, (void *)zk->off, (void *)zk->d_total, (void *)zk->d_deep_map, (void *)zk->d_deep_rows, (void *)zk->d_stats})
        if (p) (void)hipFree(p);
    delete zk;
}

int wgs_zkeep_create(wgs_depth *d, int32_t i0, int32_t count, const float *key_mean, const int32_t *key_comp, int64_t *kept_out,
                     wgs_zkeep **out)
{
    return wgs_zkeep_create_deep(d, i0, count, key_mean, key_comp, nullptr, nullptr, 0, kept_out, out);
}

int wgs_zkeep_create_deep(wgs_depth *d, int32_t i0, int32_t count, const float *key_mean, const int32_t *key_comp, const int32_t *deep_map,
                          const float *deep_rows, int64_t n_deep_rows, int64_t *kept_out, wgs_zkeep **out)
{
    WGS_REQUIRE(d && key_mean && key_comp && kept_out && out, "null argument");
    WGS_REQUIRE(!deep_map || (deep_rows && n_deep_rows > 0 && n_deep_rows < (int64_t)1 << 31), "a deep map needs its rows");
    if (deep_map)                       // the kernels index the rows by what the map says: every kept depth has its d + 1 rows
        for (int64_t e = 0; e < (int64_t)count * WGS_Z_DEEP_MAP; ++e) {
            const int64_t r = deep_map[e], dl = e % WGS_Z_DEEP_MAP;
            WGS_REQUIRE(r == -1 || (dl > WGS_Z_MAXD && r >= 0 && r + dl + 1 <= n_deep_rows), "deep map: depth %lld points outside the rows",
                        (long long)dl);
            for (int64_t a = 0; r >= 0 && a <= dl; ++a) {
                const float c = deep_rows[(r + a) * WGS_Z_DEEP_ROW];
                WGS_REQUIRE(c == 0.0f || c == 1.0f || c == 2.0f, "deep rows: the component must be 0, 1 or 2");
            }
        }
    WGS_REQUIRE(d->b, "the depth table was created without a matrix (wgs_depth_create_shape)");
    wgs_beagle *b = d->b;
    wgs_ctx *ctx = b->ctx;
    std::vector<ZInd> inds;
    if (int rc = zs_fill_inds(b, i0, count, inds)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    wgs_zkeep *zk = new wgs_zkeep();
    wgs_live_add(zk, WGS_LIVE_ZKEEP, b, d);
    auto guard = on_failure([&] { wgs_zkeep_destroy(zk); });
    zk->b = b;
    zk->d = d;
    zk->i0 = i0;
    zk->count = count;
    const size_t nt = (size_t)wgs_ntiles(b->m);
    HIP_TRY(wgs_malloc(&zk->d_inds, sizeof(ZInd) * count));
    HIP_TRY(wgs_malloc(&zk->mask, sizeof(unsigned long long) * count * nt));
    HIP_TRY(wgs_malloc(&zk->off, sizeof(uint32_t) * count * nt));
    HIP_TRY(wgs_malloc(&zk->d_total, sizeof(int64_t) * count));
    ZBufs bufs;
    float *kmean = nullptr;
    int32_t *kcomp = nullptr;
    HIP_TRY(bufs.get(&kmean, sizeof(float) * 256 * count));
    HIP_TRY(bufs.get(&kcomp, sizeof(int32_t) * 256 * count));
    std::vector<float> h_mean((size_t)256 * count, 0.0f);
    std::vector<int32_t> h_comp((size_t)256 * count, -1);
    for (int j = 0; j < count; ++j)
        for (int k = 0; k < WGS_Z_NKEYS; ++k) {
            const int c = key_comp[(size_t)j * WGS_Z_NKEYS + k];
            WGS_REQUIRE(c >= -1 && c <= 2, "key_comp must be -1 (class not kept) or a component 0..2");
            h_mean[(size_t)j * 256 + k] = key_mean[(size_t)j * WGS_Z_NKEYS + k];
            h_comp[(size_t)j * 256 + k] = c;
        }
    HIP_TRY(hipMemcpyAsync(zk->d_inds, inds.data(), sizeof(ZInd) * count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(kmean, h_mean.data(), sizeof(float) * 256 * count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(kcomp, h_comp.data(), sizeof(int32_t) * 256 * count, hipMemcpyHostToDevice, ctx->stream));
    if (deep_map) {
        HIP_TRY(wgs_malloc(&zk->d_deep_map, sizeof(int32_t) * WGS_Z_DEEP_MAP * count));
        HIP_TRY(wgs_malloc(&zk->d_deep_rows, sizeof(float) * WGS_Z_DEEP_ROW * n_deep_rows));
        HIP_TRY(hipMemcpyAsync(zk->d_deep_map, deep_map, sizeof(int32_t) * WGS_Z_DEEP_MAP * count, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(zk->d_deep_rows, deep_rows, sizeof(float) * WGS_Z_DEEP_ROW * n_deep_rows, hipMemcpyHostToDevice, ctx->stream));
    }
    if (launch_zmask(ctx, zk->d_inds, count, d->table, b->m, d->mpad, kmean, kcomp, zk->d_deep_map, zk->d_deep_rows, zk->mask, zk->off,
                     zk->d_total))
        return 1;
    zk->total.resize(count);
    HIP_TRY(hipMemcpyAsync(zk->total.data(), zk->d_total, sizeof(int64_t) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < count; ++j) kept_out[j] = zk->total[j];
    guard.dismiss();
    *out = zk;
    return 0;
}

int wgs_zkeep_sites(wgs_zkeep *zk, int32_t slot, int32_t *sites_out)
{
    WGS_REQUIRE(zk && sites_out && slot >= 0 && slot < zk->count, "bad argument");
    if (zk->total[slot] == 0) return 0;
    wgs_ctx *ctx = zk->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    ZBufs bufs;
    int32_t *d_out = nullptr;
    HIP_TRY(bufs.get(&d_out, sizeof(int32_t) * zk->total[slot]));
    const size_t nt = (size_t)wgs_ntiles(zk->b->m);
    if (launch_zsites(ctx, zk->b->m, zk->mask + slot * nt, zk->off + slot * nt, d_out)) return 1;
    HIP_TRY(hipMemcpyAsync(sites_out, d_out, sizeof(int32_t) * zk->total[slot], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

}   // extern "C"

// The statistic sweep of a kept-site set into d_out = [3][all] (W_l_obs | W_l | var_W_l, the individuals one after the other inside
// each), enqueued on the context's stream; the small inputs live in `bufs` until the caller has waited for the stream.
static int zstats_enqueue(wgs_zkeep *zk, const float *tables, const float *const *freq_dev, const std::vector<int64_t> &obase, int64_t all,
                          ZBufs &bufs, float *d_out)
{
    wgs_beagle *b = zk->b;
    wgs_ctx *ctx = b->ctx;
    const int count = zk->count;
    float *d_tabs = nullptr;
    const float **d_fptr = nullptr;
    int64_t *d_obase = nullptr;
    const size_t tab_bytes = sizeof(float) * 6 * WGS_Z_NKEYS * count;
    HIP_TRY(bufs.get(&d_tabs, tab_bytes));
    HIP_TRY(bufs.get(&d_fptr, sizeof(float *) * count));
    HIP_TRY(bufs.get(&d_obase, sizeof(int64_t) * count));
    HIP_TRY(hipMemcpyAsync(d_tabs, tables, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_fptr, freq_dev, sizeof(float *) * count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_obase, obase.data(), sizeof(int64_t) * count, hipMemcpyHostToDevice, ctx->stream));
    return launch_zstat(ctx, zk->d_inds, count, zk->d->table, b->m, zk->d->mpad, d_tabs, d_fptr, zk->d_deep_map, zk->d_deep_rows, zk->mask, zk->off,
                        d_obase, d_out, d_out + all, d_out + 2 * all);
}

static int zstats_layout(wgs_zkeep *zk, const float *const *freq_dev, std::vector<int64_t> &obase, int64_t *all_out)
{
    const int count = zk->count;
    obase.resize(count);
    int64_t all = 0;
    for (int j = 0; j < count; ++j) {
        WGS_REQUIRE(freq_dev[j], "individual %d has no frequency vector", zk->i0 + j);
        obase[j] = all;
        all += zk->total[j];
    }
    *all_out = all;
    return 0;
}

extern "C" {

int wgs_zscore_stats(wgs_zkeep *zk, const float *tables, const float *const *freq_dev, float *wobs_out, float *wl_out, float *var_out)
{
    WGS_REQUIRE(zk && tables && freq_dev && wobs_out && wl_out && var_out, "null argument");
    wgs_ctx *ctx = zk->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<int64_t> obase;
    int64_t all = 0;
    if (int rc = zstats_layout(zk, freq_dev, obase, &all)) return rc;
    if (all == 0) return 0;
    ZBufs bufs;
    float *d_out = nullptr;
    if (bufs.get(&d_out, sizeof(float) * 3 * all) != hipSuccess) {
        wgs_set_error("hipMalloc of %zu bytes for the per-site statistics failed", sizeof(float) * 3 * (size_t)all);
        return 1;
    }
    if (int rc = zstats_enqueue(zk, tables, freq_dev, obase, all, bufs, d_out)) return rc;
    HIP_TRY(hipMemcpyAsync(wobs_out, d_out, sizeof(float) * all, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(wl_out, d_out + all, sizeof(float) * all, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(var_out, d_out + 2 * all, sizeof(float) * all, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int wgs_zscore_stats_dev(wgs_zkeep *zk, const float *tables, const float *const *freq_dev, const float **dev_out, int64_t *all_out)
{
    WGS_REQUIRE(zk && tables && freq_dev && dev_out && all_out, "null argument");
    wgs_ctx *ctx = zk->b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<int64_t> obase;
    int64_t all = 0;
    if (int rc = zstats_layout(zk, freq_dev, obase, &all)) return rc;
    if (zk->d_stats) (void)hipFree(zk->d_stats);
    zk->d_stats = nullptr;
    zk->stats_all = 0;
    *dev_out = nullptr;
    *all_out = all;
    if (all == 0) return 0;
    if (wgs_malloc(&zk->d_stats, sizeof(float) * 3 * all) != hipSuccess) {
        zk->d_stats = nullptr;
        wgs_set_error("hipMalloc of %zu bytes for the per-site statistics failed", sizeof(float) * 3 * (size_t)all);
        return 1;
    }
    zk->stats_all = all;
    ZBufs bufs;
    if (int rc = zstats_enqueue(zk, tables, freq_dev, obase, all, bufs, zk->d_stats)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));              // (the tables in `bufs` go with this call)
    *dev_out = zk->d_stats;
    return 0;
}

void wgs_zsum_destroy(wgs_zsum *zs)
{
    if (!zs || !wgs_live_remove(zs)) return;
    (void)hipSetDevice(zs->ctx->device);
    (void)hipStreamSynchronize(zs->ctx->stream);
    for (void *p : {(void *)zs->d_run, (void *)zs->d_tail, (void *)zs->d_class, (void *)zs->d_csum, (void *)zs->d_jobs})
        if (p) (void)hipFree(p);
    delete zs;
}

int wgs_zsum_create(wgs_ctx *ctx, int32_t count, wgs_zsum **out)
{
    WGS_REQUIRE(ctx && out, "null argument");
    WGS_REQUIRE(count > 0 && count <= 16384, "a sum state holds between 1 and 16384 individuals, not %d", count);
    HIP_TRY(hipSetDevice(ctx->device));
    wgs_zsum *zs = new wgs_zsum();
    wgs_live_add(zs, WGS_LIVE_ZSUM, nullptr);
    auto guard = on_failure([&] { wgs_zsum_destroy(zs); });
    zs->ctx = ctx;
    zs->count = count;
    zs->total.assign(count, 0);
    const size_t cells = (size_t)count * WGS_ZSUM_ARRAYS;
    HIP_TRY(wgs_malloc(&zs->d_run, sizeof(float) * cells));
    if (wgs_malloc(&zs->d_tail, sizeof(float) * cells * WGS_ZSUM_CHUNK) != hipSuccess) {
        zs->d_tail = nullptr;
        wgs_set_error("hipMalloc of %zu bytes for the open chunks of %d individuals failed", sizeof(float) * cells * WGS_ZSUM_CHUNK, count);
        return 1;
    }
    HIP_TRY(wgs_malloc(&zs->d_class, sizeof(float) * 3 * 256 * (size_t)count));
    HIP_TRY(wgs_malloc(&zs->d_jobs, sizeof(ZSumJob) * cells));
    HIP_TRY(hipMemsetAsync(zs->d_run, 0, sizeof(float) * cells, ctx->stream));                 // +0.0: where np.sum starts
    HIP_TRY(hipMemsetAsync(zs->d_class, 0, sizeof(float) * 3 * 256 * (size_t)count, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    *out = zs;
    return 0;
}

int wgs_zsum_push(wgs_zsum *zs, const float *dev_arrays, int64_t all, const int64_t *kept)
{
    WGS_REQUIRE(zs && kept, "null argument");
    wgs_ctx *ctx = zs->ctx;
    const int count = zs->count;
    int64_t sum = 0;
    for (int j = 0; j < count; ++j) {
        WGS_REQUIRE(kept[j] >= 0 && kept[j] < (int64_t)1 << 31, "individual slot %d: %lld elements in one push", j, (long long)kept[j]);
        sum += kept[j];
    }
    WGS_REQUIRE(sum == all, "the push holds %lld elements per array, the kept counts add up to %lld", (long long)all, (long long)sum);
    WGS_REQUIRE(all == 0 || dev_arrays, "null argument");
    if (all == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<ZSumJob> jobs((size_t)count * WGS_ZSUM_ARRAYS);
    int64_t obase = 0, cbase = 0;
    int max_full = 0;
    for (int j = 0; j < count; ++j) {
        const int32_t fill = (int32_t)(zs->total[j] % WGS_ZSUM_CHUNK);
        const int32_t nfull = (int32_t)((fill + kept[j]) / WGS_ZSUM_CHUNK);
        for (int a = 0; a < WGS_ZSUM_ARRAYS; ++a) {
            const size_t e = (size_t)j * WGS_ZSUM_ARRAYS + a;
            jobs[e] = ZSumJob{dev_arrays + (size_t)a * all + obase, zs->d_tail + e * WGS_ZSUM_CHUNK, zs->d_run + e, kept[j], cbase, fill, nfull};
            cbase += nfull;
        }
        if (nfull > max_full) max_full = nfull;
        obase += kept[j];
    }
    if ((size_t)cbase > zs->csum_cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (zs->d_csum) (void)hipFree(zs->d_csum);
        zs->d_csum = nullptr;
        zs->csum_cap = 0;
        HIP_TRY(wgs_malloc(&zs->d_csum, sizeof(float) * (size_t)cbase));
        zs->csum_cap = (size_t)cbase;
    }
    HIP_TRY(hipMemcpyAsync(zs->d_jobs, jobs.data(), sizeof(ZSumJob) * jobs.size(), hipMemcpyHostToDevice, ctx->stream));
    if (launch_zsum_push(ctx, zs->d_jobs, (int)jobs.size(), max_full, zs->d_csum)) return 1;
    HIP_TRY(hipStreamSynchronize(ctx->stream));              // (`jobs` and the caller's arrays may go)
    for (int j = 0; j < count; ++j) zs->total[j] += kept[j];
    return 0;
}

int wgs_zsum_totals(wgs_zsum *zs, int64_t *total_out)
{
    WGS_REQUIRE(zs && total_out, "null argument");
    for (int j = 0; j < zs->count; ++j) total_out[j] = zs->total[j];
    return 0;
}

int wgs_zsum_finish(wgs_zsum *zs, float *run_out, float *tails_out)
{
    WGS_REQUIRE(zs && run_out && tails_out, "null argument");
    wgs_ctx *ctx = zs->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t cells = (size_t)zs->count * WGS_ZSUM_ARRAYS;
    HIP_TRY(hipMemcpyAsync(run_out, zs->d_run, sizeof(float) * cells, hipMemcpyDeviceToHost, ctx->stream));
    size_t at = 0;
    for (int j = 0; j < zs->count; ++j) {
        const size_t fill = (size_t)(zs->total[j] % WGS_ZSUM_CHUNK);
        for (int a = 0; a < WGS_ZSUM_ARRAYS && fill; ++a) {
            const size_t e = (size_t)j * WGS_ZSUM_ARRAYS + a;
            HIP_TRY(hipMemcpyAsync(tails_out + at, zs->d_tail + e * WGS_ZSUM_CHUNK, sizeof(float) * fill, hipMemcpyDeviceToHost, ctx->stream));
            at += fill;
        }
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int wgs_zscore_classes_carry(wgs_depth *d, int32_t i0, int32_t count, wgs_zsum *zs, int32_t *counts_out, float *sums_out, int32_t *first_out,
                             int32_t *over_out)
{
    WGS_REQUIRE(d && zs && counts_out && sums_out && first_out && over_out, "null argument");
    WGS_REQUIRE(d->b, "the depth table was created without a matrix (wgs_depth_create_shape)");
    WGS_REQUIRE(count == zs->count, "the sum state holds %d individuals, the sweep %d", zs->count, count);
    wgs_beagle *b = d->b;
    wgs_ctx *ctx = b->ctx;
    WGS_REQUIRE(ctx == zs->ctx, "the sum state and the depth table belong to different contexts");
    std::vector<ZInd> inds;
    if (int rc = zs_fill_inds(b, i0, count, inds)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ZBufs bufs;
    ZInd *d_inds = nullptr;
    int32_t *cnt = nullptr, *first = nullptr, *over = nullptr;
    const size_t cells = (size_t)count * 256;
    HIP_TRY(bufs.get(&d_inds, sizeof(ZInd) * count));
    HIP_TRY(bufs.get(&cnt, sizeof(int32_t) * cells));
    HIP_TRY(bufs.get(&first, sizeof(int32_t) * cells));
    HIP_TRY(bufs.get(&over, sizeof(int32_t) * count));
    HIP_TRY(hipMemcpyAsync(d_inds, inds.data(), sizeof(ZInd) * count, hipMemcpyHostToDevice, ctx->stream));
    // the first window starts the chains at 0, every later one goes on from what the window before left in the state
    if (launch_zclass(ctx, d_inds, count, d->table, b->m, d->mpad, cnt, zs->d_class, first, over, zs->class_windows > 0)) return 1;
    std::vector<int32_t> h_cnt(cells), h_first(cells);
    std::vector<float> h_sums(3 * cells);
    HIP_TRY(hipMemcpyAsync(h_cnt.data(), cnt, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_first.data(), first, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_sums.data(), zs->d_class, sizeof(float) * 3 * cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(over_out, over, sizeof(int32_t) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    zs->class_windows += 1;
    for (int j = 0; j < count; ++j) {
        memcpy(counts_out + (size_t)j * WGS_Z_NKEYS, h_cnt.data() + (size_t)j * 256, sizeof(int32_t) * WGS_Z_NKEYS);
        memcpy(first_out + (size_t)j * WGS_Z_NKEYS, h_first.data() + (size_t)j * 256, sizeof(int32_t) * WGS_Z_NKEYS);
        memcpy(sums_out + (size_t)j * WGS_Z_NKEYS * 3, h_sums.data() + (size_t)j * 256 * 3, sizeof(float) * 3 * WGS_Z_NKEYS);
    }
    return 0;
}

int wgs_depth_copy_rows(wgs_depth *dst, int64_t dst_row0, wgs_depth *src, int64_t src_row0, int64_t nrows)
{
    WGS_REQUIRE(dst && src && dst != src, "null argument");
    WGS_REQUIRE(dst->ctx == src->ctx && dst->n == src->n, "the two depth tables differ in context or individuals (%lld, %lld)",
                (long long)dst->n, (long long)src->n);
    WGS_REQUIRE(nrows >= 0 && dst_row0 >= 0 && dst_row0 + nrows <= dst->m && src_row0 >= 0 && src_row0 + nrows <= src->m,
                "rows [%lld, %lld) of %lld into rows [%lld, %lld) of %lld", (long long)src_row0, (long long)(src_row0 + nrows), (long long)src->m,
                (long long)dst_row0, (long long)(dst_row0 + nrows), (long long)dst->m);
    if (nrows == 0) return 0;
    wgs_ctx *ctx = dst->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy2DAsync(dst->table + dst_row0, (size_t)dst->mpad * sizeof(uchar2), src->table + src_row0, (size_t)src->mpad * sizeof(uchar2),
                             (size_t)nrows * sizeof(uchar2), (size_t)dst->n, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// The masked fit of one shard (kept_total = NULL, comm = NULL: the divisor is the set's own kept count, no hop) and of many.
static int em_fit_masked(wgs_em *em, wgs_zkeep *zk, const int32_t *fit_slot, int32_t max_iter, double tole, const int64_t *kept_total,
                         wgs_comm *comm, int32_t *iters_out)
{
    WGS_REQUIRE(em && zk && fit_slot && iters_out, "null argument");
    if (!kept_total) kept_total = zk->total.data();
    WGS_REQUIRE(em->b == zk->b, "the EM batch and the kept-site set belong to different matrices");
    wgs_beagle *b = em->b;
    wgs_ctx *ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const int32_t generation = comm ? wgs_comm_next_generation(comm) : 0;
    const int nf = em->n_fits;
    int64_t stride = 1;                      // (an individual may have kept nothing in THIS shard: its chain hands the carry on)
    for (int j = 0; j < nf; ++j) {
        WGS_REQUIRE(fit_slot[j] >= 0 && fit_slot[j] < zk->count, "fit %d: slot %d outside the kept-site set", j, fit_slot[j]);
        WGS_REQUIRE(kept_total[fit_slot[j]] > 0, "fit %d: no site was kept", j);
        WGS_REQUIRE(kept_total[fit_slot[j]] >= zk->total[fit_slot[j]], "fit %d: kept_total is smaller than this shard's kept count", j);
        if (zk->total[fit_slot[j]] > stride) stride = zk->total[fit_slot[j]];
        iters_out[j] = 0;
    }
    ZBufs bufs;
    float *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    ZCompactJob *d_cj = nullptr;
    ChainJob *d_jobs = nullptr;
    void *work = nullptr;
    const size_t vec_bytes = sizeof(float) * (size_t)nf * stride;
    if (bufs.get(&d_a, vec_bytes) != hipSuccess || bufs.get(&d_b, vec_bytes) != hipSuccess) {
        wgs_set_error("hipMalloc of 2 x %zu bytes for the compacted frequencies failed", vec_bytes);
        return 1;
    }
    HIP_TRY(bufs.get(&d_out, wgs_relay_bytes(sizeof(float) * nf)));
    HIP_TRY(bufs.get(&d_cj, sizeof(ZCompactJob) * nf));
    HIP_TRY(bufs.get(&d_jobs, sizeof(ChainJob) * nf));
    HIP_TRY(bufs.get(&work, rmse_chain_workspace_bytes(stride) * nf));
    HIP_TRY(hipMemsetAsync(d_a, 0, vec_bytes, ctx->stream));       // what lies behind a fit's kept count stays 0: (0 - 0)^2 adds nothing
    HIP_TRY(hipMemsetAsync(d_b, 0, vec_bytes, ctx->stream));
    std::vector<ZCompactJob> cj(nf);
    std::vector<ChainJob> jobs(nf);
    std::vector<float> carry(nf);
    std::vector<int> list;
    for (int it = 1; it <= max_iter; ++it) {
        list.clear();
        for (int j = 0; j < nf; ++j)
            if (em->active[j]) list.push_back(j);
        if (list.empty()) break;
        if (wgs_em_step_dev(em, em->d_ssq)) return 1;               // the existing sweep over this shard: no sum crosses the ranks
        const int nj = (int)list.size();
        for (int q = 0; q < nj; ++q) {
            const int j = list[q];
            float *va = d_a + (size_t)j * stride, *vb = d_b + (size_t)j * stride;
            cj[q] = ZCompactJob{em_f(em, j, em->cur[j]), em_f(em, j, em->prev[j]), va, vb, fit_slot[j]};
            jobs[q] = ChainJob{va, vb, 0.0f};
        }
        HIP_TRY(hipMemcpyAsync(d_cj, cj.data(), sizeof(ZCompactJob) * nj, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(ChainJob) * nj, hipMemcpyHostToDevice, ctx->stream));
        if (launch_zcompact(ctx, d_cj, nj, b->m, zk->mask, zk->off)) return 1;
        // the chain over the kept sites crosses the shards as wgs_em_fit's chains do
        if (em_relay_chains(ctx, comm, WGS_OP_Z_CHAIN, generation, it, d_jobs, nj, stride, d_out, work, nullptr, carry.data())) return 1;
        for (int q = 0; q < nj; ++q) {
            const int j = list[q];
            if (em_chain_converged(carry[q], kept_total[fit_slot[j]], tole)) {    // n = the kept sites of ALL shards: the same value on every rank
                iters_out[j] = it;
                em->active[j] = 0;
            }
        }
    }
    return 0;
}

int wgs_em_fit_masked(wgs_em *em, wgs_zkeep *zk, const int32_t *fit_slot, int32_t max_iter, double tole, int32_t *iters_out)
{
    return em_fit_masked(em, zk, fit_slot, max_iter, tole, nullptr, nullptr, iters_out);
}

int wgs_em_fit_masked_sharded(wgs_em *em, wgs_zkeep *zk, const int32_t *fit_slot, int32_t max_iter, double tole, const int64_t *kept_total,
                              wgs_comm *comm, int32_t *iters_out)
{
    WGS_REQUIRE(kept_total, "null argument");
    return em_fit_masked(em, zk, fit_slot, max_iter, tole, kept_total, comm, iters_out);
}

/* Test hook (include/wgsassign_hip_debug.h): a push of HOST arrays -- [3][all], as wgs_zsum_push takes them on the device. */
int wgs_debug_zsum_push(wgs_zsum *zs, const float *host_arrays, int64_t all, const int64_t *kept)
{
    WGS_REQUIRE(zs && kept && (all == 0 || host_arrays) && all >= 0, "null argument");
    if (all == 0) return wgs_zsum_push(zs, nullptr, 0, kept);
    HIP_TRY(hipSetDevice(zs->ctx->device));
    ZBufs bufs;
    float *d_x = nullptr;
    HIP_TRY(bufs.get(&d_x, sizeof(float) * 3 * (size_t)all));
    HIP_TRY(hipMemcpyAsync(d_x, host_arrays, sizeof(float) * 3 * (size_t)all, hipMemcpyHostToDevice, zs->ctx->stream));
    return wgs_zsum_push(zs, d_x, all, kept);                // (waits for the stream before it returns)
}

}   // extern "C"
