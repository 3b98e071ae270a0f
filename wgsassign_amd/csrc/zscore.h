// Internal declarations of the z-score path (zscore_kernels.hip, zscore_api.hip).
#pragma once
#include "common.h"
#include "streams.h"       // the kinds of the live-object registry: WGS_LIVE_DEPTH, WGS_LIVE_ZKEEP, WGS_LIVE_ZSUM

constexpr int WGS_Z_MAXD = 21;                                        // largest depth Ar + Aa with a class of its own
constexpr int WGS_Z_NKEYS = (WGS_Z_MAXD + 1) * (WGS_Z_MAXD + 2) / 2;  // 253 classes: one per thread of a 256-thread workgroup

// The deep tier: depth pairs with WGS_Z_MAXD < Ar + Aa <= 255 + 255 (what the table's bytes hold) have no class of the dense 253.  A
// kept-site set may carry a deep table in global memory: per individual a map depth -> first row (-1: depth not kept), and per kept
// depth d the rows a = 0 .. d of {component, mean of class (d - a, a) | AD_like[0..2], AD_factorial[0..2] at AD_index[a, d - a]}.
constexpr int WGS_Z_DEEP_MAP = 511, WGS_Z_DEEP_ROW = 8;

struct ZInd {                  // one individual as the sweeps see it
    const float4 *slab;
    int32_t npairs, pair, hi;  // its column's pair inside the slab and which half of the float4
    int32_t ind;               // global index (row of the depth table)
};
struct ZCompactJob {
    const float *cur, *prev;
    float *a_out, *b_out;      // the fit's own compacted vectors
    int32_t slot;              // individual of the kept-site set whose mask applies
};

struct wgs_depth {
    wgs_beagle *b = nullptr;   // nullptr: a table of its own shape (wgs_depth_create_shape), for nothing but filling and reading back
    wgs_ctx *ctx = nullptr;
    int64_t m = 0, n = 0;
    int64_t mpad = 0;
    uchar2 *table = nullptr;   // [individual][mpad]
    int32_t *d_bad = nullptr;
};
struct wgs_zkeep {
    wgs_beagle *b = nullptr;
    wgs_depth *d = nullptr;
    int32_t i0 = 0, count = 0;
    ZInd *d_inds = nullptr;
    unsigned long long *mask = nullptr;   // [count][ntiles]
    uint32_t *off = nullptr;              // [count][ntiles]
    int64_t *d_total = nullptr;
    std::vector<int64_t> total;
    int32_t *d_deep_map = nullptr;        // [count][WGS_Z_DEEP_MAP], nullptr: no individual of the set kept a deep depth
    float *d_deep_rows = nullptr;         // [rows][WGS_Z_DEEP_ROW]
    float *d_stats = nullptr;             // wgs_zscore_stats_dev: the three compacted arrays of the last call, [3][stats_all]
    int64_t stats_all = 0;
};

// np.sum's float32 order continued from site window to site window (zscore_kernels.hip: zsum_*): per (individual, array) the running
// float32 over the closed 8192-element chunks and the elements of the open one.  Also the class sweep's running sums of a windowed pass.
constexpr int WGS_ZSUM_CHUNK = 8192, WGS_ZSUM_ARRAYS = 3;
struct ZSumJob {
    const float *x;            // the window's compacted array of this (individual, array): k elements
    float *tail, *run;         // the open chunk (WGS_ZSUM_CHUNK floats) and the running value
    int64_t k;
    int64_t cbase;             // where this job's chunk sums begin
    int32_t fill, nfull;       // elements in the open chunk before the push; chunks the push closes
};
struct wgs_zsum {
    wgs_ctx *ctx = nullptr;
    int32_t count = 0;
    float *d_run = nullptr;    // [count][3]
    float *d_tail = nullptr;   // [count][3][WGS_ZSUM_CHUNK]
    float *d_class = nullptr;  // [count][256][3]: zclass_kernel's running sums (wgs_zscore_classes_carry)
    float *d_csum = nullptr;   // chunk sums of a push
    size_t csum_cap = 0;
    ZSumJob *d_jobs = nullptr; // [count * 3]
    std::vector<int64_t> total;            // elements pushed per individual
    int64_t class_windows = 0;             // windows wgs_zscore_classes_carry has swept
};

int zs_fill_inds(wgs_beagle *b, int32_t i0, int32_t count, std::vector<ZInd> &out);
// carry: the chains go on from what `sums` holds (a later SNP shard) instead of starting at 0
int launch_zclass(wgs_ctx *ctx, const ZInd *d_inds, int count, const uchar2 *depth, int64_t m, int64_t mpad, int32_t *cnt, float *sums,
                  int32_t *first, int32_t *over, bool carry = false);
int launch_zmask(wgs_ctx *ctx, const ZInd *d_inds, int count, const uchar2 *depth, int64_t m, int64_t mpad, const float *kmean,
                 const int32_t *kcomp, const int32_t *dmap, const float *drows, unsigned long long *mask, uint32_t *off, int64_t *total);
int launch_zstat(wgs_ctx *ctx, const ZInd *d_inds, int count, const uchar2 *depth, int64_t m, int64_t mpad, const float *tabs,
                 const float *const *fptr, const int32_t *dmap, const float *drows, const unsigned long long *mask, const uint32_t *off,
                 const int64_t *obase, float *wobs, float *wl, float *var);
int launch_zdeep_flag(wgs_ctx *ctx, const ZInd *d_inds, int count, const uchar2 *depth, int64_t m, int64_t mpad, unsigned long long *words,
                      uint32_t *off, int64_t *total);
int launch_zdeep_gather(wgs_ctx *ctx, const ZInd *d_inds, int count, const uchar2 *depth, int64_t m, int64_t mpad,
                        const unsigned long long *words, const uint32_t *off, const int64_t *obase, int32_t *site, int32_t *ad, float *g);
int launch_zcompact(wgs_ctx *ctx, const ZCompactJob *d_jobs, int n_jobs, int64_t m, const unsigned long long *mask, const uint32_t *off);
int launch_zdepth_scatter(wgs_ctx *ctx, const int32_t *d_rows, int64_t nrows, int64_t n, int64_t row0, int64_t mpad, uchar2 *depth, int32_t *bad);
int launch_zdepth_gather(wgs_ctx *ctx, const uchar2 *depth, int64_t nrows, int64_t n, int64_t row0, int64_t mpad, int32_t *d_rows);
int launch_zsites(wgs_ctx *ctx, int64_t m, const unsigned long long *mask, const uint32_t *off, int32_t *out);
// the jobs' full chunks reduced in NumPy's order into csum, added to the running values in chunk order, the new open chunks stored
int launch_zsum_push(wgs_ctx *ctx, const ZSumJob *d_jobs, int n_jobs, int max_full, float *csum);
