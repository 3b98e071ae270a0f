// Kernels of the z-score options (reference zscore.py, zscore_cy.pyx): depth-class sweep, site mask, per-site statistic, and the
// compaction that feeds the masked convergence chain.  Lane <-> SNP for everything that reads the slabs; host glue: zscore_api.hip.
#include "zscore.h"
#include "log_table.h"

namespace {

__device__ double2 zs_log_table_dev[WGS_LOG_N];

// (float)log((double)s) as libm rounds it: the table logarithm of assign_kernels.hip (log_f32arg / logf_of_f32, same table, same
// sequence of operations -- restated here because a __device__ table belongs to one translation unit), one LDS copy of the table:
// this sweep is bound by its serial per-site loops, not by LDS conflicts.
__device__ __forceinline__ float zs_logf(float s, const double2 *tab)
{
    const double x = (double)s;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    const unsigned int hi = (unsigned int)(bits >> 32), lo = (unsigned int)bits;
    const unsigned int tmp = hi - WGS_LOG_OFF;
    const int k = (int)tmp >> 20;
    const unsigned int i = (tmp >> 13) & (WGS_LOG_N - 1);
    const double z = __hiloint2double((int)(hi - (tmp & 0xFFF00000u)), (int)lo);
    const double2 t = tab[i];
    const double r = __builtin_fma(z, t.x, -1.0);
    const double kd = (double)k;
    const double w = __builtin_fma(kd, WGS_LN2HI, t.y);
    const double hi_ = w + r;
    const double lo_ = __builtin_fma(kd, WGS_LN2LO, (w - hi_) + r);
    double q = __builtin_fma(r, -0.125, 1.0 / 7.0);
    q = __builtin_fma(r, q, -1.0 / 6.0);
    q = __builtin_fma(r, q, 0.2);
    q = __builtin_fma(r, q, -0.25);
    q = __builtin_fma(r, q, 1.0 / 3.0);
    q = __builtin_fma(r, q, -0.5);
    const float v = (float)(__builtin_fma(r * r, q, lo_) + hi_);
    // -inf / +inf / NaN exactly where libm returns them: v_log_f32 takes a subnormal for a zero of its sign, so a negative subnormal
    // (libm: NaN) would come out as -inf -- every negative argument goes in as -1 (log_special of assign_kernels.hip)
    const float special = __builtin_amdgcn_logf(__builtin_isfpclass(s, 0x0004 | 0x0008 | 0x0010) ? -1.0f : s);   // -inf | -normal | -subnormal
    return __builtin_isfpclass(s, 0x0100 | 0x0080) ? v : special;
}

__device__ __forceinline__ const double2 *zs_load_log_table(double2 *tab)
{
    for (int e = threadIdx.x; e < WGS_LOG_N; e += blockDim.x) tab[e] = zs_log_table_dev[e];
    __syncthreads();
    return tab;
}

// Class of a depth pair: d (d + 1) / 2 + Aa for depth d = Ar + Aa <= WGS_Z_MAXD; ZK_OVER beyond (the deep tier: zscore.h), ZK_NONE for a
// lane past the last site.
constexpr int ZK_OVER = 254, ZK_NONE = 255;
__device__ __forceinline__ int zs_key(uchar2 d, bool valid)
{
    const int dl = (int)d.x + (int)d.y;
    return !valid ? ZK_NONE : dl > WGS_Z_MAXD ? ZK_OVER : dl * (dl + 1) / 2 + (int)d.y;
}

struct ZSite {
    float g0, g1;
    uchar2 d;
};
__device__ __forceinline__ ZSite zs_load(const ZInd &I, const uchar2 *__restrict__ depth, int64_t mpad, int64_t tile, int lane)
{
    const float4 v = I.slab[((size_t)tile * I.npairs + I.pair) * 64 + lane];
    ZSite s;
    s.g0 = I.hi ? v.z : v.x;
    s.g1 = I.hi ? v.w : v.y;
    s.d = depth[(size_t)I.ind * mpad + (size_t)tile * 64 + lane];
    return s;
}

// zscore.py:AD_summary, lines 11-21 -- per (individual, depth pair) the number of sites, the float32 sums of (g0, g1, 1 - g0 - g1) IN SITE
// ORDER (np.mean over a (count, 3) float32 array adds row by row) and the first site (the dictionary's insertion order).
// One workgroup per individual; thread <-> CLASS (4 wavefronts x 64 classes), and the wavefront walks the sites: 64 at a time are
// loaded lane <-> SNP (the next tile's loads are issued before this tile is walked), then the sites whose class this wavefront
// owns are taken in order -- class and triple broadcast from the owning lane, the one thread of that class adds.  Every sum is
// the literal serial chain, so its bits are the reference's by construction.
// CARRY: the SNP shard is not the first one -- `sums` holds, per (individual, class), the three running values the shard before
// ended with, and the chains go on from them (a class without a site in this shard hands them on as they are).  cnt, first and
// over speak of this shard alone.  Without CARRY the chains start at 0: the kernel of one shard.
template <bool CARRY>
__global__ __launch_bounds__(256) void zclass_kernel(const ZInd *__restrict__ inds, const uchar2 *__restrict__ depth, int64_t m, int64_t mpad,
                                                     int32_t *__restrict__ cnt, float *__restrict__ sums, int32_t *__restrict__ first,
                                                     int32_t *__restrict__ over)
{
    const ZInd I = inds[blockIdx.x];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t ntiles = (m + 63) >> 6;
    const size_t o = (size_t)blockIdx.x * 256 + tid;
    int c = 0, f = -1, nover = 0;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    if (CARRY) {
        s0 = sums[o * 3 + 0];
        s1 = sums[o * 3 + 1];
        s2 = sums[o * 3 + 2];
    }
    ZSite cur = zs_load(I, depth, mpad, 0, lane);
    for (int64_t t = 0; t < ntiles; ++t) {
        ZSite nxt = cur;
        if (t + 1 < ntiles) nxt = zs_load(I, depth, mpad, t + 1, lane);
        const int64_t site = t * 64 + lane;
        const int k = zs_key(cur.d, site < m);
        const float g2 = (1.0f - cur.g0) - cur.g1;
        unsigned long long mine = __ballot((k >> 6) == wave && k < WGS_Z_NKEYS);
        if (wave == 0) nover += __popcll(__ballot(k == ZK_OVER));
        while (mine) {
            const int j = __builtin_ctzll(mine);
            mine &= mine - 1;
            const int kj = __builtin_amdgcn_readlane(k, j);
            const float x0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.g0), j));
            const float x1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.g1), j));
            const float x2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g2), j));
            if (tid == kj) {
                if (c == 0) f = (int)(t * 64 + j);
                ++c;
                s0 = s0 + x0;
                s1 = s1 + x1;
                s2 = s2 + x2;
            }
        }
        cur = nxt;
    }
    cnt[o] = c;
    first[o] = f;
    sums[o * 3 + 0] = s0;
    sums[o * 3 + 1] = s1;
    sums[o * 3 + 2] = s2;
    if (tid == 0) over[blockIdx.x] = nover;
}

// zscore.py:get_L_keep -- the site's class survived the key filter (kcomp >= 0: the component where the class mean is largest) and
// the site's own value there is within float32(0.01) of the mean.  One 64-bit word per (individual, tile).
// DEEP: the individuals have a deep table (zscore.h) -- a site of depth > WGS_Z_MAXD whose depth d survived whole (dmap[d] >= 0) finds
// the component and the mean of its class in row dmap[d] + Aa of that table, in global memory; without a table (the instantiation
// that data without deep sites launches) such a site has no class and is dropped.
constexpr int ZS_TILES_PER_BLOCK = 64;
template <bool DEEP>
__global__ __launch_bounds__(256) void zmask_kernel(const ZInd *__restrict__ inds, const uchar2 *__restrict__ depth, int64_t m, int64_t mpad,
                                                    const float *__restrict__ kmean, const int32_t *__restrict__ kcomp,
                                                    const int32_t *__restrict__ dmap, const float *__restrict__ drows,
                                                    unsigned long long *__restrict__ mask)
{
    __shared__ float mean_s[256];
    __shared__ int comp_s[256];
    const ZInd I = inds[blockIdx.y];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    mean_s[tid] = kmean[(size_t)blockIdx.y * 256 + tid];
    comp_s[tid] = kcomp[(size_t)blockIdx.y * 256 + tid];
    __syncthreads();
    const int64_t ntiles = (m + 63) >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * ZS_TILES_PER_BLOCK;
    for (int64_t t = t0 + wave; t < t0 + ZS_TILES_PER_BLOCK && t < ntiles; t += 4) {
        const ZSite s = zs_load(I, depth, mpad, t, lane);
        const int k = zs_key(s.d, t * 64 + lane < m);
        bool keep = false;
        if (k < WGS_Z_NKEYS) {
            const int c = comp_s[k];
            const float g2 = (1.0f - s.g0) - s.g1;
            const float v = c == 0 ? s.g0 : c == 1 ? s.g1 : g2;
            keep = c >= 0 && !(fabsf(mean_s[k] - v) > 0.01f);
        }
        if (DEEP && k == ZK_OVER) {
            const int r = dmap[(size_t)blockIdx.y * WGS_Z_DEEP_MAP + (int)s.d.x + (int)s.d.y];
            if (r >= 0) {
                const float *row = drows + ((size_t)r + s.d.y) * WGS_Z_DEEP_ROW;
                const int c = (int)row[0];
                const float g2 = (1.0f - s.g0) - s.g1;
                const float v = c == 0 ? s.g0 : c == 1 ? s.g1 : g2;
                keep = !(fabsf(row[1] - v) > 0.01f);
            }
        }
        const unsigned long long w = __ballot(keep);
        if (lane == 0) mask[(size_t)blockIdx.y * ntiles + t] = w;
    }
}

// Exclusive prefix over the tiles of the kept sites per individual: where a tile's sites go in the compacted arrays.
__global__ __launch_bounds__(256) void zscan_kernel(const unsigned long long *__restrict__ mask, int64_t ntiles, uint32_t *__restrict__ off,
                                                    int64_t *__restrict__ total)
{
    __shared__ unsigned int part[256];
    const int tid = threadIdx.x;
    const unsigned long long *w = mask + (size_t)blockIdx.x * ntiles;
    const int64_t per = (ntiles + 255) / 256;
    const int64_t lo = tid * per < ntiles ? tid * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
    unsigned int s = 0;
    for (int64_t t = lo; t < hi; ++t) s += (unsigned int)__popcll(w[t]);
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned int run = 0;
        for (int i = 0; i < 256; ++i) {
            const unsigned int v = part[i];
            part[i] = run;
            run += v;
        }
        total[blockIdx.x] = run;
    }
    __syncthreads();
    unsigned int run = part[tid];
    for (int64_t t = lo; t < hi; ++t) {
        off[(size_t)blockIdx.x * ntiles + t] = run;
        run += (unsigned int)__popcll(w[t]);
    }
}

// zscore_cy.pyx:expected_W_l and variance_W_l for the kept sites, as the C translation of the reference computes them (what the
// recorded outputs pin): 1 - A and 2 (1 - A) A in float64 -- the literals are doubles --, A A in float32; g0 P0 and g1 P1 float32
// products, ((1 - g0) - g1) P2 in float64; the logarithm in float64 of the float32 sum; W_l and var_W_l accumulate over
// Aa = 0 .. Dl in float32, three terms per step, one rounding per product and per sum (built with -ffp-contract=off).
// tab: per class row d (d + 1) / 2 + Aa the values the reference reads at AD_index[Aa, Dl - Aa] -- AD_like[0..2], AD_factorial[0..2].
// The results go to the individual's compacted arrays in site order.
// The two loops over Aa = 0 .. dl of a site; row a of the table at row + a * STRIDE: AD_like[0..2], AD_factorial[0..2].
template <int STRIDE>
__device__ __forceinline__ void zs_loops(const float *row, int dl, float P0, float P1, float P2, const double2 *lt, float &wl_out, float &var_out)
{
    float wl = 0.0f;
    for (int a = 0; a <= dl; ++a) {
        const float *r = row + a * STRIDE;
        const float lg = zs_logf((r[0] * P0 + r[1] * P1) + r[2] * P2, lt);
        wl = wl + (lg * P0) * r[3];
        wl = wl + (lg * P1) * r[4];
        wl = wl + (lg * P2) * r[5];
    }
    float var = 0.0f;
    for (int a = 0; a <= dl; ++a) {
        const float *r = row + a * STRIDE;
        const float lg = zs_logf((r[0] * P0 + r[1] * P1) + r[2] * P2, lt);
        const float d = wl - lg;
        var = var + ((d * d) * P0) * r[3];
        var = var + ((d * d) * P1) * r[4];
        var = var + ((d * d) * P2) * r[5];
    }
    wl_out = wl;
    var_out = var;
}

template <bool DEEP>
__global__ __launch_bounds__(256) void zstat_kernel(const ZInd *__restrict__ inds, const uchar2 *__restrict__ depth, int64_t m, int64_t mpad,
                                                    const float *__restrict__ tabs, const float *const *__restrict__ fptr,
                                                    const int32_t *__restrict__ dmap, const float *__restrict__ drows,
                                                    const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ off,
                                                    const int64_t *__restrict__ obase, float *__restrict__ wobs_out,
                                                    float *__restrict__ wl_out, float *__restrict__ var_out)
{
    __shared__ double2 log_s[WGS_LOG_N];
    __shared__ float tab_s[WGS_Z_NKEYS * 6];
    const ZInd I = inds[blockIdx.y];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int e = tid; e < WGS_Z_NKEYS * 6; e += 256) tab_s[e] = tabs[(size_t)blockIdx.y * WGS_Z_NKEYS * 6 + e];
    const double2 *lt = zs_load_log_table(log_s);          // (synchronises)
    const float *__restrict__ fr = fptr[blockIdx.y];
    const int64_t ntiles = (m + 63) >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * ZS_TILES_PER_BLOCK;
    const int64_t ob = obase[blockIdx.y];
    for (int64_t t = t0 + wave; t < t0 + ZS_TILES_PER_BLOCK && t < ntiles; t += 4) {
        const unsigned long long w = mask[(size_t)blockIdx.y * ntiles + t];
        if (!((w >> lane) & 1ull)) continue;
        const ZSite s = zs_load(I, depth, mpad, t, lane);
        const float A = fr[t * 64 + lane];
        const double Ad = (double)A, om = 1.0 - Ad;
        const float P0 = (float)(om * om);
        const float P1 = (float)((2.0 * om) * Ad);
        const float P2 = A * A;
        const float f0 = s.g0 * P0, f1 = s.g1 * P1;
        const float f2 = (float)(((1.0 - (double)s.g0) - (double)s.g1) * (double)P2);
        const float wobs = zs_logf((f0 + f1) + f2, lt);
        const int dl = (int)s.d.x + (int)s.d.y;              // the site's class was kept: <= WGS_Z_MAXD, or a kept depth of the deep table
        float wl, var;
        if (DEEP && dl > WGS_Z_MAXD)                         // (the mask kept it: its depth has rows)
            zs_loops<WGS_Z_DEEP_ROW>(drows + (size_t)dmap[(size_t)blockIdx.y * WGS_Z_DEEP_MAP + dl] * WGS_Z_DEEP_ROW + 2, dl, P0, P1, P2, lt, wl, var);
        else
            zs_loops<6>(tab_s + dl * (dl + 1) / 2 * 6, dl, P0, P1, P2, lt, wl, var);
        const size_t pos = (size_t)ob + off[(size_t)blockIdx.y * ntiles + t] + (unsigned int)__popcll(w & ((1ull << lane) - 1ull));
        wobs_out[pos] = wobs;
        wl_out[pos] = wl;
        var_out[pos] = var;
    }
}

// The deep-site list (sites of depth > WGS_Z_MAXD, which zclass_kernel only counts): one 64-bit word per (individual, tile) from the
// depth table alone, zscan_kernel for the offsets, then the sites of the non-empty tiles in site order -- index, (Ar, Aa), (g0, g1).
__global__ __launch_bounds__(256) void zdeepflag_kernel(const ZInd *__restrict__ inds, const uchar2 *__restrict__ depth, int64_t m, int64_t mpad,
                                                        unsigned long long *__restrict__ words)
{
    const int32_t ind = inds[blockIdx.y].ind;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t ntiles = (m + 63) >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * ZS_TILES_PER_BLOCK;
    for (int64_t t = t0 + wave; t < t0 + ZS_TILES_PER_BLOCK && t < ntiles; t += 4) {
        const uchar2 d = depth[(size_t)ind * mpad + (size_t)t * 64 + lane];
        const unsigned long long w = __ballot(zs_key(d, t * 64 + lane < m) == ZK_OVER);
        if (lane == 0) words[(size_t)blockIdx.y * ntiles + t] = w;
    }
}

__global__ __launch_bounds__(256) void zdeepgather_kernel(const ZInd *__restrict__ inds, const uchar2 *__restrict__ depth, int64_t m, int64_t mpad,
                                                          const unsigned long long *__restrict__ words, const uint32_t *__restrict__ off,
                                                          const int64_t *__restrict__ obase, int32_t *__restrict__ site_out,
                                                          int32_t *__restrict__ ad_out, float *__restrict__ g_out)
{
    const ZInd I = inds[blockIdx.y];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t ntiles = (m + 63) >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * ZS_TILES_PER_BLOCK;
    const int64_t ob = obase[blockIdx.y];
    for (int64_t t = t0 + wave; t < t0 + ZS_TILES_PER_BLOCK && t < ntiles; t += 4) {
        const unsigned long long w = words[(size_t)blockIdx.y * ntiles + t];
        if (!((w >> lane) & 1ull)) continue;
        const ZSite s = zs_load(I, depth, mpad, t, lane);
        const size_t pos = (size_t)ob + off[(size_t)blockIdx.y * ntiles + t] + (unsigned int)__popcll(w & ((1ull << lane) - 1ull));
        site_out[pos] = (int32_t)(t * 64 + lane);
        ad_out[2 * pos] = s.d.x;
        ad_out[2 * pos + 1] = s.d.y;
        g_out[2 * pos] = s.g0;
        g_out[2 * pos + 1] = s.g1;
    }
}

// The kept sites of a fit's current and previous frequencies, in site order, for the convergence chain (emMAF_cy.pyx:rmse1d over
// the rows of L[L_keep]): every fit has its own pair of vectors; what lies behind its kept count stays zero.
__global__ __launch_bounds__(256) void zcompact_kernel(const ZCompactJob *__restrict__ jobs, int64_t m, const unsigned long long *__restrict__ mask,
                                                       const uint32_t *__restrict__ off)
{
    const ZCompactJob J = jobs[blockIdx.y];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t ntiles = (m + 63) >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * ZS_TILES_PER_BLOCK;
    for (int64_t t = t0 + wave; t < t0 + ZS_TILES_PER_BLOCK && t < ntiles; t += 4) {
        const unsigned long long w = mask[(size_t)J.slot * ntiles + t];
        if (!((w >> lane) & 1ull)) continue;
        const size_t pos = (size_t)off[(size_t)J.slot * ntiles + t] + (unsigned int)__popcll(w & ((1ull << lane) - 1ull));
        J.a_out[pos] = J.cur[t * 64 + lane];
        J.b_out[pos] = J.prev[t * 64 + lane];
    }
}

// The host's (m, 2n) int32 rows into the device table [individual][site] of byte pairs; a count outside 0..255 raises the flag.
__global__ void zdepth_scatter_kernel(const int32_t *__restrict__ rows, int64_t nrows, int64_t n, int64_t row0, int64_t mpad,
                                      uchar2 *__restrict__ depth, int32_t *__restrict__ bad)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nrows * n) return;
    const int64_t r = e / n, i = e % n;
    const int32_t ar = rows[r * 2 * n + 2 * i], aa = rows[r * 2 * n + 2 * i + 1];
    if (ar < 0 || ar > 255 || aa < 0 || aa > 255) {
        atomicOr(bad, 1);
        return;
    }
    depth[(size_t)i * mpad + row0 + r] = make_uchar2((unsigned char)ar, (unsigned char)aa);
}

// ... and back: rows [row0, row0 + nrows) of the table as (nrows, 2n) int32 (a thread per pair; consecutive threads read consecutive
// sites of one individual)
__global__ void zdepth_gather_kernel(const uchar2 *__restrict__ depth, int64_t nrows, int64_t n, int64_t row0, int64_t mpad,
                                     int32_t *__restrict__ rows)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nrows * n) return;
    const int64_t i = e / nrows, r = e % nrows;
    const uchar2 v = depth[(size_t)i * mpad + row0 + r];
    rows[r * 2 * n + 2 * i] = v.x;
    rows[r * 2 * n + 2 * i + 1] = v.y;
}

// The selected sites' indices in ascending order (L_keep itself, for callers that want it).
__global__ __launch_bounds__(256) void zsites_kernel(int64_t m, const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ off,
                                                     int32_t *__restrict__ out)
{
    const int64_t ntiles = (m + 63) >> 6;
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < ntiles; t += (int64_t)gridDim.x * 4) {
        const unsigned long long w = mask[t];
        if ((w >> lane) & 1ull) out[off[t] + (unsigned int)__popcll(w & ((1ull << lane) - 1ull))] = (int32_t)(t * 64 + lane);
    }
}

// np.sum of a contiguous float32 array, continued from window to window: NumPy adds the sums of consecutive 8192-element chunks to a
// running float32 that starts at +0.0, and a full chunk is its pairwise routine's balanced tree over 64 leaves of 128 elements, a leaf
// being eight strided accumulators r[k] = a[k] + a[8 + k] + ... + a[120 + k] closed as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)).
// One workgroup per (chunk, individual, array).  The chunk is the elements [8192 c, 8192 (c + 1)) of the open chunk's `fill` elements
// followed by the window's array; it is staged through LDS with coalesced loads, leaf l at float offset 136 l: the eight floats of
// padding per leaf put the 32 lanes of a half-wave (4 leaves x 8 accumulators, stride 136 = 8 mod 32) on 32 distinct banks for every
// ds_read_b32 of the accumulator loop.  Thread <-> (leaf, accumulator) for two leaves, then 64 threads close the leaves and the fixed
// tree runs level by level.  Every add is one float32 rounding (the file is built without contraction; there is nothing to contract).
constexpr int ZSUM_LEAF_PITCH = 136;
__global__ __launch_bounds__(256) void zsum_chunk_kernel(const ZSumJob *__restrict__ jobs, float *__restrict__ csum)
{
    __shared__ float v[64 * ZSUM_LEAF_PITCH];
    __shared__ float r[512];
    const ZSumJob J = jobs[blockIdx.y];
    if ((int)blockIdx.x >= J.nfull) return;                 // (uniform over the workgroup)
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * WGS_ZSUM_CHUNK;
    for (int e = tid; e < WGS_ZSUM_CHUNK; e += 256) {
        const int64_t g = e0 + e;                           // < nfull * 8192 <= fill + k
        v[e + (e >> 7) * (ZSUM_LEAF_PITCH - 128)] = g < J.fill ? J.tail[g] : J.x[g - J.fill];
    }
    __syncthreads();
    for (int h = 0; h < 2; ++h) {
        const int leaf = (tid >> 3) + 32 * h, k = tid & 7;
        const float *p = v + leaf * ZSUM_LEAF_PITCH + k;
        float s = p[0];
        for (int i = 1; i < 16; ++i) s = s + p[8 * i];
        r[leaf * 8 + k] = s;
    }
    __syncthreads();
    float *node = v;                                        // (the staged chunk has been read)
    if (tid < 64) {
        const float *q = r + tid * 8;
        node[tid] = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    }
    __syncthreads();
    for (int w = 32; w >= 1; w >>= 1) {
        float s = 0.0f;
        if (tid < w) s = node[2 * tid] + node[2 * tid + 1];
        __syncthreads();
        if (tid < w) node[tid] = s;
        __syncthreads();
    }
    if (tid == 0) csum[J.cbase + blockIdx.x] = node[0];
}

// Behind the chunk sums, per (individual, array): the running value takes them serially in chunk order, and what the push leaves
// behind its last full chunk becomes the open chunk -- appended to the old one when the push closed none, else taken from the
// window's array alone (the old elements went into the first chunk, which zsum_chunk_kernel has read by now: stream order).
__global__ __launch_bounds__(256) void zsum_close_kernel(const ZSumJob *__restrict__ jobs, const float *__restrict__ csum)
{
    const ZSumJob J = jobs[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid == 0 && J.nfull > 0) {
        float s = *J.run;
        for (int c = 0; c < J.nfull; ++c) s = s + csum[J.cbase + c];
        *J.run = s;
    }
    if (J.nfull == 0) {
        for (int64_t e = tid; e < J.k; e += 256) J.tail[J.fill + e] = J.x[e];                 // fill + k < 8192
    } else {
        const int64_t src0 = (int64_t)J.nfull * WGS_ZSUM_CHUNK - J.fill;
        const int64_t left = J.fill + J.k - (int64_t)J.nfull * WGS_ZSUM_CHUNK;                // < 8192
        for (int64_t e = tid; e < left; e += 256) J.tail[e] = J.x[src0 + e];
    }
}

}  // namespace

int launch_zsum_push(wgs_ctx *ctx, const ZSumJob *d_jobs, int n_jobs, int max_full, float *csum)
{
    if (max_full > 0) hipLaunchKernelGGL(zsum_chunk_kernel, dim3(max_full, n_jobs), dim3(256), 0, ctx->stream, d_jobs, csum);
    hipLaunchKernelGGL(zsum_close_kernel, dim3(n_jobs), dim3(256), 0, ctx->stream, d_jobs, csum);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int zs_ensure_log_table(wgs_ctx *ctx)
{
    static std::atomic<unsigned long long> ready{0};      // one bit per device: the table lives in this code object's memory of each device
    if (ctx->device < 64 && ((ready.load() >> ctx->device) & 1ull)) return 0;
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(zs_log_table_dev), wgs_log_table_host, sizeof(double) * 2 * WGS_LOG_N));
    if (ctx->device < 64) ready.fetch_or(1ull << ctx->device);
    return 0;
}

static unsigned zs_blocks(int64_t m) { return (unsigned)((wgs_ntiles(m) + ZS_TILES_PER_BLOCK - 1) / ZS_TILES_PER_BLOCK); }

int launch_zclass(wgs_ctx *ctx, const ZInd *d_inds, int count, const uchar2 *depth, int64_t m, int64_t mpad, int32_t *cnt, float *sums,
                  int32_t *first, int32_t *over, bool carry)
{
    if (carry)
        hipLaunchKernelGGL(zclass_kernel<true>, dim3(count), dim3(256), 0, ctx->stream, d_inds, depth, m, mpad, cnt, sums, first, over);
    else
        hipLaunchKernelGGL(zclass_kernel<false>, dim3(count), dim3(256), 0, ctx->stream, d_inds, depth, m, mpad, cnt, sums, first, over);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_zmask(wgs_ctx *ctx, const ZInd *d_inds, int count, const uchar2 *depth, int64_t m, int64_t mpad, const float *kmean,
                 const int32_t *kcomp, const int32_t *dmap, const float *drows, unsigned long long *mask, uint32_t *off, int64_t *total)
{
    if (dmap)
        hipLaunchKernelGGL(zmask_kernel<true>, dim3(zs_blocks(m), count), dim3(256), 0, ctx->stream, d_inds, depth, m, mpad, kmean, kcomp, dmap,
                           drows, mask);
    else
        hipLaunchKernelGGL(zmask_kernel<false>, dim3(zs_blocks(m), count), dim3(256), 0, ctx->stream, d_inds, depth, m, mpad, kmean, kcomp, dmap,
                           drows, mask);
    hipLaunchKernelGGL(zscan_kernel, dim3(count), dim3(256), 0, ctx->stream, mask, wgs_ntiles(m), off, total);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_zstat(wgs_ctx *ctx, const ZInd *d_inds, int count, const uchar2 *depth, int64_t m, int64_t mpad, const float *tabs,
                 const float *const *fptr, const int32_t *dmap, const float *drows, const unsigned long long *mask, const uint32_t *off,
                 const int64_t *obase, float *wobs, float *wl, float *var)
{
    if (zs_ensure_log_table(ctx)) return 1;
    if (dmap)
        hipLaunchKernelGGL(zstat_kernel<true>, dim3(zs_blocks(m), count), dim3(256), 0, ctx->stream, d_inds, depth, m, mpad, tabs, fptr, dmap,
                           drows, mask, off, obase, wobs, wl, var);
    else
        hipLaunchKernelGGL(zstat_kernel<false>, dim3(zs_blocks(m), count), dim3(256), 0, ctx->stream, d_inds, depth, m, mpad, tabs, fptr, dmap,
                           drows, mask, off, obase, wobs, wl, var);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_zdeep_flag(wgs_ctx *ctx, const ZInd *d_inds, int count, const uchar2 *depth, int64_t m, int64_t mpad, unsigned long long *words,
                      uint32_t *off, int64_t *total)
{
    hipLaunchKernelGGL(zdeepflag_kernel, dim3(zs_blocks(m), count), dim3(256), 0, ctx->stream, d_inds, depth, m, mpad, words);
    hipLaunchKernelGGL(zscan_kernel, dim3(count), dim3(256), 0, ctx->stream, words, wgs_ntiles(m), off, total);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_zdeep_gather(wgs_ctx *ctx, const ZInd *d_inds, int count, const uchar2 *depth, int64_t m, int64_t mpad,
                        const unsigned long long *words, const uint32_t *off, const int64_t *obase, int32_t *site, int32_t *ad, float *g)
{
    hipLaunchKernelGGL(zdeepgather_kernel, dim3(zs_blocks(m), count), dim3(256), 0, ctx->stream, d_inds, depth, m, mpad, words, off, obase,
                       site, ad, g);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_zcompact(wgs_ctx *ctx, const ZCompactJob *d_jobs, int n_jobs, int64_t m, const unsigned long long *mask, const uint32_t *off)
{
    hipLaunchKernelGGL(zcompact_kernel, dim3(zs_blocks(m), n_jobs), dim3(256), 0, ctx->stream, d_jobs, m, mask, off);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_zdepth_scatter(wgs_ctx *ctx, const int32_t *d_rows, int64_t nrows, int64_t n, int64_t row0, int64_t mpad, uchar2 *depth, int32_t *bad)
{
    const int64_t total = nrows * n;
    hipLaunchKernelGGL(zdepth_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_rows, nrows, n, row0, mpad,
                       depth, bad);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_zdepth_gather(wgs_ctx *ctx, const uchar2 *depth, int64_t nrows, int64_t n, int64_t row0, int64_t mpad, int32_t *d_rows)
{
    const int64_t total = nrows * n;
    hipLaunchKernelGGL(zdepth_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, depth, nrows, n, row0, mpad, d_rows);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_zsites(wgs_ctx *ctx, int64_t m, const unsigned long long *mask, const uint32_t *off, int32_t *out)
{
    const int64_t blocks = (wgs_ntiles(m) + 3) / 4;
    hipLaunchKernelGGL(zsites_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, ctx->stream, m, mask, off, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
