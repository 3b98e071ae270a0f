// Device-side ingest: Beagle TEXT -> population slabs, tokenised on the MI355X.
//
// The reference parses every value on the host (reader_cy.pyx:52-66: strtok + atof per token); so did this
// library's reader until round 3 (reader.cpp: wgs_reader_next), which left the GPU idle for > 99 % of an
// end-to-end run at scale.  Here the host only inflates, finds the newlines and keeps the site names
// (reader.cpp: text_producer); the text itself goes to the device through page-locked buffers and
// `tokenise_kernel` does what strtok/atof did, writing each kept value at its place in the tile-interleaved slab
// (no row-major intermediate, no scatter pass):
//   * one wavefront per line; per step the 64 lanes take 64 consecutive 16-byte words (1 KiB, coalesced);
//   * a byte is a delimiter if it is one of "\t \n\r" (reader.cpp: is_delim); a token starts at a non-delimiter
//     that follows a delimiter; a wave-wide prefix sum of the per-lane start counts numbers the tokens of the
//     line, so every lane knows which (individual, GL) each of its tokens is: token 0 is the site name, 1-2 the
//     alleles (reader_cy.pyx:56-60), then of every triple the first two are kept and the third dropped (:62-66);
//   * a kept token is converted by the lane that holds its first byte, from registers (its word and the next):
//     ANGSD's "d.dddddd" by the eight-digit SWAR trick, any other plain decimal (optional sign, <= 15 significant
//     digits, optional exponent, net power of ten within +-22) by integer mantissa and ONE correctly rounded
//     double multiplication or division by an exact power of ten -- the correctly rounded value of the token,
//     i.e. what atof returns -- then (float), as reader_cy.pyx:66 stores it;
//   * anything else (inf/nan, hex, 16+ digits, tokens longer than 16 bytes, trailing junk), and a line with too
//     few columns, only FLAGS the line: the host re-parses flagged lines with the strtod-backed parser
//     (reader_text_parse_line) and uploads those rows -- none for ANGSD output.
// Bound: the host's inflate rate; the kernel reads 27 bytes of text and writes 8 bytes per (SNP, individual).
#include <string.h>
#include <sys/mman.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "reader_text.h"
#include "zscore.h"

size_t inflate_table_bytes(void);
constexpr size_t INFLATE_PAD = 128;   // bytes the compressed chunk is padded by on the device (inflate.hip reads a 24-byte window ahead)
int launch_inflate(wgs_ctx *ctx, const uint8_t *d_comp, const uint64_t *d_in_off, const uint32_t *d_in_len, const uint64_t *d_out_off,
                   const uint32_t *d_isize, uint8_t *d_out, uint8_t *d_status, void *d_tables, int32_t nblocks);

namespace {

__constant__ double kPow10Dev[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                     1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

struct TokArgs {
    const uint4 *text;             // the chunk, 16-byte aligned, padded with newlines
    const uint32_t *begin, *end;   // per line: [begin, end) in bytes
    const int32_t *dst;            // per line: row relative to row0, or -1 (site filtered out)
    uint8_t *flags;                // per line: 1 = the host must parse this line
    uint32_t *nflagged;            // optional: += lines flagged
    int64_t row0;                  // slab row of dst == 0
    int32_t nlines, n_inds;
    const int32_t *group_of, *col_of, *npairs;
    float4 *const *base;
};

// bit i = byte i of v is NOT one of '\t' '\n' '\r' ' '
__device__ __forceinline__ uint32_t nondelim4(uint32_t v)
{
    auto zero_bytes = [](uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); };   // 0x80 per zero byte
    const uint32_t d = zero_bytes(v ^ 0x09090909u) | zero_bytes(v ^ 0x0A0A0A0Au) | zero_bytes(v ^ 0x0D0D0D0Du) | zero_bytes(v ^ 0x20202020u);
    return ((((d >> 7) * 0x01020408u) >> 24) & 0xFu) ^ 0xFu;
}
__device__ __forceinline__ uint32_t nondelim16(const uint4 &x)
{
    return nondelim4(x.x) | (nondelim4(x.y) << 4) | (nondelim4(x.z) << 8) | (nondelim4(x.w) << 12);
}

// The token of `len` (1..16) bytes held in lo (bytes 0-7) and hi (8-15), first character in the lowest byte.
// Returns false when the host has to convert it (see the file comment).
__device__ __forceinline__ bool parse_token(uint64_t lo, uint64_t hi, int len, float *out)
{
    if (len == 8) {                                            // "d.dddddd" (reader.cpp: parse_f6)
        uint64_t d = lo ^ 0x3030303030302E30ull;
        if (!((((d + 0x7676767676767676ull) | d) & 0x8080808080808080ull) || (d & 0xFF00ull))) {
            d = (d >> 8) | (d & 0xFF);
            d = d * 10 + (d >> 8);
            const uint64_t mask = 0x000000FF000000FFull;
            d = (((d & mask) * (100 + (1000000ull << 32))) + (((d >> 16) & mask) * (1 + (10000ull << 32)))) >> 32;
            *out = (float)((double)(uint32_t)d / 1e7);
            return true;
        }
    }
    auto at = [&](int i) { return (uint32_t)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xFF); };
    int i = 0;
    bool neg = false;
    uint32_t c = at(0);
    if (c == '-' || c == '+') {
        neg = c == '-';
        i = 1;
    }
    uint64_t mant = 0;
    int digits = 0, frac = 0, seen = 0;
    bool dot = false;
    for (; i < len; ++i) {
        c = at(i);
        if (c >= '0' && c <= '9') {
            ++seen;
            if (mant == 0 && c == '0') {
                if (dot) ++frac;
                continue;
            }
            if (++digits > 15) return false;
            mant = mant * 10 + (uint64_t)(c - '0');
            if (dot) ++frac;
        } else if (c == '.' && !dot) {
            dot = true;
        } else {
            break;
        }
    }
    if (seen == 0) return false;
    int ex = 0;
    if (i < len) {
        if (c != 'e' && c != 'E') return false;
        ++i;
        bool xneg = false;
        if (i < len && (at(i) == '-' || at(i) == '+')) xneg = at(i++) == '-';
        int xd = 0;
        for (; i < len && at(i) >= '0' && at(i) <= '9' && xd < 4; ++i, ++xd) ex = ex * 10 + (int)(at(i) - '0');
        if (xd == 0 || xd > 3 || i < len) return false;
        if (xneg) ex = -ex;
    }
    const int net = ex - frac;
    if (net < -22 || net > 22) return false;
    const double v = net < 0 ? (double)mant / kPow10Dev[-net] : (double)mant * kPow10Dev[net];
    *out = (float)(neg ? -v : v);
    return true;
}

__global__ __launch_bounds__(256) void tokenise_kernel(TokArgs a)
{
    const int lane = threadIdx.x & 63;
    const int line = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (line >= a.nlines) return;                              // whole waves leave together
    const int32_t rel = a.dst[line];
    if (rel < 0) return;
    const uint32_t b = a.begin[line], e = a.end[line];
    const int64_t row = a.row0 + rel;
    const uint32_t need = 3u + 3u * (uint32_t)a.n_inds;
    const uint32_t w0 = b >> 4, w1 = (e + 15u) >> 4;           // the 16-byte words that hold the line
    uint32_t tok = 0;                                          // tokens that start before this step's words
    uint32_t prev_nd = 0;                                      // the byte before this step's words is a non-delimiter
    bool bad = false;
    for (uint32_t wb = w0; wb < w1 && tok < need; wb += 64) {
        const uint32_t w = wb + (uint32_t)lane;
        uint4 x = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au), y = x;
        if (w < w1) {
            x = a.text[w];
            y = a.text[w + 1];                                 // in bounds: the buffer is padded by TEXT_PAD bytes
        }
        uint32_t nd = nondelim16(x) | (nondelim16(y) << 16);
        // bytes outside [b, e) count as delimiters: bit i is byte 16 w + i
        const int64_t first = (int64_t)b - (int64_t)w * 16, last = (int64_t)e - (int64_t)w * 16;
        if (first > 0) nd &= first >= 32 ? 0u : ~0u << first;
        if (last < 32) nd &= last <= 0 ? 0u : ~0u >> (32 - last);
        const uint32_t own = nd & 0xFFFFu;
        uint32_t before = (uint32_t)__shfl_up((int)(own >> 15), 1);
        if (lane == 0) before = prev_nd;
        uint32_t starts = own & ~((own << 1) | before);
        const int cnt = __popc(starts);
        int incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        uint32_t k = tok + (uint32_t)(incl - cnt);
        while (starts) {
            const int bit = __ffs((int)starts) - 1;
            starts &= starts - 1;
            if (k >= 3 && k < need) {
                const uint32_t j = k - 3, ind = j / 3, which = j - ind * 3;
                if (which < 2) {
                    const uint32_t inv = ~(nd >> bit);
                    const int len = inv ? __ffs((int)inv) - 1 : 32;        // non-delimiters from `bit` on
                    float v = 0.0f;
                    bool ok = bit + len < 32 && len <= 16;                 // the token ends inside the two words
                    if (ok) {
                        const uint64_t q0 = x.x | ((uint64_t)x.y << 32), q1 = x.z | ((uint64_t)x.w << 32);
                        const uint64_t q2 = y.x | ((uint64_t)y.y << 32), q3 = y.z | ((uint64_t)y.w << 32);
                        const uint64_t A = bit & 8 ? q1 : q0, B = bit & 8 ? q2 : q1, C = bit & 8 ? q3 : q2;
                        const int s = (bit & 7) * 8;
                        const uint64_t lo = s ? (A >> s) | (B << (64 - s)) : A, hi = s ? (B >> s) | (C << (64 - s)) : B;
                        ok = parse_token(lo, hi, len, &v);
                    }
                    if (ok) {
                        const int g = a.group_of[ind], col = a.col_of[ind];
                        const int64_t at = ((((row >> 6) * a.npairs[g] + (col >> 1)) << 6) + (row & 63)) * 4 + (col & 1) * 2 + (int)which;
                        reinterpret_cast<float *>(a.base[g])[at] = v;
                    } else {
                        bad = true;
                    }
                }
            }
            ++k;
        }
        tok += (uint32_t)__shfl(incl, 63);
        prev_nd = (uint32_t)__shfl((int)(own >> 15), 63);
    }
    if (tok < need) bad = true;                                // too few columns: the host reports the line
    const bool any_bad = __any(bad);
    if (lane == 0) {
        a.flags[line] = any_bad ? 1 : 0;
        if (any_bad && a.nflagged) atomicAdd(a.nflagged, 1u);
    }
}

// ---- integer tables: allele depths (--ind_ad_file) and ANGSD counts into the depth table [individual][site] of byte pairs ------------
// Same hand-over and token numbering as tokenise_kernel (one wavefront per line, 1 KiB per step, wave-wide prefix sum of the token
// starts), but a line is one SITE and each of its n pairs belongs to another row of the table, mpad pairs apart: stored directly,
// every pair would be a 2-byte store at a stride of 2 mpad bytes.  So a workgroup takes a TILE of 64 consecutive lines (16 per
// wavefront) times a STRIP of DEPTH_STRIP individuals, collects the pairs in LDS as [individual][line] and then stores per
// individual the 64 sites of the tile side by side: 128 bytes per wavefront store, what zclass_kernel reads per wavefront.
//   * pairs  (tpi = 2): individual i of a line owns tokens 2i, 2i + 1;
//   * counts (tpi = 4): tokens 4i .. 4i + 3 (A, C, G, T reads); the pair is (token 4i + major, token 4i + minor) with the
//     site's selectors from sel[row][2] -- np.take_along_axis in the reference's allele_counts_beagle.py.
// LDS: a row of the tile is 64 pairs + 2 of padding = 33 dwords, so the tokens of one step -- consecutive individuals, one line --
// fall into different banks, and the read-out of a row is 64 consecutive 2-byte words.  256 individuals x 132 bytes = 33 KiB: four
// workgroups per CU.  More than DEPTH_STRIP individuals: the strips follow one another inside the workgroup; per line the step
// where the strip ended is kept in LDS and taken up again (that step's 1 KiB is read twice, nothing else).
// The kernel converts runs of 1-3 digits with value <= 255; any other token among those it owns, or too few of them, flags the
// line, whose pairs are not stored (in the strip where the flag is raised and the strips after it; the host parses a flagged line
// and either uploads its whole row or refuses the file).  dst = -1: the line has no row and is not looked at; dst = DEPTH_CHECK_ONLY:
// no row either, but its tokens are read and a bad one flags it (a data line before the row range of a SNP shard).
constexpr int DEPTH_STRIP = 256, DEPTH_ROW = 132;
constexpr int32_t DEPTH_CHECK_ONLY = -2;

struct DepthTokArgs {
    const uint4 *text;
    const uint32_t *begin, *end;
    const int32_t *dst;
    uint8_t *flags;
    uint32_t *nflagged;
    int64_t row0;
    int32_t nlines, n_inds, tpi;
    const uint8_t *sel;            // counts: [site][2] selectors 0..3 (checked on the host)
    uchar2 *table;
    int64_t mpad;
};

__global__ __launch_bounds__(256) void depth_tokenise_kernel(DepthTokArgs a)
{
    __shared__ __attribute__((aligned(4))) uint8_t tile[DEPTH_STRIP * DEPTH_ROW];
    __shared__ uint32_t s_wb[64], s_tok[64], s_prev[64];
    __shared__ int32_t s_rel[64];
    __shared__ uint8_t s_bad[64], s_major[64], s_minor[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int line0 = (int)blockIdx.x * 64;
    if (threadIdx.x < 64) {
        const int l = line0 + (int)threadIdx.x;
        const int32_t rel = l < a.nlines ? a.dst[l] : -1;
        s_rel[threadIdx.x] = rel;
        s_wb[threadIdx.x] = rel != -1 ? a.begin[l] >> 4 : 0u;
        s_tok[threadIdx.x] = 0;
        s_prev[threadIdx.x] = 0;
        s_bad[threadIdx.x] = 0;
        s_major[threadIdx.x] = a.sel && rel >= 0 ? a.sel[(a.row0 + rel) * 2] & 3 : 0;
        s_minor[threadIdx.x] = a.sel && rel >= 0 ? a.sel[(a.row0 + rel) * 2 + 1] & 3 : 1;
    }
    __syncthreads();
    const uint32_t tpi = (uint32_t)a.tpi;
    for (int strip0 = 0; strip0 < a.n_inds; strip0 += DEPTH_STRIP) {
        const int strip_n = min(DEPTH_STRIP, a.n_inds - strip0);
        const uint32_t tok_lo = (uint32_t)strip0 * tpi, tok_hi = (uint32_t)(strip0 + strip_n) * tpi;
        for (int q = 0; q < 16; ++q) {
            const int li = wave * 16 + q;
            if (s_rel[li] == -1 || s_bad[li]) continue;        // (the same for the whole wavefront)
            const uint32_t b = a.begin[line0 + li], e = a.end[line0 + li];
            const uint32_t w1 = (e + 15u) >> 4;
            uint32_t wb = s_wb[li], tok = s_tok[li], prev_nd = s_prev[li];
            const uint32_t major = s_major[li], minor = s_minor[li];
            bool bad = false, enough = false;
            while (wb < w1 && !enough) {
                const uint32_t w = wb + (uint32_t)lane;
                uint4 x = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au), y = x;
                if (w < w1) {
                    x = a.text[w];
                    y = a.text[w + 1];                         // in bounds: the buffer is padded by TEXT_PAD bytes
                }
                uint32_t nd = nondelim16(x) | (nondelim16(y) << 16);
                const int64_t first = (int64_t)b - (int64_t)w * 16, last = (int64_t)e - (int64_t)w * 16;
                if (first > 0) nd &= first >= 32 ? 0u : ~0u << first;
                if (last < 32) nd &= last <= 0 ? 0u : ~0u >> (32 - last);
                const uint32_t own = nd & 0xFFFFu;
                uint32_t before = (uint32_t)__shfl_up((int)(own >> 15), 1);
                if (lane == 0) before = prev_nd;
                uint32_t starts = own & ~((own << 1) | before);
                const int cnt = __popc(starts);
                int incl = cnt;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int up = __shfl_up(incl, off);
                    if (lane >= off) incl += up;
                }
                const uint64_t lo64 = x.x | ((uint64_t)x.y << 32), hi64 = x.z | ((uint64_t)x.w << 32);
                uint32_t k = tok + (uint32_t)(incl - cnt);
                while (starts) {
                    const int bit = __ffs((int)starts) - 1;
                    starts &= starts - 1;
                    if (k >= tok_lo && k < tok_hi) {
                        const uint32_t inv = ~(nd >> bit);
                        const int len = inv ? __ffs((int)inv) - 1 : 32;
                        // the token's first four bytes (it starts in this lane's word; bytes 16.. come from the next word)
                        const uint64_t A = bit & 8 ? hi64 : lo64, B = bit & 8 ? (uint64_t)y.x : hi64;
                        const int sh = (bit & 7) * 8;
                        const uint32_t c4 = (uint32_t)(sh ? (A >> sh) | (B << (64 - sh)) : A);
                        const uint32_t d0 = (c4 & 0xFFu) - '0', d1 = ((c4 >> 8) & 0xFFu) - '0', d2 = ((c4 >> 16) & 0xFFu) - '0';
                        uint32_t v = 256;
                        if (len == 1 && d0 <= 9) v = d0;
                        else if (len == 2 && d0 <= 9 && d1 <= 9) v = d0 * 10 + d1;
                        else if (len == 3 && d0 <= 9 && d1 <= 9 && d2 <= 9) v = d0 * 100 + d1 * 10 + d2;
                        if (v <= 255) {
                            const uint32_t j = k - tok_lo, ind = j / tpi, which = j - ind * tpi;
                            uint8_t *cell = tile + ind * DEPTH_ROW + li * 2;
                            if (tpi == 2) {
                                cell[which] = (uint8_t)v;
                            } else {
                                if (which == major) cell[0] = (uint8_t)v;
                                if (which == minor) cell[1] = (uint8_t)v;
                            }
                        } else {
                            bad = true;
                        }
                    }
                    ++k;
                }
                const uint32_t total = (uint32_t)__shfl(incl, 63);
                enough = tok + total >= tok_hi;
                if (tok + total > tok_hi && strip0 + strip_n < a.n_inds) break;     // the next strip starts inside this step: taken up there
                tok += total;
                prev_nd = (uint32_t)__shfl((int)(own >> 15), 63);
                wb += 64;
            }
            if (!enough) bad = true;                           // too few columns
            const bool any_bad = __any(bad);
            if (lane == 0) {
                s_wb[li] = wb;
                s_tok[li] = tok;
                s_prev[li] = prev_nd;
                if (any_bad) s_bad[li] = 1;
            }
        }
        __syncthreads();
        const int32_t rel = s_rel[lane];
        if (rel >= 0 && !s_bad[lane]) {
            uchar2 *out = a.table + a.row0 + rel;
            for (int ind = wave; ind < strip_n; ind += 4)
                out[(int64_t)(strip0 + ind) * a.mpad] = *reinterpret_cast<const uchar2 *>(tile + ind * DEPTH_ROW + lane * 2);
        }
        __syncthreads();
    }
    if (threadIdx.x < 64 && s_rel[threadIdx.x] != -1 && s_bad[threadIdx.x]) {
        a.flags[line0 + (int)threadIdx.x] = 1;
        if (a.nflagged) atomicAdd(a.nflagged, 1u);
    }
}

// ---- line listing on the device (BGZF members inflated there: the text never exists on the host) -----------------------
// What reader.cpp: list_lines does with memchr on the host: the positions of the newlines (count per 4 KiB block, scan,
// write), then per line its extent, whether it is blank, and its first token (the site name); exclusive scans number the
// non-blank lines and place the names in one blob.  T_* index the totals the host reads back.
enum { T_NEWLINES = 0, T_NONBLANK = 1, T_NAME_BYTES = 2, T_TAIL = 3, T_NAME_CUT = 4, T_FLAGGED = 5, T_COUNT = 8 };

__device__ __forceinline__ uint32_t newline_mask16(const uint4 &x)
{
    auto m4 = [](uint32_t v) {
        const uint32_t y = v ^ 0x0A0A0A0Au;
        const uint32_t z = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);       // 0x80 per newline
        return (((z >> 7) * 0x01020408u) >> 24) & 0xFu;
    };
    return m4(x.x) | (m4(x.y) << 4) | (m4(x.z) << 8) | (m4(x.w) << 12);
}

// this thread's 16 bytes of text[0 .. total): bit i = byte i is a newline
__device__ __forceinline__ uint32_t newline_bits(const uint4 *text, uint64_t total, uint64_t word)
{
    if (word * 16 >= total) return 0;
    uint32_t m = newline_mask16(text[word]);
    const uint64_t left = total - word * 16;
    if (left < 16) m &= (1u << left) - 1u;
    return m;
}

__global__ __launch_bounds__(256) void count_newlines_kernel(const uint4 *text, uint64_t total, uint32_t *counts)
{
    __shared__ uint32_t part[4];
    const uint64_t word = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t c = (uint32_t)__popc(newline_bits(text, total, word));
#pragma unroll
    for (int off = 32; off; off >>= 1) c += (uint32_t)__shfl_down((int)c, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void write_newlines_kernel(const uint4 *text, uint64_t total, const uint32_t *offsets, uint32_t *nl_pos)
{
    __shared__ uint32_t part[4];
    const uint64_t word = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t m = newline_bits(text, total, word);
    const uint32_t c = (uint32_t)__popc(m);
    uint32_t incl = c;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
        if (lane >= off) incl += up;
    }
    if (lane == 63) part[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t at = offsets[blockIdx.x] + incl - c;
    for (unsigned w = 0; w < (threadIdx.x >> 6); ++w) at += part[w];
    while (m) {
        const int bit = __ffs((int)m) - 1;
        m &= m - 1;
        nl_pos[at++] = (uint32_t)(word * 16 + (uint64_t)bit);
    }
}

// out[i] = in[0] + ... + in[i-1]; *total = the whole sum (one workgroup: the arrays are small next to the text)
__global__ __launch_bounds__(1024) void scan_u32_kernel(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *total)
{
    __shared__ uint32_t part[16];
    __shared__ uint32_t carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 4096) {
        const uint32_t i0 = base + threadIdx.x * 4;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? in[i0 + k] : 0u;
        const uint32_t mine = v[0] + v[1] + v[2] + v[3];
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        uint32_t at = carry_s + incl - mine;
        for (int w = 0; w < wave; ++w) at += part[w];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < n) out[i0 + k] = at;
            at += v[k];
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = at;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}

__device__ __forceinline__ bool is_delim_dev(uint8_t c) { return c == '\t' || c == ' ' || c == '\n' || c == '\r'; }

struct LineArgs {
    const uint8_t *text;
    const uint32_t *nl_pos;
    uint32_t nlines;               // newline-terminated lines of the chunk (blank ones included)
    uint32_t *begin, *end;         // per line: [begin, end) without the newline
    uint32_t *nonblank;            // 1 = a data row
    uint32_t *name_start, *name_len1;   // first token; its length + 1 (0 for blank lines)
    uint32_t *totals;
    int32_t table;                 // an integer table: a line that starts with '#' is no row (np.loadtxt)
};

__global__ __launch_bounds__(256) void line_info_kernel(LineArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.nlines) return;
    const uint32_t b = i ? a.nl_pos[i - 1] + 1u : 0u, e = a.nl_pos[i];
    uint32_t q = b;
    while (q < e && is_delim_dev(a.text[q])) ++q;
    uint32_t x = q;
    while (x < e && !is_delim_dev(a.text[x])) ++x;
    a.begin[i] = b;
    a.end[i] = e;
    const bool row = q < e && !(a.table && a.text[q] == '#');
    a.nonblank[i] = row ? 1u : 0u;
    a.name_start[i] = q;
    a.name_len1[i] = !row ? 0u : a.table ? 1u : x - q + 1u;      // (a table has no names: one newline per row)
    if (i == a.nlines - 1) a.totals[T_TAIL] = e + 1u;          // where the partial last line starts
}

struct DstArgs {
    uint32_t nlines, take;         // rows of this chunk: the first `take` non-blank lines
    const uint32_t *nonblank, *rank, *name_start, *name_len1, *name_off;
    const int32_t *dstmap;         // optional, per rank: the row (relative to row0) or -1 = the site is filtered out
    const uint8_t *text;
    int32_t *dst;
    uint8_t *names;
    uint32_t *totals;
};

__global__ __launch_bounds__(256) void dst_names_kernel(DstArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.nlines) return;
    const bool row = a.nonblank[i] != 0;
    const uint32_t r = a.rank[i];
    if (row && r == a.take) a.totals[T_NAME_CUT] = a.name_off[i];   // the row limit cuts the chunk here
    if (!row || r >= a.take) {
        a.dst[i] = -1;
        return;
    }
    a.dst[i] = a.dstmap ? a.dstmap[r] : (int32_t)r;
    const uint32_t n = a.name_len1[i] - 1u;
    const uint8_t *src = a.text + a.name_start[i];
    uint8_t *out = a.names + a.name_off[i];
    for (uint32_t k = 0; k < n; ++k) out[k] = src[k];
    out[n] = '\n';
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Page-locked staging.  hipHostMalloc takes 0.18 s per GB on this platform and hipHostFree 0.1 s (tools/ubench_pin.hip: 48 and
// 28 ms for the 272 MB of bench.py's ingest leg -- half of that leg's time); anonymous memory in transparent huge pages, faulted
// in by a few threads and then registered, takes 4 ms for the same 272 MB and copies to the device at the same 57 GB/s.  Without
// huge pages (the kernel's setting) it is 4 KiB pages as before, still three times cheaper; what mmap or the registration
// refuses falls back to hipHostMalloc.  The pages go back to the system on a thread of their own (munmap: 12-20 ms).
struct PinnedBlock {
    void *raw = nullptr;          // nullptr: from hipHostMalloc
    size_t raw_bytes = 0;
};
std::mutex g_pinned_mu;
std::unordered_map<void *, PinnedBlock> g_pinned;

void *pinned_alloc(size_t bytes, void *user)                  // called from the producer thread too
{
    if (hipSetDevice((int)(intptr_t)user) != hipSuccess) return nullptr;
    const size_t huge = (size_t)2 << 20;
    if (bytes >= 4 * huge) {
        const size_t len = (bytes + huge - 1) & ~(huge - 1);
        void *raw = mmap(nullptr, len + huge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (raw != MAP_FAILED) {
            char *p = reinterpret_cast<char *>(((uintptr_t)raw + huge - 1) & ~(uintptr_t)(huge - 1));
            (void)madvise(p, len, MADV_HUGEPAGE);
            const int T = (int)std::max<size_t>(1, std::min<size_t>(8, std::min<size_t>(std::thread::hardware_concurrency(), len / (16 * huge))));
            std::vector<std::thread> th;
            for (int t = 1; t < T; ++t)
                th.emplace_back([=] {
                    for (size_t i = len * (size_t)t / (size_t)T; i < len * (size_t)(t + 1) / (size_t)T; i += 4096) p[i] = 0;
                });
            for (size_t i = 0; i < len / (size_t)T; i += 4096) p[i] = 0;
            for (auto &x : th) x.join();
            if (hipHostRegister(p, len, hipHostRegisterDefault) == hipSuccess) {
                std::lock_guard<std::mutex> lk(g_pinned_mu);
                g_pinned[p] = PinnedBlock{raw, len + huge};
                return p;
            }
            (void)hipGetLastError();
            munmap(raw, len + huge);
        }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    g_pinned[p] = PinnedBlock{};
    return p;
}
void pinned_release(void *p, void *)
{
    if (!p) return;
    PinnedBlock blk;
    {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        auto it = g_pinned.find(p);
        if (it == g_pinned.end()) return;
        blk = it->second;
        g_pinned.erase(it);
    }
    if (!blk.raw) {
        (void)hipHostFree(p);
        return;
    }
    (void)hipHostUnregister(p);
    std::thread([blk] { munmap(blk.raw, blk.raw_bytes); }).detach();
}


// A device array that only grows, owned by the object it is a member of.  reserve() is the one way to more room: it waits for the
// stream (kernels in flight may still read the old array), frees, allocates (wgs_malloc: common.h on what that can cost) and
// leaves the capacity at 0 when that fails, so that no later call trusts an array that is gone.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;                 // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    // Room for `count` elements; where that takes a new array it has `new_cap` of them, and the first keep_bytes of the old one.
    int reserve(hipStream_t st, size_t count, size_t new_cap, size_t keep_bytes = 0)
    {
        if (count <= cap) return 0;
        cap = 0;
        HIP_TRY(hipStreamSynchronize(st));
        T *old = p;
        p = nullptr;
        if (old && !keep_bytes) HIP_TRY(hipFree(old));           // first: the old and the new array need not fit side by side
        const hipError_t made = wgs_malloc(&p, new_cap * sizeof(T));
        const hipError_t kept = made == hipSuccess && keep_bytes ? hipMemcpy(p, old, keep_bytes, hipMemcpyDeviceToDevice) : hipSuccess;
        if (keep_bytes) (void)hipFree(old);
        HIP_TRY(made);
        HIP_TRY(kept);
        cap = new_cap;
        return 0;
    }
};

// Arrays that grow together, to one capacity.
template <class... B>
int reserve_all(hipStream_t st, size_t count, size_t new_cap, B &...bufs)
{
    int rc = 0;
    ((rc = rc ? rc : bufs.reserve(st, count, new_cap)), ...);
    return rc;
}

}  // namespace

struct wgs_ingest {
    wgs_beagle *b = nullptr;        // the matrix the lines go to, or ...
    wgs_depth *depth = nullptr;     // ... the depth table (wgs_depth_ingest_*: an integer table through the same hand-overs)
    wgs_ctx *ctx = nullptr;
    int64_t m_rows = 0;             // rows of the target
    struct {                        // what only the depth table's ingest uses
        int32_t tpi = 2;                // tokens per individual (2: pairs, 4: ANGSD counts)
        DevBuf<uint8_t> sel;            // counts: the sites' (major, minor) selectors
        std::vector<int32_t> irows;     // host-parsed row of a flagged line
        int64_t lines_before = 0;       // device-resident: lines of the text in the chunks before this one
        size_t host_peak = 0;           // largest host buffer this object allocated itself
        bool overflow = false;          // the file has more data lines than the table rows
        bool ranged = false;            // wgs_depth_ingest_set_first_row: the table holds the file's rows [first_row, first_row + m_rows)
        int64_t before = 0;             // ... data lines still to come before that range: checked, no row
        double tok_ms = 0.0;            // the tokeniser kernel alone (WGSASSIGN_INGEST_TIME_KERNEL=1)
        hipEvent_t kev0 = nullptr, kev1 = nullptr;
    } dp;
    wgs_reader *r = nullptr;
    DevBuf<uint8_t> d_text;
    DevBuf<uint32_t> d_begin, d_end;                         // per line (ensure_line_arrays)
    DevBuf<int32_t> d_dst;
    DevBuf<uint8_t> d_flags;
    std::vector<int32_t> dst;
    std::vector<uint8_t> flags;
    std::vector<float> rows;        // host-parsed rows of flagged lines
    std::string names;              // site names of the last chunk
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // statistics
    double wait_s = 0.0, inflate_s = 0.0, scan_s = 0.0, device_ms = 0.0;
    int64_t host_lines = 0, text_bytes = 0, lines = 0, chunks = 0;
    // ---- BGZF: the device-resident pipeline (compressed members in, slab rows out; see wgs_ingest_next) ----
    bool resident = false, done = false;
    int64_t limit = -1, rows_done = 0;
    size_t carry = 0;               // d_text[0 .. carry) = the partial last line of the previous chunk
    DevBuf<uint8_t> d_carry, d_comp;
    DevBuf<uint64_t> d_in_off, d_out_off;                    // per member, as are the next three
    DevBuf<uint32_t> d_in_len, d_isize;
    DevBuf<uint8_t> d_status, d_tables;
    DevBuf<uint32_t> d_counts, d_offsets;                    // newlines per 4 KiB of text, and their exclusive scan
    DevBuf<uint32_t> d_nl_pos, d_nonblank, d_rank, d_name_start, d_name_len1, d_name_off;    // per line, as is the next
    DevBuf<int32_t> d_dstmap;
    DevBuf<uint8_t> d_names;
    DevBuf<uint32_t> d_totals;
    uint32_t *h_totals = nullptr;
    std::vector<uint64_t> out_off;
    std::vector<uint8_t> status;
    std::vector<int32_t> dstmap;
    std::vector<uint32_t> h_begin, h_end, h_rank;
    std::vector<char> line;
    hipEvent_t iev0 = nullptr, iev1 = nullptr;
    double inflate_kernel_ms = 0.0, read_s = 0.0, create_s = 0.0, next_s = 0.0;
    int64_t blocks_inflated = 0, blocks_host = 0;
};

namespace {

int ensure_line_arrays(wgs_ingest *g, size_t nl)
{
    hipStream_t st = g->ctx->stream;
    const size_t cap = nl + nl / 2 + 1024;
    if (int rc = reserve_all(st, nl, cap, g->d_begin, g->d_end, g->d_dst, g->d_flags)) return rc;
    if (!g->resident) return 0;
    return reserve_all(st, nl, cap, g->d_nl_pos, g->d_nonblank, g->d_rank, g->d_name_start, g->d_name_len1, g->d_name_off, g->d_dstmap);
}

// device_ms: from clock_start to the end of what the chunk has put on the stream by clock_stop, which waits for it.
int clock_start(wgs_ingest *g)
{
    HIP_TRY(hipEventRecord(g->ev0, g->ctx->stream));
    return 0;
}
int clock_stop(wgs_ingest *g)
{
    HIP_TRY(hipEventRecord(g->ev1, g->ctx->stream));
    HIP_TRY(hipStreamSynchronize(g->ctx->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, g->ev0, g->ev1));
    g->device_ms += ms;
    return 0;
}

// Rows for the n data lines of a chunk: line i goes to row0 + its number among the lines `keep` keeps (keep == NULL: all), which
// is what *map receives where one is asked for (-1: no row); *written = the rows taken.
int place_rows(wgs_ingest *g, int64_t row0, const uint8_t *keep, int64_t keep_len, size_t n, std::vector<int32_t> *map, int64_t *written)
{
    if (keep) WGS_REQUIRE((int64_t)n <= keep_len, "site mask shorter than the file (%lld lines left in it, %lld in the chunk)", (long long)keep_len, (long long)n);
    if (g->dp.ranged) {
        // a row range of the file: lines before it are checked and take no row, the next m_rows - row0 fill the table, the rest
        // is counted only -- the caller compares the total with the whole file's rows
        WGS_REQUIRE(map && row0 >= 0 && row0 <= g->m_rows, "row %lld outside the device table (%lld rows)", (long long)row0, (long long)g->m_rows);
        map->resize(n);
        *written = 0;
        for (size_t i = 0; i < n; ++i) {
            if (g->dp.before > 0) {
                (*map)[i] = DEPTH_CHECK_ONLY;
                --g->dp.before;
            } else {
                (*map)[i] = row0 + *written < g->m_rows ? (int32_t)(*written)++ : -1;
            }
        }
        return 0;
    }
    *written = (int64_t)n;
    if (map) {
        map->resize(n);
        *written = 0;
        for (size_t i = 0; i < n; ++i) (*map)[i] = (!keep || keep[i]) ? (int32_t)(*written)++ : -1;
    }
    // a table with more data lines than the target has rows: nothing more is stored, the lines are still counted (the caller
    // reports both numbers)
    if (g->depth && row0 + *written > g->m_rows) g->dp.overflow = true;
    if (g->dp.overflow) {
        if (map) std::fill(map->begin(), map->end(), -1);
        *written = 0;
    }
    WGS_REQUIRE(row0 >= 0 && row0 + *written <= g->m_rows, "rows [%lld, %lld) outside the device matrix (%lld rows)", (long long)row0,
                (long long)(row0 + *written), (long long)g->m_rows);
    return 0;
}

// The tokeniser of the target over the nl lines listed in d_begin / d_end / d_dst; flags what it leaves to the host's parser.
int launch_tokenise(wgs_ingest *g, const void *text, int64_t row0, size_t nl, uint32_t *nflagged)
{
    hipStream_t st = g->ctx->stream;
    HIP_TRY(hipMemsetAsync(g->d_flags.p, 0, nl, st));
    auto lines = [&](auto &a, int64_t n_inds) {               // what the two kernels' arguments have in common
        a.text = reinterpret_cast<const uint4 *>(text);
        a.begin = g->d_begin.p;
        a.end = g->d_end.p;
        a.dst = g->d_dst.p;
        a.flags = g->d_flags.p;
        a.nflagged = nflagged;
        a.row0 = row0;
        a.nlines = (int32_t)nl;
        a.n_inds = (int32_t)n_inds;
    };
    if (g->depth) {
        DepthTokArgs d;
        lines(d, g->depth->n);
        d.tpi = g->dp.tpi;
        d.sel = g->dp.sel.p;
        d.table = g->depth->table;
        d.mpad = g->depth->mpad;
        static const bool timed = getenv("WGSASSIGN_INGEST_TIME_KERNEL") != nullptr;
        hipEvent_t &kev0 = g->dp.kev0, &kev1 = g->dp.kev1;
        if (timed && !kev0 && (hipEventCreate(&kev0) != hipSuccess || hipEventCreate(&kev1) != hipSuccess)) kev0 = kev1 = nullptr;
        if (timed && kev1) (void)hipEventRecord(kev0, st);
        hipLaunchKernelGGL(depth_tokenise_kernel, dim3((unsigned)((nl + 63) / 64)), dim3(256), 0, st, d);
        if (timed && kev1) {
            float ms = 0.0f;
            (void)hipEventRecord(kev1, st);
            if (hipEventSynchronize(kev1) == hipSuccess && hipEventElapsedTime(&ms, kev0, kev1) == hipSuccess) g->dp.tok_ms += ms;
        }
    } else {
        wgs_beagle *b = g->b;
        TokArgs a;
        lines(a, b->n);
        a.group_of = b->d_group_of;
        a.col_of = b->d_col_of;
        a.npairs = b->d_npairs;
        a.base = b->d_base;
        hipLaunchKernelGGL(tokenise_kernel, dim3((unsigned)((nl + 3) / 4)), dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// parse_flagged for an integer table: a line by np.loadtxt's rules (reader_table_parse_line); its pairs are picked as the kernel
// picks them and the row goes through wgs_depth_upload_rows, which refuses counts outside 0..255.  Messages name the line's
// 1-based number in the file.
template <class TextOf, class LineOf>
int parse_flagged_table(wgs_ingest *g, int64_t row0, size_t nl, TextOf text_of, LineOf line_of)
{
    wgs_depth *d = g->depth;
    const int tpi = g->dp.tpi, need = (int)d->n * tpi;
    std::vector<int32_t> toks((size_t)need);
    std::vector<int32_t> &irows = g->dp.irows;
    irows.resize((size_t)2 * d->n);
    for (size_t t = 0; t < nl; ++t) {
        if (!g->flags[t] || g->dst[t] == -1) continue;
        const bool check_only = g->dst[t] == DEPTH_CHECK_ONLY;      // before the row range: the same refusals, no row
        const char *lb = nullptr, *le = nullptr;
        if (int rc = text_of(t, &lb, &le)) return rc;
        const long long line = (long long)(reader_table_skip_lines(g->r) + (int64_t)line_of(t, true) + 1);
        int bad_col = 0;
        const int k = reader_table_parse_line(lb, le, need, toks.data(), &bad_col);
        if (k == 1) {
            wgs_set_error("line %lld has fewer than %d columns (%lld individuals)", line, need, (long long)d->n);
            return 2;
        }
        if (k) {
            wgs_set_error("line %lld, column %d: not an integer np.loadtxt reads as int32", line, bad_col);
            return 2;
        }
        if (check_only && tpi != 2) continue;      // (counts: which two of a line's tokens matter is the row's owner's to say)
        const int64_t row = row0 + g->dst[t];
        if (tpi == 2) {
            memcpy(irows.data(), toks.data(), sizeof(int32_t) * (size_t)need);
        } else {
            uint8_t mm[2];
            HIP_TRY(hipMemcpy(mm, g->dp.sel.p + row * 2, 2, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < d->n; ++i) {
                irows[(size_t)(2 * i)] = toks[(size_t)(4 * i + (mm[0] & 3))];
                irows[(size_t)(2 * i + 1)] = toks[(size_t)(4 * i + (mm[1] & 3))];
            }
        }
        for (int32_t v : irows)
            if (v < 0 || v > 255) {
                wgs_set_error("line %lld: allele depths outside 0..255 do not fit the device table", line);
                return 2;
            }
        g->host_lines += 1;
        if (check_only) continue;
        if (int rc = wgs_depth_upload_rows(d, irows.data(), row, 1)) return rc;
    }
    return 0;
}

// Lines the device flagged (g->flags; bit patterns it leaves to strtod) and that have a row (g->dst), host-parsed and uploaded.
// text_of(t, &b, &e) fetches line t as [b, e) in host memory.  line_of(t, in_text) numbers it from 0: among the data lines the
// reader has handed out since the ingest began (what a Beagle file's messages count), or with in_text among all lines of the text
// (a table's).  A Beagle line goes through reader_text_parse_line, in runs of consecutive rows; a table's through the function above.
template <class TextOf, class LineOf>
int parse_flagged(wgs_ingest *g, int64_t row0, size_t nl, TextOf text_of, LineOf line_of)
{
    if (g->depth) return parse_flagged_table(g, row0, nl, text_of, line_of);
    wgs_beagle *b = g->b;
    const uint8_t *flags = g->flags.data();
    const int32_t *dst = g->dst.data();
    const size_t row_floats = (size_t)2 * (size_t)b->n;
    for (size_t i = 0; i < nl;) {
        if (!flags[i] || dst[i] < 0) {
            ++i;
            continue;
        }
        size_t j = i;
        while (j < nl && flags[j] && dst[j] == dst[i] + (int32_t)(j - i) && j - i < 4096) ++j;
        g->rows.resize((j - i) * row_floats);
        for (size_t t = i; t < j; ++t) {
            const char *lb = nullptr, *le = nullptr;
            if (int rc = text_of(t, &lb, &le)) return rc;
            if (reader_text_parse_line(g->r, lb, le, g->rows.data() + (t - i) * row_floats)) {
                wgs_set_error("Beagle data line %lld has fewer than %d genotype-likelihood columns",
                              (long long)(reader_text_lines_read(g->r) + (int64_t)line_of(t, false) + 2), reader_text_gl_cols(g->r));
                return 2;
            }
        }
        if (int rc = wgs_beagle_upload_rows(b, g->rows.data(), row0 + dst[i], (int64_t)(j - i))) return rc;
        g->host_lines += (int64_t)(j - i);
        i = j;
    }
    return 0;
}

/* BGZF, device-resident: per chunk the producer thread only READS the next members (reader.cpp: comp_producer); here
 *   H2D of the compressed bytes -> inflate_kernel (inflate.hip; one lane per member) into d_text behind the carried partial
 *   line -> newline positions (count per 4 KiB, scan, write) -> per line extent / blank / site name -> scans number the data
 *   lines and place the names -> dst (row limit, site mask) + names blob -> tokenise_kernel -> the partial last line moves
 *   to the front for the next chunk.
 * The host sees three small read-backs per chunk (counts, the names, the flag count) and the text never exists there.
 * One function per stage, in the order ingest_next_resident calls them; what they hand on about the chunk: */
struct Chunk {
    int nb = 0;                     // compressed members
    bool last = false;              // of the file
    size_t lead = 0;                // text ahead of the members': the carried partial line and what the reader had inflated itself
    size_t total = 0;               // all of the text in d_text
    size_t padded = 0;              // ... and with the newlines behind it that the kernels may read into
    size_t nl = 0;                  // whole lines
    size_t rows_here = 0, take = 0; // data lines among them, and those within the row limit
    size_t name_bytes = 0;          // of all the data lines' site names
    int64_t written = 0;            // rows of the target the chunk fills
    size_t nblk() const { return (total + 4095) / 4096; }
};

// The chunk's extent, and room for it in the buffers it is staged and inflated in.
int size_chunk(wgs_ingest *g, const CompChunk *c, Chunk &k)
{
    hipStream_t st = g->ctx->stream;
    k.last = c->last;
    k.nb = (int)c->isize.size();
    k.lead = g->carry + c->pre_len;
    k.total = k.lead + c->text_bytes + (k.last ? 1 : 0);     // a newline closes an unterminated last line
    WGS_REQUIRE(k.total + TEXT_PAD + 64 < (1ull << 32), "a Beagle line longer than 4 GiB");
    g->read_s += c->read_s;
    k.padded = ((k.total + TEXT_PAD + 15) & ~(size_t)15) + 64;
    if (int rc = g->d_text.reserve(st, k.padded, k.padded + k.padded / 8, g->carry)) return rc;      // keeps the carried partial line
    const size_t nb = (size_t)k.nb, cap = nb + nb / 4 + 256;
    if (int rc = reserve_all(st, nb, cap, g->d_in_off, g->d_out_off, g->d_in_len, g->d_isize, g->d_status)) return rc;
    if (int rc = g->d_tables.reserve(st, nb * inflate_table_bytes(), cap * inflate_table_bytes())) return rc;
    return g->d_comp.reserve(st, c->len + INFLATE_PAD, c->len + INFLATE_PAD);
}

// Compressed members to the device and through the inflate kernel, behind the text that leads the chunk.
int copy_and_inflate(wgs_ingest *g, const CompChunk *c, const Chunk &k)
{
    hipStream_t st = g->ctx->stream;
    uint8_t *text = g->d_text.p;
    const int nb = k.nb;
    if (int rc = clock_start(g)) return rc;
    HIP_TRY(hipMemsetAsync(g->d_totals.p, 0, T_COUNT * sizeof(uint32_t), st));
    if (c->pre_len) HIP_TRY(hipMemcpyAsync(text + g->carry, c->pre_text, c->pre_len, hipMemcpyHostToDevice, st));
    if (nb) {
        g->out_off.resize((size_t)nb);
        uint64_t at = k.lead;
        for (int i = 0; i < nb; ++i) {
            g->out_off[(size_t)i] = at;
            at += c->isize[(size_t)i];
        }
        HIP_TRY(hipMemcpyAsync(g->d_comp.p, c->comp, c->len, hipMemcpyHostToDevice, st));
        // zeros behind the chunk: a damaged last member that reads on finds an invalid stored-block header there, not the
        // stale bytes of the chunk before (the kernel stops a lane a few bytes past its stream's end anyway)
        HIP_TRY(hipMemsetAsync(g->d_comp.p + c->len, 0, INFLATE_PAD, st));
        HIP_TRY(hipMemcpyAsync(g->d_in_off.p, c->in_off.data(), sizeof(uint64_t) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(g->d_out_off.p, g->out_off.data(), sizeof(uint64_t) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(g->d_in_len.p, c->in_len.data(), sizeof(uint32_t) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(g->d_isize.p, c->isize.data(), sizeof(uint32_t) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(g->iev0, st));
        if (launch_inflate(g->ctx, g->d_comp.p, g->d_in_off.p, g->d_in_len.p, g->d_out_off.p, g->d_isize.p, text, g->d_status.p, g->d_tables.p, nb)) return 1;
        HIP_TRY(hipEventRecord(g->iev1, st));
        g->status.resize((size_t)nb);
        HIP_TRY(hipMemcpyAsync(g->status.data(), g->d_status.p, (size_t)nb, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemsetAsync(text + k.lead + c->text_bytes, '\n', k.padded - (k.lead + c->text_bytes), st));
    return 0;
}

// Newlines per 4 KiB of the text and their scan; waits for the stream: k.nl, and after the first call the members' status.
int count_newlines(wgs_ingest *g, Chunk &k)
{
    hipStream_t st = g->ctx->stream;
    const size_t nblk = k.nblk();
    if (int rc = reserve_all(st, nblk, nblk + nblk / 4 + 64, g->d_counts, g->d_offsets)) return rc;
    if (nblk) {
        hipLaunchKernelGGL(count_newlines_kernel, dim3((unsigned)nblk), dim3(256), 0, st, reinterpret_cast<const uint4 *>(g->d_text.p), (uint64_t)k.total, g->d_counts.p);
        hipLaunchKernelGGL(scan_u32_kernel, dim3(1), dim3(1024), 0, st, g->d_counts.p, g->d_offsets.p, (uint32_t)nblk, g->d_totals.p + T_NEWLINES);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(g->h_totals, g->d_totals.p, T_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    k.nl = g->h_totals[T_NEWLINES];
    return 0;
}

// Members the device did not accept: the host's inflater, patched into the device text; the newlines are counted again
// (WGSASSIGN_DEBUG_REJECT_MEMBERS=k, tests: every k-th member is treated as rejected and its device text wiped first).
int patch_rejected_members(wgs_ingest *g, const CompChunk *c, Chunk &k)
{
    uint8_t *text = g->d_text.p;
    const char *reject_env = getenv("WGSASSIGN_DEBUG_REJECT_MEMBERS");
    const int reject_every = reject_env ? atoi(reject_env) : 0;
    for (int i = 0; reject_every > 0 && i < k.nb; i += reject_every) {
        g->status[(size_t)i] = 1;
        HIP_TRY(hipMemset(text + g->out_off[(size_t)i], '#', c->isize[(size_t)i]));
    }
    bool patched = false;
    for (int i = 0; i < k.nb; ++i) {
        if (!g->status[(size_t)i]) continue;
        g->line.resize(65536);
        if (!reader_inflate_member(c->comp + c->in_off[(size_t)i], c->in_len[(size_t)i], c->isize[(size_t)i], reinterpret_cast<unsigned char *>(g->line.data()))) {
            wgs_set_error("read error in the BGZF file (corrupt block)");
            return 1;
        }
        HIP_TRY(hipMemcpy(text + g->out_off[(size_t)i], g->line.data(), c->isize[(size_t)i], hipMemcpyHostToDevice));
        ++g->blocks_host;
        patched = true;
    }
    return patched ? count_newlines(g, k) : 0;
}

// Where the newlines are, and per line its extent, whether it is a data line and its site name; waits for the stream:
// k.rows_here, k.name_bytes.
int list_lines(wgs_ingest *g, Chunk &k)
{
    hipStream_t st = g->ctx->stream;
    const size_t nl = k.nl;
    if (int rc = ensure_line_arrays(g, nl)) return rc;
    hipLaunchKernelGGL(write_newlines_kernel, dim3((unsigned)k.nblk()), dim3(256), 0, st, reinterpret_cast<const uint4 *>(g->d_text.p), (uint64_t)k.total, g->d_offsets.p, g->d_nl_pos.p);
    LineArgs la;
    la.text = g->d_text.p;
    la.nl_pos = g->d_nl_pos.p;
    la.nlines = (uint32_t)nl;
    la.begin = g->d_begin.p;
    la.end = g->d_end.p;
    la.nonblank = g->d_nonblank.p;
    la.name_start = g->d_name_start.p;
    la.name_len1 = g->d_name_len1.p;
    la.totals = g->d_totals.p;
    la.table = g->depth ? 1 : 0;
    hipLaunchKernelGGL(line_info_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st, la);
    hipLaunchKernelGGL(scan_u32_kernel, dim3(1), dim3(1024), 0, st, g->d_nonblank.p, g->d_rank.p, (uint32_t)nl, g->d_totals.p + T_NONBLANK);
    hipLaunchKernelGGL(scan_u32_kernel, dim3(1), dim3(1024), 0, st, g->d_name_len1.p, g->d_name_off.p, (uint32_t)nl, g->d_totals.p + T_NAME_BYTES);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(g->h_totals, g->d_totals.p, T_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    k.rows_here = g->h_totals[T_NONBLANK];
    k.name_bytes = g->h_totals[T_NAME_BYTES];
    return 0;
}

// The row limit and the site mask decide which data lines get which rows (k.take, k.written); per line its row, and the names blob.
int place_chunk_rows(wgs_ingest *g, int64_t row0, const uint8_t *keep, int64_t keep_len, Chunk &k)
{
    hipStream_t st = g->ctx->stream;
    k.take = k.rows_here;
    if (g->limit >= 0 && (int64_t)k.take >= g->limit - g->rows_done) {
        k.take = (size_t)(g->limit - g->rows_done);
        g->done = true;
    }
    if (k.last) g->done = true;
    const bool mapped = keep || g->dp.ranged;
    if (int rc = place_rows(g, row0, keep, keep_len, k.take, mapped ? &g->dstmap : nullptr, &k.written)) return rc;
    if (mapped && k.take) HIP_TRY(hipMemcpyAsync(g->d_dstmap.p, g->dstmap.data(), k.take * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (int rc = g->d_names.reserve(st, k.name_bytes + 16, k.name_bytes + k.name_bytes / 2 + 4096)) return rc;
    DstArgs da;
    da.nlines = (uint32_t)k.nl;
    da.take = g->dp.overflow ? 0u : (uint32_t)k.take;
    da.nonblank = g->d_nonblank.p;
    da.rank = g->d_rank.p;
    da.name_start = g->d_name_start.p;
    da.name_len1 = g->d_name_len1.p;
    da.name_off = g->d_name_off.p;
    da.dstmap = mapped ? g->d_dstmap.p : nullptr;
    da.text = g->d_text.p;
    da.dst = g->d_dst.p;
    da.names = g->d_names.p;
    da.totals = g->d_totals.p;
    hipLaunchKernelGGL(dst_names_kernel, dim3((unsigned)((k.nl + 255) / 256)), dim3(256), 0, st, da);
    return 0;
}

// The tokeniser over the chunk's lines; waits for the stream: the names, and the lines left to the host's parser.
int tokenise_chunk(wgs_ingest *g, int64_t row0, const Chunk &k)
{
    hipStream_t st = g->ctx->stream;
    const uint8_t *text = g->d_text.p;
    const size_t nl = k.nl;
    if (int rc = launch_tokenise(g, text, row0, nl, g->d_totals.p + T_FLAGGED)) return rc;
    g->names.resize(k.name_bytes);
    if (k.name_bytes) HIP_TRY(hipMemcpyAsync(&g->names[0], g->d_names.p, k.name_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(g->h_totals, g->d_totals.p, T_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (int rc = clock_stop(g)) return rc;
    if (k.take < k.rows_here || g->dp.overflow) g->names.resize(g->h_totals[T_NAME_CUT]);
    if (!g->h_totals[T_FLAGGED]) return 0;
    // rare: fetch what the host parser needs -- flags, extents, numbering -- and the flagged lines themselves
    auto fetch = [nl](auto &host, const auto &dev) {
        host.resize(nl);
        return hipMemcpy(host.data(), dev.p, nl * sizeof(*dev.p), hipMemcpyDeviceToHost);
    };
    HIP_TRY(fetch(g->flags, g->d_flags));
    HIP_TRY(fetch(g->dst, g->d_dst));
    HIP_TRY(fetch(g->h_begin, g->d_begin));
    HIP_TRY(fetch(g->h_end, g->d_end));
    HIP_TRY(fetch(g->h_rank, g->d_rank));
    auto text_of = [&](size_t t, const char **lb, const char **le) -> int {
        const size_t n = g->h_end[t] - g->h_begin[t];
        g->line.resize(n + 1);
        HIP_TRY(hipMemcpy(g->line.data(), text + g->h_begin[t], n, hipMemcpyDeviceToHost));
        *lb = g->line.data();
        *le = g->line.data() + n;
        return 0;
    };
    return parse_flagged(g, row0, nl, text_of, [&](size_t t, bool in_text) { return in_text ? g->dp.lines_before + (int64_t)t : g->rows_done + (int64_t)g->h_rank[t]; });
}

// The partial last line moves to the front for the next chunk (through a side buffer: the two ranges may overlap); queued behind
// the tokeniser, waited for by nobody but the next chunk's kernels.
int carry_tail(wgs_ingest *g, const Chunk &k)
{
    hipStream_t st = g->ctx->stream;
    const size_t tail = g->h_totals[T_TAIL];
    const size_t left = g->done ? 0 : k.total - tail;
    if (left) {
        if (int rc = g->d_carry.reserve(st, left, left + left / 2 + 65536)) return rc;
        HIP_TRY(hipMemcpyAsync(g->d_carry.p, g->d_text.p + tail, left, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(g->d_text.p, g->d_carry.p, left, hipMemcpyDeviceToDevice, st));
    }
    g->carry = left;
    return 0;
}

int ingest_next_resident(wgs_ingest *g, int64_t row0, const uint8_t *keep, int64_t keep_len, int64_t *file_rows, int64_t *rows_written)
{
    static const bool trace = getenv("WGSASSIGN_INGEST_TRACE") != nullptr;       // per-chunk wall times on stderr
    while (!g->done) {
        const double t_begin = now_s();
        CompChunk *c = nullptr;
        double waited = 0.0;
        if (int rc = reader_comp_next(g->r, &c, &waited)) return rc;
        g->wait_s += waited;
        if (!c) {
            g->done = true;
            break;
        }
        auto guard = on_failure([&] { reader_comp_release(g->r, c); });
        Chunk k;
        if (int rc = size_chunk(g, c, k)) return rc;
        const double t_alloc = now_s();
        if (int rc = copy_and_inflate(g, c, k)) return rc;
        if (int rc = count_newlines(g, k)) return rc;
        if (int rc = patch_rejected_members(g, c, k)) return rc;
        if (k.nb) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, g->iev0, g->iev1);
            g->inflate_kernel_ms += ms;
            g->blocks_inflated += k.nb;
        }
        const double t_inflated = now_s();
        reader_comp_release(g->r, c);                                   // the producer may refill it while the device works on
        guard.dismiss();
        g->text_bytes += (int64_t)(k.total - g->carry);
        g->chunks += 1;
        if (k.nl == 0) {                                                // not one whole line yet
            g->carry = k.total;
            if (k.last) g->done = true;
            continue;
        }
        if (int rc = list_lines(g, k)) return rc;
        const double t_listed = now_s();
        if (int rc = place_chunk_rows(g, row0, keep, keep_len, k)) return rc;
        if (int rc = tokenise_chunk(g, row0, k)) return rc;
        if (int rc = carry_tail(g, k)) return rc;
        g->dp.lines_before += (int64_t)k.nl;
        g->rows_done += (int64_t)k.take;
        g->lines += (int64_t)k.take;
        if (trace)
            fprintf(stderr, "ingest chunk %lld: %zu B text, %d members, %zu lines | wait %.1f ms, buffers %.1f, copy+inflate %.1f, list %.1f, rows+names+tokenise %.1f\n",
                    (long long)g->chunks, k.total, k.nb, k.nl, waited * 1e3, (t_alloc - t_begin - waited) * 1e3, (t_inflated - t_alloc) * 1e3,
                    (t_listed - t_inflated) * 1e3, (now_s() - t_listed) * 1e3);
        if (k.take == 0) continue;
        *file_rows = (int64_t)k.take;
        *rows_written = k.written;
        return 0;
    }
    return 0;
}

}  // namespace

int ingest_start(wgs_ingest *g, wgs_reader *r, int64_t limit_rows, int64_t chunk_bytes, int64_t resident_default, int64_t host_default,
                 wgs_ingest **out);

extern "C" {

void wgs_ingest_destroy(wgs_ingest *g)
{
    if (!g) return;
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);
    if (g->resident) {
        reader_add_lines_read(g->r, g->rows_done);
        reader_comp_stop(g->r);
    }
    reader_text_stop(g->r);                                    // joins the producer, frees the pinned buffers
    if (g->h_totals) (void)hipHostFree(g->h_totals);
    for (hipEvent_t e : {g->ev0, g->ev1, g->iev0, g->iev1, g->dp.kev0, g->dp.kev1})
        if (e) (void)hipEventDestroy(e);
    delete g;                                                  // frees the device arrays
}

/* chunk_bytes: text per chunk (<= 0: the default -- 256 MiB through the host inflater; 3 GiB -- or the members one launch has lanes for -- when the device inflates, one
 * lane per BGZF member: the more members per launch, the better the chip is used). */
int wgs_ingest_create(wgs_beagle *b, wgs_reader *r, int64_t limit_rows, int64_t chunk_bytes, wgs_ingest **out)
{
    WGS_REQUIRE(b && r && out, "null argument");
    WGS_REQUIRE(!reader_is_table(r), "the reader was opened for an integer table, not a Beagle file");
    WGS_REQUIRE(reader_text_n_inds(r) == b->n, "the Beagle file has %d individuals, the device matrix %lld", reader_text_n_inds(r),
                (long long)b->n);
    wgs_ingest *g = new wgs_ingest();
    g->b = b;
    g->ctx = b->ctx;
    g->m_rows = b->m;
    return ingest_start(g, r, limit_rows, chunk_bytes, 3ll << 30, 256ll << 20, out);
}

}  // extern "C"

// The part of the creation that both targets share; takes over `g` (destroyed on failure).
int ingest_start(wgs_ingest *g, wgs_reader *r, int64_t limit_rows, int64_t chunk_bytes, int64_t resident_default, int64_t host_default,
                 wgs_ingest **out)
{
    const double t_create = now_s();
    wgs_ctx *ctx = g->ctx;
    g->r = r;
    g->limit = limit_rows;
    auto guard = on_failure([&] { wgs_ingest_destroy(g); });
    HIP_TRY(hipSetDevice(ctx->device));
    // BGZF (what ANGSD writes): inflated on the device unless WGSASSIGN_INFLATE says host / zlib
    const char *how = getenv("WGSASSIGN_INFLATE");
    const bool resident = reader_text_is_bgzf(r) && !(how && (strcmp(how, "host") == 0 || strcmp(how, "zlib") == 0));
    // (one lane per member and three wavefronts per CU: a launch of up to 49 k members takes the time of one member, so a
    // chunk is that many members -- see reader_comp_start below -- or 3 GiB of text, whichever comes first)
    if (chunk_bytes <= 0) chunk_bytes = resident ? resident_default : host_default;
    chunk_bytes = std::min<int64_t>(chunk_bytes, resident ? (3ll << 30) : (1ll << 30));
    TextAllocator a;
    a.alloc = pinned_alloc;
    a.release = pinned_release;
    a.user = (void *)(intptr_t)ctx->device;
    HIP_TRY(hipEventCreate(&g->ev0));
    HIP_TRY(hipEventCreate(&g->ev1));
    if (resident) {
        HIP_TRY(hipEventCreate(&g->iev0));
        HIP_TRY(hipEventCreate(&g->iev1));
        if (int rc = g->d_totals.reserve(ctx->stream, T_COUNT, T_COUNT)) return rc;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&g->h_totals), T_COUNT * sizeof(uint32_t), hipHostMallocDefault));
        const size_t chunk_text = (size_t)std::max<int64_t>(chunk_bytes, g->depth ? 65536 : 1 << 20);
        g->resident = true;
        if (limit_rows == 0) g->done = true;
        // page-locked staging for the compressed members: an eighth of the text (low-depth ANGSD output deflates 10 : 1 and
        // more; where a file compresses less a chunk simply ends early), one buffer when the rest of the file fits into it
        else {
            size_t staging = std::max<size_t>(chunk_text / 8, 1u << 20);
            const int64_t left = reader_comp_bytes_left(r);
            int nbuf = 2;
            if (left >= 0 && (size_t)left + 4096 <= staging) {
                staging = std::max<size_t>(((size_t)left + 4096 + 0xFFFFF) & ~(size_t)0xFFFFF, 1u << 20);
                nbuf = 1;
            }
            // one lane per member and three wavefronts per CU (52 KiB of tables each): members beyond that many wait for a
            // second round of the launch
            const size_t lanes = (size_t)std::max(1, ctx->cus) * 3 * 64;
            if (int rc = reader_comp_start(r, staging, chunk_text, nbuf, a, lanes)) return rc;
        }
    } else if (int rc = reader_text_start(r, (size_t)chunk_bytes, 3, a, limit_rows)) {
        return rc;
    }
    guard.dismiss();
    g->create_s = now_s() - t_create;
    *out = g;
    return 0;
}

extern "C" {

/* The next chunk of the file: its lines are tokenised on the device into the slab rows row0, row0 + 1, ...
 * (keep != NULL: keep[i] says whether the i-th line of THIS chunk is kept; dropped lines take no row).
 * *file_rows = lines of the chunk (0 at the end of the file / the row limit), *rows_written = rows they filled. */
int wgs_ingest_next(wgs_ingest *g, int64_t row0, const uint8_t *keep, int64_t keep_len, int64_t *file_rows, int64_t *rows_written)
{
    WGS_REQUIRE(g && file_rows && rows_written, "null argument");
    HIP_TRY(hipSetDevice(g->ctx->device));
    hipStream_t st = g->ctx->stream;
    *file_rows = *rows_written = 0;
    g->names.clear();
    if (g->b) wgs_beagle_drop_codes(g->b);                     // the matrix changes: its class codes are rebuilt on next use
    struct Clock {
        wgs_ingest *g;
        double t0;
        ~Clock() { g->next_s += now_s() - t0; }
    } clock{g, now_s()};
    if (g->resident) return ingest_next_resident(g, row0, keep, keep_len, file_rows, rows_written);
    TextChunk *c = nullptr;
    double waited = 0.0;
    if (int rc = reader_text_next(g->r, &c, &waited)) return rc;
    g->wait_s += waited;
    if (!c) return 0;
    auto guard = on_failure([&] { reader_text_release(g->r, c); });
    const size_t nl = c->begin.size();
    int64_t written = 0;
    if (int rc = place_rows(g, row0, keep, keep_len, nl, &g->dst, &written)) return rc;
    const size_t text_bytes = (c->len + TEXT_PAD + 15) & ~(size_t)15;
    if (int rc = g->d_text.reserve(st, text_bytes, std::max(text_bytes, c->cap))) return rc;
    if (int rc = ensure_line_arrays(g, nl)) return rc;
    if (int rc = clock_start(g)) return rc;
    HIP_TRY(hipMemcpyAsync(g->d_text.p, c->data, text_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(g->d_begin.p, c->begin.data(), nl * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(g->d_end.p, c->end.data(), nl * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(g->d_dst.p, g->dst.data(), nl * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (int rc = launch_tokenise(g, g->d_text.p, row0, nl, nullptr)) return rc;
    g->flags.resize(nl);
    HIP_TRY(hipMemcpyAsync(g->flags.data(), g->d_flags.p, nl, hipMemcpyDeviceToHost, st));
    if (int rc = clock_stop(g)) return rc;
    auto text_of = [&](size_t t, const char **lb, const char **le) -> int {
        *lb = c->data + c->begin[t];
        *le = c->data + c->end[t];
        return 0;
    };
    auto line_of = [&](size_t t, bool in_text) { return in_text ? c->first_line + (int64_t)c->lineno[t] : c->first_row + (int64_t)t; };
    if (int rc = parse_flagged(g, row0, nl, text_of, line_of)) return rc;
    g->names.swap(c->names);
    g->inflate_s += c->inflate_s;
    g->scan_s += c->scan_s;
    g->text_bytes += (int64_t)c->len;
    g->lines += (int64_t)nl;
    g->chunks += 1;
    reader_text_release(g->r, c);
    guard.dismiss();
    *file_rows = (int64_t)nl;
    *rows_written = written;
    return 0;
}

/* Site names of the chunk wgs_ingest_next just returned (every line of it, kept or not), '\n'-terminated each. */
const char *wgs_ingest_chunk_sites(wgs_ingest *g, int64_t *bytes)
{
    if (!g) return nullptr;
    if (bytes) *bytes = (int64_t)g->names.size();
    return g->names.c_str();
}

/* stats[0..13]: seconds the consumer waited for the producer, producer seconds in inflate and in the newline scan (host
 * inflate), device milliseconds (copies + all kernels), lines parsed on the host, text bytes, lines, chunks, milliseconds of
 * the device inflate kernel, BGZF members inflated on the device, members the device left to the host's inflater, producer
 * seconds reading compressed members (device inflate), seconds in wgs_ingest_create and in wgs_ingest_next. */
int wgs_ingest_stats(wgs_ingest *g, double *stats)
{
    WGS_REQUIRE(g && stats, "null argument");
    stats[0] = g->wait_s;
    stats[1] = g->inflate_s;
    stats[2] = g->scan_s;
    stats[3] = g->device_ms;
    stats[4] = (double)g->host_lines;
    stats[5] = (double)g->text_bytes;
    stats[6] = (double)g->lines;
    stats[7] = (double)g->chunks;
    stats[8] = g->inflate_kernel_ms;
    stats[9] = (double)g->blocks_inflated;
    stats[10] = (double)g->blocks_host;
    stats[11] = g->read_s;
    stats[12] = g->create_s;
    stats[13] = g->next_s;
    return 0;
}

}  // extern "C"

/* ---- integer tables into the depth table (include/wgsassign_hip.h: wgs_depth_ingest_*): the ingest above with another target.
 * Chunks are small next to the Beagle ingest's -- 4 MiB of text through the host's inflater, 32 MiB when the device inflates --
 * because the point of this path is that the table never exists on the host: the page-locked buffers are all it holds. */
extern "C" {

int wgs_depth_ingest_create(wgs_depth *d, wgs_reader *r, int mode, const uint8_t *majmin, int64_t limit_rows, int64_t chunk_bytes,
                            wgs_depth_ingest **out)
{
    WGS_REQUIRE(d && r && out, "null argument");
    WGS_REQUIRE(reader_is_table(r), "the reader was not opened with wgs_reader_open_table");
    WGS_REQUIRE(mode == WGS_DEPTH_PAIRS || mode == WGS_DEPTH_COUNTS, "mode must be WGS_DEPTH_PAIRS or WGS_DEPTH_COUNTS");
    WGS_REQUIRE((mode == WGS_DEPTH_COUNTS) == (majmin != nullptr), "the (major, minor) selectors go with WGS_DEPTH_COUNTS, and only with it");
    const int tpi = mode == WGS_DEPTH_COUNTS ? 4 : 2;
    const int cols = reader_table_cols(r);
    if (cols > 0 && (int64_t)cols < d->n * tpi) {
        wgs_set_error("line %lld has %d columns, %lld individuals need %lld", (long long)(reader_table_skip_lines(r) + 1), cols, (long long)d->n,
                      (long long)(d->n * tpi));
        return 2;
    }
    if (majmin)
        for (int64_t i = 0; i < 2 * d->m; ++i)
            WGS_REQUIRE(majmin[i] <= 3, "site %lld: selector %d outside 0..3", (long long)(i / 2), (int)majmin[i]);
    wgs_ingest *g = new wgs_ingest();
    g->depth = d;
    g->ctx = d->ctx;
    g->m_rows = d->m;
    g->dp.tpi = tpi;
    if (majmin) {
        auto guard = on_failure([&] { delete g; });
        HIP_TRY(hipSetDevice(d->ctx->device));
        if (g->dp.sel.reserve(d->ctx->stream, (size_t)(2 * d->m), (size_t)(2 * d->m))) {
            wgs_set_error("hipMalloc of %lld bytes for the allele selectors failed", (long long)(2 * d->m));
            return 1;
        }
        HIP_TRY(hipMemcpy(g->dp.sel.p, majmin, (size_t)(2 * d->m), hipMemcpyHostToDevice));
        guard.dismiss();
    }
    wgs_ingest *made = nullptr;
    if (int rc = ingest_start(g, r, limit_rows, chunk_bytes, 32ll << 20, 4ll << 20, &made)) return rc;
    *out = reinterpret_cast<wgs_depth_ingest *>(made);
    return 0;
}

void wgs_depth_ingest_destroy(wgs_depth_ingest *g) { wgs_ingest_destroy(reinterpret_cast<wgs_ingest *>(g)); }

int wgs_depth_ingest_set_first_row(wgs_depth_ingest *gi, int64_t first_row)
{
    wgs_ingest *g = reinterpret_cast<wgs_ingest *>(gi);
    WGS_REQUIRE(g && g->depth, "null argument");
    WGS_REQUIRE(first_row >= 0, "first_row must not be negative");
    if (g->chunks || g->lines || g->dp.ranged) {
        wgs_set_error("the row range of a depth ingest is set once, before its first chunk");
        return 2;
    }
    g->dp.ranged = true;
    g->dp.before = first_row;
    return 0;
}

int wgs_depth_ingest_set_selectors(wgs_depth_ingest *gi, const uint8_t *majmin, int64_t nrows)
{
    wgs_ingest *g = reinterpret_cast<wgs_ingest *>(gi);
    WGS_REQUIRE(g && g->depth && majmin, "null argument");
    WGS_REQUIRE(g->dp.tpi == 4, "the (major, minor) selectors go with WGS_DEPTH_COUNTS, and only with it");
    WGS_REQUIRE(nrows >= 0 && nrows <= g->m_rows, "selectors of %lld rows for a table of %lld", (long long)nrows, (long long)g->m_rows);
    for (int64_t i = 0; i < 2 * nrows; ++i) WGS_REQUIRE(majmin[i] <= 3, "row %lld: selector %d outside 0..3", (long long)(i / 2), (int)majmin[i]);
    if (nrows == 0) return 0;
    HIP_TRY(hipSetDevice(g->ctx->device));
    HIP_TRY(hipStreamSynchronize(g->ctx->stream));           // (the chunk before has been tokenised)
    HIP_TRY(hipMemcpyAsync(g->dp.sel.p, majmin, (size_t)(2 * nrows), hipMemcpyHostToDevice, g->ctx->stream));
    HIP_TRY(hipStreamSynchronize(g->ctx->stream));
    return 0;
}

int wgs_depth_ingest_next(wgs_depth_ingest *gi, int64_t row0, int64_t *file_rows, int64_t *rows_written)
{
    wgs_ingest *g = reinterpret_cast<wgs_ingest *>(gi);
    WGS_REQUIRE(g && g->depth, "null argument");
    return wgs_ingest_next(g, row0, nullptr, 0, file_rows, rows_written);
}

/* stats[0..7]: largest single host buffer held (bytes: the reader's own buffers, the page-locked staging, a flagged line's row) |
 * device ms (copies + kernels) | lines parsed on the host | text bytes | data lines | chunks | BGZF members inflated on the device |
 * ms of the tokeniser kernel alone, from HIP events around its launches (0 unless WGSASSIGN_INGEST_TIME_KERNEL=1: the events
 * cost a synchronisation per chunk). */
int wgs_depth_ingest_stats(wgs_depth_ingest *gi, double *stats)
{
    wgs_ingest *g = reinterpret_cast<wgs_ingest *>(gi);
    WGS_REQUIRE(g && g->depth && stats, "null argument");
    size_t peak = std::max(reader_host_peak(g->r), g->dp.host_peak);
    peak = std::max(peak, g->dp.irows.capacity() * sizeof(int32_t));
    peak = std::max(peak, std::max(g->flags.capacity(), g->line.capacity()));
    peak = std::max(peak, std::max(g->dst.capacity(), g->h_begin.capacity()) * sizeof(int32_t));
    stats[0] = (double)peak;
    stats[1] = g->device_ms;
    stats[2] = (double)g->host_lines;
    stats[3] = (double)g->text_bytes;
    stats[4] = (double)g->lines;
    stats[5] = (double)g->chunks;
    stats[6] = (double)g->blocks_inflated;
    stats[7] = g->dp.tok_ms;
    return 0;
}

}  // extern "C"
