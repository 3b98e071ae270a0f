// What wgs_fisher_stream_push and wgs_fisher_stream_finish (api.hip) refuse before they launch anything, host-only and free of HIP:
// where a window may lie in the file, what its matrix and frequencies must look like, and when the means may be read.  Standard
// headers only, so a stand-alone program drives the checks on the CPU under the sanitizers
// (tests/c_abi/fisher_stream_checks_check.cpp).  Returns 0, or 2 with the reason in msg.
#pragma once
#include <stdint.h>
#include <stdio.h>

#define FISHER_STREAM_REFUSE(cond, ...)          \
    do {                                         \
        if (!(cond)) {                           \
            snprintf(msg, msg_len, __VA_ARGS__); \
            return 2;                            \
        }                                        \
    } while (0)

// The shape of a window: its matrix (n_window individuals in groups_window population slabs of slab_cols[g] individuals) and its
// frequencies (K_af columns of af_rows sites) against the stream's n individuals and K populations.
inline int fisher_stream_shape_refusal(int64_t n_window, int32_t groups_window, const int32_t *slab_cols, int32_t K_af, int64_t af_rows, int64_t rows,
                                       int64_t n, int32_t K, char *msg, size_t msg_len)
{
    FISHER_STREAM_REFUSE(n_window == n && K_af == K, "the window is %lld individuals x %d populations, the Fisher stream %lld x %d", (long long)n_window,
                         K_af, (long long)n, K);
    FISHER_STREAM_REFUSE(groups_window == K, "the window's matrix has %d population slabs, the Fisher stream %d populations", groups_window, K);
    FISHER_STREAM_REFUSE(rows > 0, "an empty window");
    FISHER_STREAM_REFUSE(af_rows == rows, "allele frequencies cover %lld SNPs, the window %lld", (long long)af_rows, (long long)rows);
    for (int32_t g = 0; g < groups_window; ++g) FISHER_STREAM_REFUSE(slab_cols[g] > 0, "population %d has no individuals", g);
    return 0;
}

// A window of `rows` sites from `site0` after `pushed` of the file's `m_total` sites; nothing is taken once the means were read.
inline int fisher_stream_window_refusal(int64_t site0, int64_t rows, int64_t pushed, int64_t m_total, int64_t align, int finished, char *msg,
                                        size_t msg_len)
{
    FISHER_STREAM_REFUSE(!finished, "the Fisher stream was finished: it takes no further window");
    FISHER_STREAM_REFUSE(site0 % align == 0, "the window starts at site %lld, which is not a multiple of %lld", (long long)site0, (long long)align);
    FISHER_STREAM_REFUSE(site0 == pushed, "the window starts at site %lld, but %lld sites were pushed so far", (long long)site0, (long long)pushed);
    FISHER_STREAM_REFUSE(rows <= m_total - pushed, "the window's %lld sites after %lld pushed exceed the %lld sites of the Fisher stream", (long long)rows,
                         (long long)pushed, (long long)m_total);
    FISHER_STREAM_REFUSE(pushed + rows == m_total || rows % align == 0, "a window of %lld sites that is not the last one (not a multiple of %lld)",
                         (long long)rows, (long long)align);
    return 0;
}

// The means are read once, after the file's last site.
inline int fisher_stream_finish_refusal(int64_t pushed, int64_t m_total, int finished, char *msg, size_t msg_len)
{
    FISHER_STREAM_REFUSE(pushed == m_total, "only %lld of the %lld sites were pushed", (long long)pushed, (long long)m_total);
    FISHER_STREAM_REFUSE(!finished, "the Fisher stream was finished already");
    return 0;
}

// How a window of `rows` sites splits for the per-individual sums: the sites of its full 8192-site chunks (fused sweep: 128-site
// leaves) and the rest, the file's last, shorter chunk (row route).
inline int64_t fisher_stream_full_sites(int64_t rows, int64_t align) { return rows / align * align; }
