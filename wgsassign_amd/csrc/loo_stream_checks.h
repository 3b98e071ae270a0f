// What wgs_loo_stream_push (score_api.hip) refuses before it launches anything, host-only and free of HIP: where a window may lie in
// the file and what its batch of re-fits and its frequencies must look like.  Standard headers only, so a stand-alone program drives
// the checks on the CPU under the sanitizers (tests/c_abi/loo_stream_checks_check.cpp).  Returns 0, or 2 with the reason in msg.
#pragma once
#include <stdint.h>
#include <stdio.h>

#define LOO_STREAM_REFUSE(cond, ...)         \
    do {                                     \
        if (!(cond)) {                       \
            snprintf(msg, msg_len, __VA_ARGS__); \
            return 2;                        \
        }                                    \
    } while (0)

// The shape of a window: its matrix (n_window individuals in groups_window population slabs), its batch (n_fits fits) and its
// frequencies (K_af columns of af_rows sites) against the stream's n individuals and K populations.
inline int loo_stream_shape_refusal(int64_t n_window, int32_t groups_window, int32_t n_fits, int32_t K_af, int64_t af_rows, int64_t rows,
                                    int64_t n, int32_t K, char *msg, size_t msg_len)
{
    LOO_STREAM_REFUSE(n_window == n && K_af == K, "the window is %lld individuals x %d populations, the leave-one-out stream %lld x %d",
                      (long long)n_window, K_af, (long long)n, K);
    LOO_STREAM_REFUSE(groups_window == K, "the window's matrix has %d population slabs, the leave-one-out stream %d populations", groups_window, K);
    LOO_STREAM_REFUSE((int64_t)n_fits == n, "the window's batch has %d fits, the leave-one-out stream %lld individuals", n_fits, (long long)n);
    LOO_STREAM_REFUSE(rows > 0, "an empty window");
    LOO_STREAM_REFUSE(af_rows == rows, "allele frequencies cover %lld SNPs, the window %lld", (long long)af_rows, (long long)rows);
    return 0;
}

// Fit i of the batch must be the re-fit of individual i: its population without it.  skipped[i] < 0: the fit leaves nobody out.
inline int loo_stream_fits_refusal(int64_t n, const int32_t *fit_group, const int32_t *skipped, const int32_t *group_of, char *msg, size_t msg_len)
{
    for (int64_t i = 0; i < n; ++i) {
        LOO_STREAM_REFUSE(fit_group[i] == group_of[i], "fit %lld is of population %d, individual %lld of population %d", (long long)i, fit_group[i],
                          (long long)i, group_of[i]);
        LOO_STREAM_REFUSE(skipped[i] >= 0, "fit %lld leaves nobody out: not a leave-one-out re-fit", (long long)i);
    }
    return 0;
}

// A window of `rows` sites from `site0` after `pushed` of the file's `m_total` sites.
inline int loo_stream_window_refusal(int64_t site0, int64_t rows, int64_t pushed, int64_t m_total, int64_t align, char *msg, size_t msg_len)
{
    LOO_STREAM_REFUSE(site0 % align == 0, "the window starts at site %lld, which is not a multiple of %lld", (long long)site0, (long long)align);
    LOO_STREAM_REFUSE(site0 == pushed, "the window starts at site %lld, but %lld sites were pushed so far", (long long)site0, (long long)pushed);
    LOO_STREAM_REFUSE(rows <= m_total - pushed, "the window's %lld sites after %lld pushed exceed the %lld sites of the leave-one-out stream",
                      (long long)rows, (long long)pushed, (long long)m_total);
    LOO_STREAM_REFUSE(pushed + rows == m_total || rows % align == 0, "a window of %lld sites that is not the last one (not a multiple of %lld)",
                      (long long)rows, (long long)align);
    return 0;
}

// wgs_loo_stream_push_scored: the matrix that is scored in place of the window the re-fits were made from (the downsampled file's window)
// must be that window's twin -- the same individuals, kept sites and first site, the same population slabs in the same file order.
inline int loo_stream_scored_refusal(int64_t n_scored, int64_t rows_scored, int64_t site0_scored, int32_t groups_scored, const int32_t *group_of_scored,
                                     int64_t n, int64_t rows, int64_t site0, int32_t groups, const int32_t *group_of, char *msg, size_t msg_len)
{
    LOO_STREAM_REFUSE(n_scored == n, "the scored window holds %lld individuals, the fitted window %lld", (long long)n_scored, (long long)n);
    LOO_STREAM_REFUSE(rows_scored == rows, "the scored window holds %lld sites, the fitted window %lld", (long long)rows_scored, (long long)rows);
    LOO_STREAM_REFUSE(site0_scored == site0, "the scored window starts at site %lld, the fitted window at site %lld", (long long)site0_scored,
                      (long long)site0);
    LOO_STREAM_REFUSE(groups_scored == groups, "the scored window has %d population slabs, the fitted window %d", groups_scored, groups);
    for (int64_t i = 0; i < n; ++i)
        LOO_STREAM_REFUSE(group_of_scored[i] == group_of[i], "individual %lld is of population %d in the scored window, of population %d in the fitted one",
                          (long long)i, group_of_scored[i], group_of[i]);
    return 0;
}
