// What the windowed streams refuse before they launch anything (wgs_score_stream_*, wgs_em_stream_*, wgs_loo_stream_*,
// wgs_fisher_stream_*), host-only and free of HIP.  Standard headers only, so stand-alone programs drive every check on the CPU: under
// the sanitizers (tests/c_abi/stream_checks_check.cpp), and message by message (tests/c_abi/stream_refusals_dump.cpp).  Each check
// returns 0, or 2 with the reason in msg; a push reports the first check that refuses, so their order is part of the ABI.
//
// The window rule, once: a window's first site equals the sites pushed so far and is a multiple of `align` (WGS_WINDOW_ALIGN, 8192:
// the sites of one addend of NumPy's running totals, which a window that began elsewhere would regroup); every window but the last
// holds a multiple of `align` sites; no window overruns the file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#define STREAM_REFUSE(cond, ...)                 \
    do {                                         \
        if (!(cond)) {                           \
            snprintf(msg, msg_len, __VA_ARGS__); \
            return 2;                            \
        }                                        \
    } while (0)

/* ---- shared by every stream; `stream` names it in the message ("score stream", "fit stream", "leave-one-out stream", "Fisher stream") */

// The window rule: a window of `rows` sites from `site0` after `pushed` of the `m_total` sites.
inline int stream_window_refusal(const char *stream, int64_t site0, int64_t rows, int64_t pushed, int64_t m_total, int64_t align, char *msg,
                                 size_t msg_len)
{
    STREAM_REFUSE(site0 % align == 0, "the window starts at site %lld, which is not a multiple of %lld", (long long)site0, (long long)align);
    STREAM_REFUSE(site0 == pushed, "the window starts at site %lld, but %lld sites were pushed so far", (long long)site0, (long long)pushed);
    STREAM_REFUSE(rows <= m_total - pushed, "the window's %lld sites after %lld pushed exceed the %lld sites of the %s", (long long)rows,
                  (long long)pushed, (long long)m_total, stream);
    STREAM_REFUSE(pushed + rows == m_total || rows % align == 0, "a window of %lld sites that is not the last one (not a multiple of %lld)",
                  (long long)rows, (long long)align);
    return 0;
}

// The pieces of the shape rule: the window's n individuals and K_af frequency columns are the stream's, its matrix has one slab per
// population, it is not empty and its frequencies cover its rows.
inline int stream_dims_refusal(const char *stream, int64_t n_window, int32_t K_af, int64_t n, int32_t K, char *msg, size_t msg_len)
{
    STREAM_REFUSE(n_window == n && K_af == K, "the window is %lld individuals x %d populations, the %s %lld x %d", (long long)n_window, K_af, stream,
                  (long long)n, K);
    return 0;
}
inline int stream_slabs_refusal(const char *stream, int32_t groups_window, int32_t K, char *msg, size_t msg_len)
{
    STREAM_REFUSE(groups_window == K, "the window's matrix has %d population slabs, the %s %d populations", groups_window, stream, K);
    return 0;
}
inline int stream_rows_refusal(int64_t af_rows, int64_t rows, char *msg, size_t msg_len)
{
    STREAM_REFUSE(rows > 0, "an empty window");
    STREAM_REFUSE(af_rows == rows, "allele frequencies cover %lld SNPs, the window %lld", (long long)af_rows, (long long)rows);
    return 0;
}

// What a stream holds is read only after the last site.
inline int stream_all_pushed_refusal(int64_t pushed, int64_t m_total, char *msg, size_t msg_len)
{
    STREAM_REFUSE(pushed == m_total, "only %lld of the %lld sites were pushed", (long long)pushed, (long long)m_total);
    return 0;
}

/* ---- wgs_score_stream_push */

inline int score_stream_shape_refusal(int64_t n_window, int32_t K_af, int64_t af_rows, int64_t rows, int64_t n, int32_t K, char *msg, size_t msg_len)
{
    if (int rc = stream_dims_refusal("score stream", n_window, K_af, n, K, msg, msg_len)) return rc;
    return stream_rows_refusal(af_rows, rows, msg, msg_len);
}

/* ---- wgs_em_stream_push and its kin */

// A window of `rows` sites from `site0` in a batch made for `cap_rows`, after `pushed` of the round's `m_total` sites.
inline int em_stream_window_refusal(int64_t site0, int64_t rows, int64_t cap_rows, int64_t pushed, int64_t m_total, int64_t align, char *msg,
                                    size_t msg_len)
{
    STREAM_REFUSE(rows > 0 && rows <= cap_rows, "a window of %lld sites in a batch made for %lld", (long long)rows, (long long)cap_rows);
    return stream_window_refusal("fit stream", site0, rows, pushed, m_total, align, msg, msg_len);
}

// The plan of a push over a window of `rows` sites: iterations per fit, final fits and where they go, the chains.  *T_out: the most
// iterations any fit runs.
inline int em_stream_plan_refusal(int32_t n_fits, int32_t max_iter, const int32_t *run_iters, const int32_t *final, bool have_clamps,
                                  bool have_out, int64_t f_stride, int64_t rows, const int32_t *chain_fit, const int32_t *chain_iter,
                                  int32_t n_chain, int32_t *T_out, bool *any_final_out, char *msg, size_t msg_len)
{
    int32_t T = 0;
    bool any_final = false;
    STREAM_REFUSE(n_chain >= 0 && (n_chain == 0 || (chain_fit && chain_iter)), "chains without their fits and iterations");
    for (int32_t j = 0; j < n_fits; ++j) {
        STREAM_REFUSE(run_iters[j] >= 0 && run_iters[j] <= max_iter, "fit %d: %d iterations, the fit stream has %d", j, run_iters[j], max_iter);
        if (run_iters[j] > T) T = run_iters[j];
        any_final = any_final || (final && final[j]);
    }
    STREAM_REFUSE(!any_final || (have_clamps && have_out && f_stride >= rows), "final fits need their clamps and %lld floats each to go to",
                  (long long)rows);
    for (int32_t i = 0; i < n_chain; ++i) {
        STREAM_REFUSE(chain_fit[i] >= 0 && chain_fit[i] < n_fits, "chain %d: fit %d out of range", i, chain_fit[i]);
        STREAM_REFUSE(chain_iter[i] >= 1 && chain_iter[i] <= run_iters[chain_fit[i]], "chain %d: iteration %d of fit %d, which runs %d", i,
                      chain_iter[i], chain_fit[i], run_iters[chain_fit[i]]);
        STREAM_REFUSE(i == 0 || chain_iter[i - 1] <= chain_iter[i], "the chains are not sorted by iteration");
    }
    *T_out = T;
    *any_final_out = any_final;
    return 0;
}

// wgs_em_stream_push_keep: the iterations of every fit whose sums the table holds already lie inside what the fit runs.
inline int em_stream_sums_from_refusal(int32_t n_fits, const int32_t *run_iters, const int32_t *sums_from, char *msg, size_t msg_len)
{
    for (int32_t j = 0; j < n_fits; ++j)
        STREAM_REFUSE(sums_from[j] >= 0 && sums_from[j] <= run_iters[j], "fit %d: sums above iteration %d, but it runs %d", j, sums_from[j],
                      run_iters[j]);
    return 0;
}

constexpr int32_t EM_STREAM_MASKED_MAX_FITS = 65535;      // the compaction of one iteration is ONE launch: one grid row per fit

// wgs_em_stream_push_masked: the kept-site set was made from the batch's own matrix (the pointers are only compared), and fit j takes
// fit_slot[j] of its `keep_count` slots.
inline int em_stream_masked_refusal(const void *batch_matrix, const void *keep_matrix, int32_t n_fits, int32_t keep_count,
                                    const int32_t *fit_slot, char *msg, size_t msg_len)
{
    STREAM_REFUSE(fit_slot, "a masked push needs the slot of every fit");
    STREAM_REFUSE(batch_matrix == keep_matrix, "the EM batch and the kept-site set belong to different matrices");
    STREAM_REFUSE(n_fits <= EM_STREAM_MASKED_MAX_FITS, "a masked push holds at most %d fits, not %d", EM_STREAM_MASKED_MAX_FITS, n_fits);
    for (int32_t j = 0; j < n_fits; ++j)
        STREAM_REFUSE(fit_slot[j] >= 0 && fit_slot[j] < keep_count, "fit %d: slot %d outside the kept-site set", j, fit_slot[j]);
    return 0;
}

// Floats per fit of each of the two compacted vectors of a masked push: the largest kept count of this window among the fits' slots,
// at least 1 (kept[s]: the sites slot s kept; the slots were checked by em_stream_masked_refusal).
inline int64_t em_stream_masked_stride(int32_t n_fits, const int32_t *fit_slot, const int64_t *kept)
{
    int64_t stride = 1;
    for (int32_t j = 0; j < n_fits; ++j)
        if (kept[fit_slot[j]] > stride) stride = kept[fit_slot[j]];
    return stride;
}

/* ---- wgs_loo_stream_push and wgs_loo_stream_push_scored */

// The shape of a window: its matrix (n_window individuals in groups_window population slabs), its batch (n_fits fits) and its
// frequencies (K_af columns of af_rows sites) against the stream's n individuals and K populations.
inline int loo_stream_shape_refusal(int64_t n_window, int32_t groups_window, int32_t n_fits, int32_t K_af, int64_t af_rows, int64_t rows,
                                    int64_t n, int32_t K, char *msg, size_t msg_len)
{
    if (int rc = stream_dims_refusal("leave-one-out stream", n_window, K_af, n, K, msg, msg_len)) return rc;
    if (int rc = stream_slabs_refusal("leave-one-out stream", groups_window, K, msg, msg_len)) return rc;
    STREAM_REFUSE((int64_t)n_fits == n, "the window's batch has %d fits, the leave-one-out stream %lld individuals", n_fits, (long long)n);
    return stream_rows_refusal(af_rows, rows, msg, msg_len);
}

// Fit i of the batch must be the re-fit of individual i: its population without it.  skipped[i] < 0: the fit leaves nobody out.
inline int loo_stream_fits_refusal(int64_t n, const int32_t *fit_group, const int32_t *skipped, const int32_t *group_of, char *msg, size_t msg_len)
{
    for (int64_t i = 0; i < n; ++i) {
        STREAM_REFUSE(fit_group[i] == group_of[i], "fit %lld is of population %d, individual %lld of population %d", (long long)i, fit_group[i],
                      (long long)i, group_of[i]);
        STREAM_REFUSE(skipped[i] >= 0, "fit %lld leaves nobody out: not a leave-one-out re-fit", (long long)i);
    }
    return 0;
}

// wgs_loo_stream_push_scored: the matrix that is scored in place of the window the re-fits were made from (the downsampled file's window)
// must be that window's twin -- the same individuals, kept sites and first site, the same population slabs in the same file order.
inline int loo_stream_scored_refusal(int64_t n_scored, int64_t rows_scored, int64_t site0_scored, int32_t groups_scored, const int32_t *group_of_scored,
                                     int64_t n, int64_t rows, int64_t site0, int32_t groups, const int32_t *group_of, char *msg, size_t msg_len)
{
    STREAM_REFUSE(n_scored == n, "the scored window holds %lld individuals, the fitted window %lld", (long long)n_scored, (long long)n);
    STREAM_REFUSE(rows_scored == rows, "the scored window holds %lld sites, the fitted window %lld", (long long)rows_scored, (long long)rows);
    STREAM_REFUSE(site0_scored == site0, "the scored window starts at site %lld, the fitted window at site %lld", (long long)site0_scored,
                  (long long)site0);
    STREAM_REFUSE(groups_scored == groups, "the scored window has %d population slabs, the fitted window %d", groups_scored, groups);
    for (int64_t i = 0; i < n; ++i)
        STREAM_REFUSE(group_of_scored[i] == group_of[i], "individual %lld is of population %d in the scored window, of population %d in the fitted one",
                      (long long)i, group_of_scored[i], group_of[i]);
    return 0;
}

/* ---- wgs_fisher_stream_push and wgs_fisher_stream_finish */

// The shape of a window: its matrix (n_window individuals in groups_window population slabs of slab_cols[g] individuals) and its
// frequencies (K_af columns of af_rows sites) against the stream's n individuals and K populations.
inline int fisher_stream_shape_refusal(int64_t n_window, int32_t groups_window, const int32_t *slab_cols, int32_t K_af, int64_t af_rows, int64_t rows,
                                       int64_t n, int32_t K, char *msg, size_t msg_len)
{
    if (int rc = stream_dims_refusal("Fisher stream", n_window, K_af, n, K, msg, msg_len)) return rc;
    if (int rc = stream_slabs_refusal("Fisher stream", groups_window, K, msg, msg_len)) return rc;
    if (int rc = stream_rows_refusal(af_rows, rows, msg, msg_len)) return rc;
    for (int32_t g = 0; g < groups_window; ++g) STREAM_REFUSE(slab_cols[g] > 0, "population %d has no individuals", g);
    return 0;
}

// The window rule; nothing is taken once the means were read.
inline int fisher_stream_window_refusal(int64_t site0, int64_t rows, int64_t pushed, int64_t m_total, int64_t align, int finished, char *msg,
                                        size_t msg_len)
{
    STREAM_REFUSE(!finished, "the Fisher stream was finished: it takes no further window");
    return stream_window_refusal("Fisher stream", site0, rows, pushed, m_total, align, msg, msg_len);
}

// The means are read once, after the file's last site.
inline int fisher_stream_finish_refusal(int64_t pushed, int64_t m_total, int finished, char *msg, size_t msg_len)
{
    if (int rc = stream_all_pushed_refusal(pushed, m_total, msg, msg_len)) return rc;
    STREAM_REFUSE(!finished, "the Fisher stream was finished already");
    return 0;
}

// How a window of `rows` sites splits for the per-individual sums: the sites of its full 8192-site chunks (fused sweep: 128-site
// leaves) and the rest, the file's last, shorter chunk (row route).
inline int64_t fisher_stream_full_sites(int64_t rows, int64_t align) { return rows / align * align; }
