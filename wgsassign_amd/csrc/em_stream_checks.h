// What wgs_em_stream_push (em_api.hip) refuses before it launches anything, host-only and free of HIP: where a window may lie in its
// round and what a round's plan may ask of it.  Standard headers only, so a stand-alone program drives the checks on the CPU under
// the sanitizers (tests/c_abi/em_stream_checks_check.cpp).  Each returns 0, or 2 with the reason in msg.
#pragma once
#include <stdint.h>
#include <stdio.h>

#define EM_STREAM_REFUSE(cond, ...)          \
    do {                                     \
        if (!(cond)) {                       \
            snprintf(msg, msg_len, __VA_ARGS__); \
            return 2;                        \
        }                                    \
    } while (0)

// A window of `rows` sites from `site0` in a batch made for `cap_rows`, after `pushed` of the round's `m_total` sites.
inline int em_stream_window_refusal(int64_t site0, int64_t rows, int64_t cap_rows, int64_t pushed, int64_t m_total, int64_t align, char *msg,
                                    size_t msg_len)
{
    EM_STREAM_REFUSE(rows > 0 && rows <= cap_rows, "a window of %lld sites in a batch made for %lld", (long long)rows, (long long)cap_rows);
    EM_STREAM_REFUSE(site0 % align == 0, "the window starts at site %lld, which is not a multiple of %lld", (long long)site0, (long long)align);
    EM_STREAM_REFUSE(site0 == pushed, "the window starts at site %lld, but %lld sites were pushed so far", (long long)site0, (long long)pushed);
    EM_STREAM_REFUSE(rows <= m_total - pushed, "the window's %lld sites after %lld pushed exceed the %lld sites of the fit stream", (long long)rows,
                     (long long)pushed, (long long)m_total);
    EM_STREAM_REFUSE(pushed + rows == m_total || rows % align == 0, "a window of %lld sites that is not the last one (not a multiple of %lld)",
                     (long long)rows, (long long)align);
    return 0;
}

// The plan of a push over a window of `rows` sites: iterations per fit, final fits and where they go, the chains.  *T_out: the most
// iterations any fit runs.
inline int em_stream_plan_refusal(int32_t n_fits, int32_t max_iter, const int32_t *run_iters, const int32_t *final, bool have_clamps,
                                  bool have_out, int64_t f_stride, int64_t rows, const int32_t *chain_fit, const int32_t *chain_iter,
                                  int32_t n_chain, int32_t *T_out, bool *any_final_out, char *msg, size_t msg_len)
{
    int32_t T = 0;
    bool any_final = false;
    EM_STREAM_REFUSE(n_chain >= 0 && (n_chain == 0 || (chain_fit && chain_iter)), "chains without their fits and iterations");
    for (int32_t j = 0; j < n_fits; ++j) {
        EM_STREAM_REFUSE(run_iters[j] >= 0 && run_iters[j] <= max_iter, "fit %d: %d iterations, the fit stream has %d", j, run_iters[j], max_iter);
        if (run_iters[j] > T) T = run_iters[j];
        any_final = any_final || (final && final[j]);
    }
    EM_STREAM_REFUSE(!any_final || (have_clamps && have_out && f_stride >= rows), "final fits need their clamps and %lld floats each to go to",
                     (long long)rows);
    for (int32_t i = 0; i < n_chain; ++i) {
        EM_STREAM_REFUSE(chain_fit[i] >= 0 && chain_fit[i] < n_fits, "chain %d: fit %d out of range", i, chain_fit[i]);
        EM_STREAM_REFUSE(chain_iter[i] >= 1 && chain_iter[i] <= run_iters[chain_fit[i]], "chain %d: iteration %d of fit %d, which runs %d", i,
                         chain_iter[i], chain_fit[i], run_iters[chain_fit[i]]);
        EM_STREAM_REFUSE(i == 0 || chain_iter[i - 1] <= chain_iter[i], "the chains are not sorted by iteration");
    }
    *T_out = T;
    *any_final_out = any_final;
    return 0;
}

// wgs_em_stream_push_keep: the iterations of every fit whose sums the table holds already lie inside what the fit runs.
inline int em_stream_sums_from_refusal(int32_t n_fits, const int32_t *run_iters, const int32_t *sums_from, char *msg, size_t msg_len)
{
    for (int32_t j = 0; j < n_fits; ++j)
        EM_STREAM_REFUSE(sums_from[j] >= 0 && sums_from[j] <= run_iters[j], "fit %d: sums above iteration %d, but it runs %d", j, sums_from[j],
                         run_iters[j]);
    return 0;
}
