// Every case the pre-launch checks of the windowed streams (csrc/stream_checks.h) are held to, stream by stream.  Two programs run
// them: stream_checks_check.cpp over every window of long files, under AddressSanitizer + UBSan, and stream_refusals_dump.cpp over a
// small grid, printing each message.  The checks that several streams share are reached through the adapters below, so that the same
// cases can be bound to another set of functions; the checks that are one stream's own are called by name.
#pragma once
#include "check_harness.h"
#include "stream_checks.h"

static const int64_t N = 12;        // the shapes: 12 individuals in 3 populations
static const int32_t K = 3;

// ---- adapters
static int score_window(int64_t site0, int64_t rows, int64_t pushed, int64_t m) { return stream_window_refusal("score stream", site0, rows, pushed, m, A, msg, sizeof msg); }
static int score_shape(int64_t n, int32_t Kaf, int64_t af_rows, int64_t rows) { return score_stream_shape_refusal(n, Kaf, af_rows, rows, N, K, msg, sizeof msg); }
static int all_pushed(int64_t pushed, int64_t m) { return stream_all_pushed_refusal(pushed, m, msg, sizeof msg); }
static int em_window(int64_t site0, int64_t rows, int64_t cap, int64_t pushed, int64_t m) { return em_stream_window_refusal(site0, rows, cap, pushed, m, A, msg, sizeof msg); }
static int loo_window(int64_t site0, int64_t rows, int64_t pushed, int64_t m) { return stream_window_refusal("leave-one-out stream", site0, rows, pushed, m, A, msg, sizeof msg); }
static int loo_shape(int64_t n, int32_t groups, int32_t fits, int32_t Kaf, int64_t af_rows, int64_t rows)
{
    return loo_stream_shape_refusal(n, groups, fits, Kaf, af_rows, rows, N, K, msg, sizeof msg);
}
static int fisher_window(int64_t site0, int64_t rows, int64_t pushed, int64_t m, int finished)
{
    return fisher_stream_window_refusal(site0, rows, pushed, m, A, finished, msg, sizeof msg);
}
static int fisher_shape(int64_t n, int32_t groups, const int32_t *cols, int32_t Kaf, int64_t af_rows, int64_t rows)
{
    return fisher_stream_shape_refusal(n, groups, cols, Kaf, af_rows, rows, N, K, msg, sizeof msg);
}
static int fisher_finish(int64_t pushed, int64_t m, int finished) { return fisher_stream_finish_refusal(pushed, m, finished, msg, sizeof msg); }
// ---- end of adapters

// The faults every shape rule knows, as bits of a mask: 0 another n, 1 another K, 2 an empty window, 3 frequencies of other rows.
static int64_t n_of(unsigned f) { return N + (f & 1u); }
static int32_t K_of(unsigned f) { return K + (f >> 1 & 1u); }
static int64_t rows_of(unsigned f) { return f & 4u ? 0 : 8192; }
static int64_t af_rows_of(unsigned f) { return f & 8u ? 8191 : rows_of(f); }

/* ---- the score stream: every window of a file accepted in order and refused out of order, the totals read only after the last one */
static void score_cases(Sizes files, Sizes windows)
{
    if (g_dump) g_dump = "score";
    walk_windows(files, windows,
        [](int64_t m_total, int64_t W, int64_t pushed, int64_t rows) {
            expect_window_rule([&](int64_t s, int64_t r) { return score_window(s, r, pushed, m_total); }, m_total, W, pushed, rows);
            expect(all_pushed(pushed, m_total), "sites were pushed", "the totals before the last window");
        },
        [](int64_t m_total, int64_t) { expect(all_pushed(m_total, m_total), nullptr, "the totals after the last window"); });
    expect_shape_faults({{"another n", "13 individuals x 3 populations, the score stream 12 x 3", "13 individuals x 4 populations"},
                         {"another K", "12 individuals x 4 populations, the score stream 12 x 3"}, {"no rows", "an empty window"},
                         {"frequencies of other rows", "allele frequencies cover 8191 SNPs, the window 8192"}},
                        [](unsigned f) { return score_shape(n_of(f), K_of(f), af_rows_of(f), rows_of(f)); });
}

/* ---- the fit stream: the windows of a round, and every way a plan can be wrong */
static void em_cases(Sizes files, Sizes windows)
{
    if (g_dump) g_dump = "em";
    walk_windows(files, windows,
        [](int64_t m_total, int64_t W, int64_t pushed, int64_t rows) {
            expect_window_rule([&](int64_t s, int64_t r) { return em_window(s, r, W, pushed, m_total); }, m_total, W, pushed, rows);
            expect(em_window(pushed, W + 1, W, pushed, m_total), "in a batch made for", "more rows than the batch holds");
            expect(em_window(pushed, 0, W, pushed, m_total), "in a batch made for", "an empty window");
            expect(all_pushed(pushed, m_total), "sites were pushed", "a read before the last window");
        },
        [](int64_t m_total, int64_t) { expect(all_pushed(m_total, m_total), nullptr, "a read after the last window"); });
    // plans
    const int n = 3, max_iter = 10;
    std::vector<int32_t> run = {5, 10, 0}, fin = {0, 1, 1}, cf = {0, 1, 0, 1}, ci = {1, 1, 5, 10};
    int32_t T = -1;
    bool any = false;
    auto plan = [&](const int32_t *f, bool clamps, bool out, int64_t stride, int nc) {
        return em_stream_plan_refusal(n, max_iter, run.data(), f, clamps, out, stride, 8192, cf.data(), ci.data(), nc, &T, &any, msg, sizeof msg);
    };
    expect(plan(fin.data(), true, true, 8192, 4), nullptr, "a good plan");
    expect_true(T == 10 && any, "the good plan's iterations and final fits");
    expect(plan(nullptr, false, false, 0, 0), nullptr, "no final fits, no chains");
    expect_true(!any, "no final fits without `final`");
    expect(plan(fin.data(), false, true, 8192, 0), "final fits need their clamps", "no clamps");
    expect(plan(fin.data(), true, false, 8192, 0), "final fits need their clamps", "nowhere to go");
    expect(plan(fin.data(), true, true, 8191, 0), "final fits need their clamps", "a short stride");
    run[1] = 11;
    expect(plan(nullptr, false, false, 0, 0), "fit 1: 11 iterations, the fit stream has 10", "too many iterations");
    run[1] = -1;
    expect(plan(nullptr, false, false, 0, 0), "fit 1: -1 iterations", "negative iterations");
    run[1] = 10;
    ci[2] = 6;
    expect(plan(nullptr, false, false, 0, 4), "chain 2: iteration 6 of fit 0, which runs 5", "a chain past its fit's last iteration");
    ci[2] = 0;
    expect(plan(nullptr, false, false, 0, 4), "chain 2: iteration 0", "a chain of iteration 0");
    ci[2] = 5;
    cf[3] = 3;
    expect(plan(nullptr, false, false, 0, 4), "chain 3: fit 3 out of range", "a chain of no fit");
    cf[3] = 2;
    expect(plan(nullptr, false, false, 0, 4), "chain 3: iteration 10 of fit 2, which runs 0", "a chain of a fit that does not run");
    cf[3] = 1;
    ci[1] = 7;
    expect(plan(nullptr, false, false, 0, 4), "not sorted by iteration", "unsorted chains");
    expect(em_stream_plan_refusal(n, max_iter, run.data(), nullptr, false, false, 0, 8192, nullptr, nullptr, 2, &T, &any, msg, sizeof msg),
           "chains without their fits", "chains without arrays");
}

/* ---- the masked push: every way the kept-site set can be wrong, the stride of its compacted vectors, and the plan check it shares */
static void masked_cases(std::initializer_list<int32_t> fit_counts, std::initializer_list<int32_t> keep_counts)
{
    if (g_dump) g_dump = "em";
    int matrix_a = 0, matrix_b = 0;         // two matrices: only their addresses are compared
    auto masked = [&](const void *keep_matrix, int32_t n_fits, int32_t keep_count, const int32_t *slot) {
        return em_stream_masked_refusal(&matrix_a, keep_matrix, n_fits, keep_count, slot, msg, sizeof msg);
    };
    for (int32_t n_fits : fit_counts)
        for (int32_t keep_count : keep_counts) {
            std::vector<int32_t> slot(n_fits);
            for (int32_t j = 0; j < n_fits; ++j) slot[j] = j % keep_count;
            expect(masked(&matrix_a, n_fits, keep_count, slot.data()), nullptr, "slots inside the set");
            expect(masked(&matrix_b, n_fits, keep_count, slot.data()), "belong to different matrices", "a set of another matrix");
            expect(masked(&matrix_a, n_fits, keep_count, nullptr), "needs the slot of every fit", "no slots");
            for (int32_t j : {0, n_fits / 2, n_fits - 1}) {
                const int32_t was = slot[j];
                char want[64];
                slot[j] = keep_count;
                snprintf(want, sizeof want, "fit %d: slot %d outside the kept-site set", j, keep_count);
                expect(masked(&matrix_a, n_fits, keep_count, slot.data()), want, "a slot past the set");
                slot[j] = -1;
                snprintf(want, sizeof want, "fit %d: slot -1 outside the kept-site set", j);
                expect(masked(&matrix_a, n_fits, keep_count, slot.data()), want, "a negative slot");
                slot[j] = was;
            }
            // the stride: the largest kept count among the slots the fits name, never below 1, whatever a slot nobody names holds
            std::vector<int64_t> kept(keep_count, 0);
            expect_true(em_stream_masked_stride(n_fits, slot.data(), kept.data()) == 1, "the stride of fits that kept nothing");
            for (int32_t s = 0; s < keep_count; ++s) kept[s] = (int64_t)(s * 37 % 101) * 83;
            int64_t want = 1;
            for (int32_t j = 0; j < n_fits; ++j) want = kept[slot[j]] > want ? kept[slot[j]] : want;
            expect_true(em_stream_masked_stride(n_fits, slot.data(), kept.data()) == want, "the stride of the fits");
            if (keep_count > n_fits) {
                kept[keep_count - 1] = (int64_t)1 << 40;
                expect_true(em_stream_masked_stride(n_fits, slot.data(), kept.data()) == want, "an unnamed slot set the stride");
            }
            kept[slot[n_fits - 1]] = ((int64_t)1 << 31) + 5;
            expect_true(em_stream_masked_stride(n_fits, slot.data(), kept.data()) == ((int64_t)1 << 31) + 5, "a stride beyond 2^31");
        }
    std::vector<int32_t> slot(EM_STREAM_MASKED_MAX_FITS + 1, 0);
    expect(masked(&matrix_a, EM_STREAM_MASKED_MAX_FITS, 1, slot.data()), nullptr, "the most fits");
    expect(masked(&matrix_a, EM_STREAM_MASKED_MAX_FITS + 1, 1, slot.data()), "holds at most 65535 fits", "too many fits for one launch");
    // the plan of a masked push is a keep push's plan: a chain beyond its fit's run_iters, final fits without clamps
    const int n = 3, max_iter = 10;
    std::vector<int32_t> run = {4, 8, 0}, fin = {1, 1, 1}, cf, ci;
    for (int t = 1; t <= 8; ++t)
        for (int k = 0; k < 2; ++k)
            if (t <= run[k]) {
                cf.push_back(k);
                ci.push_back(t);
            }
    int32_t T = -1;
    bool any = false;
    auto plan = [&](const int32_t *f, bool clamps, bool chains) {
        return em_stream_plan_refusal(n, max_iter, run.data(), f, clamps, true, 8192, 8192, chains ? cf.data() : nullptr, chains ? ci.data() : nullptr,
                                      chains ? (int32_t)cf.size() : 0, &T, &any, msg, sizeof msg);
    };
    expect(plan(nullptr, true, true), nullptr, "every iteration of every fit");
    expect_true(T == 8 && !any, "the masked plan's iterations and final fits");
    for (size_t i = 0; i < cf.size(); ++i) {
        if (cf[i] != 0) continue;
        const int32_t was = ci[i];
        ci[i] = 5;                          // fit 0 runs 4
        expect(plan(nullptr, true, true), "iteration 5 of fit 0, which runs 4", "a chain beyond its fit's run_iters");
        ci[i] = was;
    }
    expect(plan(fin.data(), false, false), "final fits need their clamps", "final fits without clamps");
    expect(plan(fin.data(), true, false), nullptr, "the final round");
}

/* ---- the leave-one-out stream: its windows, shapes and batch of re-fits, and wgs_em_stream_push_keep's sums above a horizon */
static void loo_cases(Sizes files, Sizes windows)
{
    if (g_dump) g_dump = "loo";
    walk_windows(files, windows,
        [](int64_t m_total, int64_t W, int64_t pushed, int64_t rows) {
            expect_window_rule([&](int64_t s, int64_t r) { return loo_window(s, r, pushed, m_total); }, m_total, W, pushed, rows);
            expect(all_pushed(pushed, m_total), "sites were pushed", "the totals before the last window");
        },
        [](int64_t m_total, int64_t) { expect(all_pushed(m_total, m_total), nullptr, "the totals after the last window"); });
    // shapes: n individuals in K slabs, a batch of n fits, K columns of as many rows as the window
    expect(loo_shape(N, K, (int32_t)N, K, 100, 100), nullptr, "a short good window");
    expect_shape_faults({{"another n", "13 individuals x 3 populations, the leave-one-out stream 12 x 3", "13 individuals x 4 populations"},
                         {"another K", "12 individuals x 4 populations"}, {"a matrix of one group", "has 1 population slabs"},
                         {"the batch of the population fits", "the window's batch has 3 fits, the leave-one-out stream 12 individuals"},
                         {"no rows", "an empty window"}, {"frequencies of other rows", "allele frequencies cover 8191 SNPs, the window 8192"}},
                        [&](unsigned f) {
                            const unsigned common = (f & 3u) | (f >> 2 & 12u);       // (bits 4 and 5 are the faults all rules share)
                            return loo_shape(n_of(common), f & 4u ? 1 : K, f & 8u ? K : (int32_t)N, K_of(common), af_rows_of(common), rows_of(common));
                        });
    // the batch: fit i is the population of individual i without i
    std::vector<int32_t> group_of = {0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2}, fit_group = group_of, skipped = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3};
    auto fits = [&]() { return loo_stream_fits_refusal(N, fit_group.data(), skipped.data(), group_of.data(), msg, sizeof msg); };
    expect(fits(), nullptr, "the n re-fits");
    fit_group[4] = 2;
    expect(fits(), "fit 4 is of population 2, individual 4 of population 1", "a fit of another population");
    fit_group[4] = 1;
    skipped[11] = -1;
    expect(fits(), "fit 11 leaves nobody out", "a full-population fit among the re-fits");
    skipped[11] = 3;
    expect(fits(), nullptr, "the n re-fits again");
    // sums above a horizon
    if (g_dump) g_dump = "em";
    std::vector<int32_t> run = {5, 10, 0}, from = {0, 10, 0};
    expect(em_stream_sums_from_refusal(3, run.data(), from.data(), msg, sizeof msg), nullptr, "sums from inside what the fits run");
    from[0] = 6;
    expect(em_stream_sums_from_refusal(3, run.data(), from.data(), msg, sizeof msg), "fit 0: sums above iteration 6, but it runs 5", "a horizon past the fit's run");
    from[0] = 5;
    from[2] = -1;
    expect(em_stream_sums_from_refusal(3, run.data(), from.data(), msg, sizeof msg), "fit 2: sums above iteration -1", "a negative horizon");
}

/* ---- wgs_loo_stream_push_scored: a window's twin is accepted; other individuals, sites, first site, slabs or grouping are refused */
static void scored_cases(Sizes files, Sizes windows)
{
    if (g_dump) g_dump = "loo";
    const std::vector<int32_t> group_of = {0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2};
    std::vector<int32_t> scored = group_of;
    auto twin = [&](int64_t n_s, int64_t rows_s, int64_t site0_s, int32_t groups_s, int64_t rows, int64_t site0) {
        return loo_stream_scored_refusal(n_s, rows_s, site0_s, groups_s, scored.data(), N, rows, site0, K, group_of.data(), msg, sizeof msg);
    };
    walk_windows(files, windows,
        [&](int64_t, int64_t W, int64_t site0, int64_t rows) {
            if (site0 / W > 65) return;     // (the long files: their first windows do)
            expect(twin(N, rows, site0, K, rows, site0), nullptr, "the window's twin");
            expect(twin(N, rows + 1, site0, K, rows, site0), "sites, the fitted window", "a site more");
            expect(twin(N, rows - 1, site0, K, rows, site0), "sites, the fitted window", "a site fewer");
            expect(twin(N, rows, site0 + A, K, rows, site0), "the fitted window at site", "the window after");
            expect(twin(N, rows, site0 + 1, K, rows, site0), "the fitted window at site", "a site further on");
            if (site0 >= W) expect(twin(N, rows, site0 - W, K, rows, site0), "the fitted window at site", "the window before");
        },
        [](int64_t, int64_t) {});
    expect(twin(N, 100, 0, K, 8192, 0), "the scored window holds 100 sites, the fitted window 8192", "a short window");
    expect(twin(N, 8192, 8192, K, 8192, 0), "the scored window starts at site 8192, the fitted window at site 0", "another first site");
    expect(twin(N + 1, 8192, 0, K, 8192, 0), "the scored window holds 13 individuals, the fitted window 12", "another n");
    expect(twin(N - 1, 8192, 0, K, 8192, 0), "the scored window holds 11 individuals, the fitted window 12", "an individual fewer");
    expect(twin(N, 8192, 0, 1, 8192, 0), "the scored window has 1 population slabs, the fitted window 3", "a matrix of one group");
    expect(twin(N, 8192, 0, K + 1, 8192, 0), "the scored window has 4 population slabs, the fitted window 3", "a slab more");
    // the order of the checks: the first difference is the one that is named, and group_of is read only once the shapes agree
    expect(twin(N + 1, 100, 8192, 1, 8192, 0), "individuals", "everything wrong at once");
    expect(twin(N, 100, 8192, 1, 8192, 0), "sites, the fitted window", "all but n wrong");
    expect(twin(N, 8192, 8192, 1, 8192, 0), "starts at site", "first site and slabs wrong");
    // every individual in every other population
    for (int64_t i = 0; i < N; ++i)
        for (int32_t g = 0; g < K; ++g) {
            scored = group_of;
            scored[i] = g;
            char want[96];
            snprintf(want, sizeof want, "individual %lld is of population %d in the scored window, of population %d in the fitted one", (long long)i, g,
                     group_of[i]);
            expect(twin(N, 8192, 0, K, 8192, 0), g == group_of[i] ? nullptr : want, "one individual regrouped");
        }
    // the same slab sizes in another file order are another grouping
    scored = {2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1};
    expect(twin(N, 8192, 0, K, 8192, 0), "individual 0 is of population 2 in the scored window, of population 0 in the fitted one", "a rotated grouping");
    scored = group_of;
    expect(twin(N, 8192, 0, K, 8192, 0), nullptr, "the twin again");
}

/* ---- the Fisher stream: its windows, the means given once after the last site, its shapes, the split into full chunks and a rest */
static void fisher_cases(Sizes files, Sizes windows)
{
    if (g_dump) g_dump = "fisher";
    int64_t full_seen = 0;
    walk_windows(files, windows,
        [&](int64_t m_total, int64_t W, int64_t pushed, int64_t rows) {
            expect(fisher_finish(pushed, m_total, 0), "sites were pushed", "the means before the last window");
            expect_window_rule([&](int64_t s, int64_t r) { return fisher_window(s, r, pushed, m_total, 0); }, m_total, W, pushed, rows);
            expect(fisher_window(pushed, rows, pushed, m_total, 1), "takes no further window", "a window after the means");
            if (g_dump)
                expect_window_rule([&](int64_t s, int64_t r) { return fisher_window(s, r, pushed, m_total, 1); }, m_total, W, pushed, rows,
                                   "takes no further window");
            if (pushed) expect(fisher_window(0, rows, pushed, m_total, 0), "sites were pushed so far", "the first window again");
            // the split: full chunks first, and only the file's last window has a rest
            const int64_t full = fisher_stream_full_sites(rows, A);
            expect_true(full % A == 0 && full <= rows && rows - full < A, "full chunks of a window");
            expect_true(rows - full == 0 || pushed + rows == m_total, "a rest outside the last window");
            full_seen += full;
        },
        [&](int64_t m_total, int64_t) {
            expect_true(full_seen == m_total / A * A, "the full chunks of all windows are the file's");
            full_seen = 0;
            expect(fisher_finish(m_total, m_total, 0), nullptr, "the means after the last window");
            expect(fisher_finish(m_total, m_total, 1), "finished already", "the means a second time");
            expect(fisher_window(m_total, 1, m_total, m_total, 0), m_total % A ? "not a multiple of 8192" : "exceed the", "a window past the end");
        });
    // shapes: n individuals in K slabs, none empty, K columns of as many rows as the window
    std::vector<int32_t> cols = {1, 4, 7};
    auto shape = [&](int64_t n, int32_t groups, int32_t Kaf, int64_t af_rows, int64_t rows) { return fisher_shape(n, groups, cols.data(), Kaf, af_rows, rows); };
    expect(shape(N, K, K, 100, 100), nullptr, "a short good window");
    expect(shape(N, K, K - 1, 8192, 8192), "12 individuals x 2 populations", "a wrong K");
    cols[2] = 0;
    expect(shape(N, K, K, 8192, 8192), "population 2 has no individuals", "an empty last population");
    cols[2] = 7;
    expect_shape_faults({{"another n", "13 individuals x 3 populations, the Fisher stream 12 x 3", "13 individuals x 4 populations"},
                         {"another K", "12 individuals x 4 populations"}, {"a matrix of one group", "has 1 population slabs"},
                         {"no rows", "an empty window"}, {"frequencies of other rows", "allele frequencies cover 8191 SNPs, the window 8192"},
                         {"an empty population", "population 1 has no individuals"}},
                        [&](unsigned f) {
                            const unsigned common = (f & 3u) | (f >> 1 & 12u);       // (bits 3 and 4 are the faults all rules share)
                            cols[1] = f & 32u ? 0 : 4;
                            return shape(n_of(common), f & 4u ? 1 : K, K_of(common), af_rows_of(common), rows_of(common));
                        });
}
