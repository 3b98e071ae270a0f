// What wgs_loo_stream_push refuses before any launch (csrc/loo_stream_checks.h) and what wgs_em_stream_push_keep adds to the checks of
// wgs_em_stream_push (csrc/em_stream_checks.h: sums above a horizon), driven on the CPU under AddressSanitizer + UBSan: every window of
// a file in windows of 8192 sites is accepted in order and refused out of order, and every way a window's shape or its batch of re-fits
// can be wrong is refused with its reason.  Prints "ok" and the number of checks; any surprise ends it with status 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "em_stream_checks.h"
#include "loo_stream_checks.h"

static int g_checks = 0;
static char msg[256];

static void expect(int rc, const char *part, const char *what)
{
    ++g_checks;
    const bool ok = part ? (rc == 2 && strstr(msg, part)) : rc == 0;
    if (!ok) {
        printf("FAILED: %s: rc %d, message '%s', expected %s\n", what, rc, msg, part ? part : "acceptance");
        exit(1);
    }
    msg[0] = 0;
}

int main()
{
    const int64_t A = 8192;
    for (int64_t m_total : {1ll, 100ll, 8192ll, 8193ll, 20000ll, 16384ll, 3 * 8192ll + 63, (1ll << 33) + 5}) {
        for (int64_t W : {A, 2 * A, 1000 * A}) {
            int64_t pushed = 0;
            while (pushed < m_total) {
                const int64_t rows = m_total - pushed < W ? m_total - pushed : W;
                expect(loo_stream_window_refusal(pushed, rows, pushed, m_total, A, msg, sizeof msg), nullptr, "a window in its place");
                expect(loo_stream_window_refusal(pushed + A, rows, pushed, m_total, A, msg, sizeof msg), "sites were pushed so far", "a window too far on");
                expect(loo_stream_window_refusal(pushed + 100, rows, pushed, m_total, A, msg, sizeof msg), "not a multiple of 8192", "an unaligned window");
                if (rows > 1 && pushed + rows - 1 < m_total && (rows - 1) % A)
                    expect(loo_stream_window_refusal(pushed, rows - 1, pushed, m_total, A, msg, sizeof msg), "not the last one", "a ragged middle window");
                if (m_total - pushed < W)
                    expect(loo_stream_window_refusal(pushed, W, pushed, m_total, A, msg, sizeof msg), "exceed the", "an overrun");
                pushed += rows;
            }
        }
    }
    // shapes: n individuals in K slabs, a batch of n fits, K columns of as many rows as the window
    const int64_t n = 12;
    const int32_t K = 3;
    auto shape = [&](int64_t nw, int32_t groups, int32_t fits, int32_t Kaf, int64_t af_rows, int64_t rows) {
        return loo_stream_shape_refusal(nw, groups, fits, Kaf, af_rows, rows, n, K, msg, sizeof msg);
    };
    expect(shape(n, K, (int32_t)n, K, 8192, 8192), nullptr, "a good window");
    expect(shape(n, K, (int32_t)n, K, 100, 100), nullptr, "a short good window");
    expect(shape(n + 1, K, (int32_t)n, K, 8192, 8192), "13 individuals x 3 populations, the leave-one-out stream 12 x 3", "another n");
    expect(shape(n, K, (int32_t)n, K + 1, 8192, 8192), "12 individuals x 4 populations", "another K");
    expect(shape(n, 1, (int32_t)n, K, 8192, 8192), "has 1 population slabs", "a matrix of one group");
    expect(shape(n, K, K, K, 8192, 8192), "the window's batch has 3 fits, the leave-one-out stream 12 individuals", "the batch of the population fits");
    expect(shape(n, K, (int32_t)n, K, 0, 0), "an empty window", "no rows");
    expect(shape(n, K, (int32_t)n, K, 8191, 8192), "allele frequencies cover 8191 SNPs, the window 8192", "frequencies of other rows");
    // the batch: fit i is the population of individual i without i
    std::vector<int32_t> group_of = {0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2}, fit_group = group_of, skipped = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3};
    auto fits = [&]() { return loo_stream_fits_refusal(n, fit_group.data(), skipped.data(), group_of.data(), msg, sizeof msg); };
    expect(fits(), nullptr, "the n re-fits");
    fit_group[4] = 2;
    expect(fits(), "fit 4 is of population 2, individual 4 of population 1", "a fit of another population");
    fit_group[4] = 1;
    skipped[11] = -1;
    expect(fits(), "fit 11 leaves nobody out", "a full-population fit among the re-fits");
    skipped[11] = 3;
    expect(fits(), nullptr, "the n re-fits again");
    // sums above a horizon
    std::vector<int32_t> run = {5, 10, 0}, from = {0, 10, 0};
    expect(em_stream_sums_from_refusal(3, run.data(), from.data(), msg, sizeof msg), nullptr, "sums from inside what the fits run");
    from[0] = 6;
    expect(em_stream_sums_from_refusal(3, run.data(), from.data(), msg, sizeof msg), "fit 0: sums above iteration 6, but it runs 5", "a horizon past the fit's run");
    from[0] = 5;
    from[2] = -1;
    expect(em_stream_sums_from_refusal(3, run.data(), from.data(), msg, sizeof msg), "fit 2: sums above iteration -1", "a negative horizon");
    printf("ok %d\n", g_checks);
    return 0;
}
