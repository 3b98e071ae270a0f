// What wgs_loo_stream_push_scored refuses of the matrix that is scored in place of the fitted window (csrc/loo_stream_checks.h:
// loo_stream_scored_refusal), driven on the CPU under AddressSanitizer + UBSan: the twin of every window of a file is accepted, and
// every way the scored window can differ from the fitted one -- individuals, sites, first site, slabs, the population of any one
// individual -- is refused with its reason.  Prints "ok" and the number of checks; any surprise ends it with status 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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
    const int64_t n = 12;
    const int32_t K = 3;
    const std::vector<int32_t> group_of = {0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2};
    std::vector<int32_t> scored = group_of;
    auto twin = [&](int64_t n_s, int64_t rows_s, int64_t site0_s, int32_t groups_s, int64_t rows, int64_t site0) {
        return loo_stream_scored_refusal(n_s, rows_s, site0_s, groups_s, scored.data(), n, rows, site0, K, group_of.data(), msg, sizeof msg);
    };
    for (int64_t m_total : {1ll, 100ll, 8192ll, 8193ll, 20000ll, 16384ll, 3 * 8192ll + 63, (1ll << 33) + 5}) {
        for (int64_t W : {A, 2 * A, 1000 * A}) {
            for (int64_t site0 = 0; site0 < m_total; site0 += W) {
                const int64_t rows = m_total - site0 < W ? m_total - site0 : W;
                expect(twin(n, rows, site0, K, rows, site0), nullptr, "the window's twin");
                expect(twin(n, rows + 1, site0, K, rows, site0), "sites, the fitted window", "a site more");
                expect(twin(n, rows - 1, site0, K, rows, site0), "sites, the fitted window", "a site fewer");
                expect(twin(n, rows, site0 + A, K, rows, site0), "the fitted window at site", "the window after");
                expect(twin(n, rows, site0 + 1, K, rows, site0), "the fitted window at site", "a site further on");
                if (site0 >= W) expect(twin(n, rows, site0 - W, K, rows, site0), "the fitted window at site", "the window before");
                if (site0 / W > 64) break;      // (the long files: their first windows do)
            }
        }
    }
    expect(twin(n, 100, 0, K, 8192, 0), "the scored window holds 100 sites, the fitted window 8192", "a short window");
    expect(twin(n, 8192, 8192, K, 8192, 0), "the scored window starts at site 8192, the fitted window at site 0", "another first site");
    expect(twin(n + 1, 8192, 0, K, 8192, 0), "the scored window holds 13 individuals, the fitted window 12", "another n");
    expect(twin(n - 1, 8192, 0, K, 8192, 0), "the scored window holds 11 individuals, the fitted window 12", "an individual fewer");
    expect(twin(n, 8192, 0, 1, 8192, 0), "the scored window has 1 population slabs, the fitted window 3", "a matrix of one group");
    expect(twin(n, 8192, 0, K + 1, 8192, 0), "the scored window has 4 population slabs, the fitted window 3", "a slab more");
    // the order of the checks: the first difference is the one that is named, and group_of is read only once the shapes agree
    expect(twin(n + 1, 100, 8192, 1, 8192, 0), "individuals", "everything wrong at once");
    expect(twin(n, 100, 8192, 1, 8192, 0), "sites, the fitted window", "all but n wrong");
    expect(twin(n, 8192, 8192, 1, 8192, 0), "starts at site", "first site and slabs wrong");
    // every individual in every other population
    for (int64_t i = 0; i < n; ++i)
        for (int32_t g = 0; g < K; ++g) {
            scored = group_of;
            scored[i] = g;
            char want[96];
            snprintf(want, sizeof want, "individual %lld is of population %d in the scored window, of population %d in the fitted one", (long long)i, g,
                     group_of[i]);
            expect(twin(n, 8192, 0, K, 8192, 0), g == group_of[i] ? nullptr : want, "one individual regrouped");
        }
    // the same slab sizes in another file order are another grouping
    scored = {2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1};
    expect(twin(n, 8192, 0, K, 8192, 0), "individual 0 is of population 2 in the scored window, of population 0 in the fitted one", "a rotated grouping");
    scored = group_of;
    expect(twin(n, 8192, 0, K, 8192, 0), nullptr, "the twin again");
    printf("ok %d\n", g_checks);
    return 0;
}
