// What wgs_fisher_stream_push and wgs_fisher_stream_finish refuse before any launch (csrc/fisher_stream_checks.h), driven on the CPU
// under AddressSanitizer + UBSan: every window of a file in windows of 8192 sites is accepted in order and refused out of order, the
// means are given once and only after the last site, every way a window's shape can be wrong is refused with its reason, and the split
// of a window into full chunks and the file's last, shorter chunk.  Prints "ok" and the number of checks; any surprise ends it with
// status 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fisher_stream_checks.h"

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

static void expect_true(bool ok, const char *what)
{
    ++g_checks;
    if (!ok) {
        printf("FAILED: %s\n", what);
        exit(1);
    }
}

int main()
{
    const int64_t A = 8192;
    for (int64_t m_total : {1ll, 100ll, 8192ll, 8193ll, 8199ll, 8200ll, 8321ll, 20000ll, 16384ll, 24576ll, 3 * 8192ll + 63, (1ll << 33) + 5}) {
        for (int64_t W : {A, 2 * A, 1000 * A}) {
            int64_t pushed = 0, full_seen = 0;
            while (pushed < m_total) {
                const int64_t rows = m_total - pushed < W ? m_total - pushed : W;
                expect(fisher_stream_finish_refusal(pushed, m_total, 0, msg, sizeof msg), "sites were pushed", "the means before the last window");
                expect(fisher_stream_window_refusal(pushed, rows, pushed, m_total, A, 0, msg, sizeof msg), nullptr, "a window in its place");
                expect(fisher_stream_window_refusal(pushed, rows, pushed, m_total, A, 1, msg, sizeof msg), "takes no further window", "a window after the means");
                expect(fisher_stream_window_refusal(pushed + A, rows, pushed, m_total, A, 0, msg, sizeof msg), "sites were pushed so far", "a window too far on");
                expect(fisher_stream_window_refusal(pushed + 100, rows, pushed, m_total, A, 0, msg, sizeof msg), "not a multiple of 8192", "an unaligned window");
                if (pushed)
                    expect(fisher_stream_window_refusal(0, rows, pushed, m_total, A, 0, msg, sizeof msg), "sites were pushed so far", "the first window again");
                if (rows > 1 && pushed + rows - 1 < m_total && (rows - 1) % A)
                    expect(fisher_stream_window_refusal(pushed, rows - 1, pushed, m_total, A, 0, msg, sizeof msg), "not the last one", "a ragged middle window");
                if (m_total - pushed < W)
                    expect(fisher_stream_window_refusal(pushed, W, pushed, m_total, A, 0, msg, sizeof msg), "exceed the", "an overrun");
                // the split: full chunks first, and only the file's last window has a rest
                const int64_t full = fisher_stream_full_sites(rows, A);
                expect_true(full % A == 0 && full <= rows && rows - full < A, "full chunks of a window");
                expect_true(rows - full == 0 || pushed + rows == m_total, "a rest outside the last window");
                full_seen += full;
                pushed += rows;
            }
            expect_true(full_seen == m_total / A * A, "the full chunks of all windows are the file's");
            expect(fisher_stream_finish_refusal(pushed, m_total, 0, msg, sizeof msg), nullptr, "the means after the last window");
            expect(fisher_stream_finish_refusal(pushed, m_total, 1, msg, sizeof msg), "finished already", "the means a second time");
            expect(fisher_stream_window_refusal(pushed, 1, pushed, m_total, A, 0, msg, sizeof msg), pushed % A ? "not a multiple of 8192" : "exceed the",
                   "a window past the end");
        }
    }
    // shapes: n individuals in K slabs, none empty, K columns of as many rows as the window
    const int64_t n = 12;
    const int32_t K = 3;
    std::vector<int32_t> cols = {1, 4, 7};
    auto shape = [&](int64_t nw, int32_t groups, int32_t Kaf, int64_t af_rows, int64_t rows) {
        return fisher_stream_shape_refusal(nw, groups, cols.data(), Kaf, af_rows, rows, n, K, msg, sizeof msg);
    };
    expect(shape(n, K, K, 8192, 8192), nullptr, "a good window");
    expect(shape(n, K, K, 100, 100), nullptr, "a short good window");
    expect(shape(n + 1, K, K, 8192, 8192), "13 individuals x 3 populations, the Fisher stream 12 x 3", "another n");
    expect(shape(n, K, K + 1, 8192, 8192), "12 individuals x 4 populations", "another K");
    expect(shape(n, K, K - 1, 8192, 8192), "12 individuals x 2 populations", "a wrong K");
    expect(shape(n, 1, K, 8192, 8192), "has 1 population slabs", "a matrix of one group");
    expect(shape(n, K, K, 0, 0), "an empty window", "no rows");
    expect(shape(n, K, K, 8191, 8192), "allele frequencies cover 8191 SNPs, the window 8192", "frequencies of other rows");
    cols[1] = 0;
    expect(shape(n, K, K, 8192, 8192), "population 1 has no individuals", "an empty population");
    cols[1] = 4;
    cols[2] = 0;
    expect(shape(n, K, K, 8192, 8192), "population 2 has no individuals", "an empty last population");
    cols[2] = 7;
    expect(shape(n, K, K, 8192, 8192), nullptr, "a good window again");
    printf("ok %d\n", g_checks);
    return 0;
}
