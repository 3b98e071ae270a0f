// What wgs_em_stream_push refuses before any launch (csrc/em_stream_checks.h), driven on the CPU under AddressSanitizer + UBSan:
// every window of every round of a file in windows of 8192 sites is accepted in order and refused out of order, and every way a
// plan can be wrong is refused with its reason.  Prints "ok" and the number of checks; any surprise ends it with status 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "em_stream_checks.h"

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
                expect(em_stream_window_refusal(pushed, rows, W, pushed, m_total, A, msg, sizeof msg), nullptr, "a window in its place");
                expect(em_stream_window_refusal(pushed + A, rows, W, pushed, m_total, A, msg, sizeof msg), "sites were pushed so far", "a window too far on");
                expect(em_stream_window_refusal(pushed + 100, rows, W, pushed, m_total, A, msg, sizeof msg), "not a multiple of 8192", "an unaligned window");
                expect(em_stream_window_refusal(pushed, W + 1, W, pushed, m_total, A, msg, sizeof msg), "in a batch made for", "more rows than the batch holds");
                expect(em_stream_window_refusal(pushed, 0, W, pushed, m_total, A, msg, sizeof msg), "in a batch made for", "an empty window");
                if (rows > 1 && pushed + rows - 1 < m_total && (rows - 1) % A)
                    expect(em_stream_window_refusal(pushed, rows - 1, W, pushed, m_total, A, msg, sizeof msg), "not the last one", "a ragged middle window");
                if (m_total - pushed < W)
                    expect(em_stream_window_refusal(pushed, W, W, pushed, m_total, A, msg, sizeof msg), "exceed the", "an overrun");
                pushed += rows;
            }
        }
    }
    // plans
    const int n = 3, max_iter = 10;
    std::vector<int32_t> run = {5, 10, 0}, fin = {0, 1, 1}, cf = {0, 1, 0, 1}, ci = {1, 1, 5, 10};
    int32_t T = -1;
    bool any = false;
    auto plan = [&](const int32_t *f, bool clamps, bool out, int64_t stride, int nc) {
        return em_stream_plan_refusal(n, max_iter, run.data(), f, clamps, out, stride, 8192, cf.data(), ci.data(), nc, &T, &any, msg, sizeof msg);
    };
    expect(plan(fin.data(), true, true, 8192, 4), nullptr, "a good plan");
    if (T != 10 || !any) return printf("FAILED: T %d any %d\n", T, (int)any), 1;
    expect(plan(nullptr, false, false, 0, 0), nullptr, "no final fits, no chains");
    if (any) return printf("FAILED: any_final without final\n"), 1;
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
    printf("ok %d\n", g_checks);
    return 0;
}
