// What wgs_em_stream_push_masked refuses before any launch beyond what every push refuses (csrc/em_stream_masked_checks.h), and the
// room its compacted vectors take, driven on the CPU under AddressSanitizer + UBSan: every way the kept-site set can be wrong is
// refused with its reason, a chain named for an iteration beyond its fit's run_iters is refused by the plan check the masked push
// shares with the others, and the stride is the largest kept count among the fits' slots over enumerated kept counts.  Prints "ok"
// and the number of checks; any surprise ends it with status 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "em_stream_masked_checks.h"

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
    int matrix_a = 0, matrix_b = 0;         // two matrices: only their addresses are compared
    for (int32_t n_fits : {1, 2, 3, 8, 64, 1000}) {
        for (int32_t keep_count : {1, 2, 8, 64, 1000, 4096}) {
            std::vector<int32_t> slot(n_fits);
            for (int32_t j = 0; j < n_fits; ++j) slot[j] = j % keep_count;
            expect(em_stream_masked_refusal(&matrix_a, &matrix_a, n_fits, keep_count, slot.data(), msg, sizeof msg), nullptr, "slots inside the set");
            expect(em_stream_masked_refusal(&matrix_a, &matrix_b, n_fits, keep_count, slot.data(), msg, sizeof msg), "belong to different matrices",
                   "a set of another matrix");
            expect(em_stream_masked_refusal(&matrix_a, &matrix_a, n_fits, keep_count, nullptr, msg, sizeof msg), "needs the slot of every fit",
                   "no slots");
            for (int32_t j : {0, n_fits / 2, n_fits - 1}) {
                const int32_t was = slot[j];
                char want[64];
                slot[j] = keep_count;
                snprintf(want, sizeof want, "fit %d: slot %d outside the kept-site set", j, keep_count);
                expect(em_stream_masked_refusal(&matrix_a, &matrix_a, n_fits, keep_count, slot.data(), msg, sizeof msg), want, "a slot past the set");
                slot[j] = -1;
                snprintf(want, sizeof want, "fit %d: slot -1 outside the kept-site set", j);
                expect(em_stream_masked_refusal(&matrix_a, &matrix_a, n_fits, keep_count, slot.data(), msg, sizeof msg), want, "a negative slot");
                slot[j] = was;
            }
            // the stride: the largest kept count among the slots the fits name, never below 1; a large count in a slot nobody names
            // does not matter
            std::vector<int64_t> kept(keep_count, 0);
            ++g_checks;
            if (em_stream_masked_stride(n_fits, slot.data(), kept.data()) != 1) return printf("FAILED: the stride of fits that kept nothing\n"), 1;
            for (int32_t s = 0; s < keep_count; ++s) kept[s] = (int64_t)(s * 37 % 101) * 83;
            int64_t want = 1;
            for (int32_t j = 0; j < n_fits; ++j) want = kept[slot[j]] > want ? kept[slot[j]] : want;
            ++g_checks;
            if (em_stream_masked_stride(n_fits, slot.data(), kept.data()) != want) return printf("FAILED: the stride of %d fits\n", n_fits), 1;
            if (keep_count > n_fits) {
                kept[keep_count - 1] = (int64_t)1 << 40;
                ++g_checks;
                if (em_stream_masked_stride(n_fits, slot.data(), kept.data()) != want) return printf("FAILED: an unnamed slot set the stride\n"), 1;
            }
            kept[slot[n_fits - 1]] = ((int64_t)1 << 31) + 5;
            ++g_checks;
            if (em_stream_masked_stride(n_fits, slot.data(), kept.data()) != ((int64_t)1 << 31) + 5) return printf("FAILED: a stride beyond 2^31\n"), 1;
        }
    }
    {
        std::vector<int32_t> slot(EM_STREAM_MASKED_MAX_FITS + 1, 0);
        expect(em_stream_masked_refusal(&matrix_a, &matrix_a, EM_STREAM_MASKED_MAX_FITS, 1, slot.data(), msg, sizeof msg), nullptr, "the most fits");
        expect(em_stream_masked_refusal(&matrix_a, &matrix_a, EM_STREAM_MASKED_MAX_FITS + 1, 1, slot.data(), msg, sizeof msg), "holds at most 65535 fits",
               "too many fits for one launch");
    }
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
    expect(em_stream_plan_refusal(n, max_iter, run.data(), nullptr, true, true, 8192, 8192, cf.data(), ci.data(), (int32_t)cf.size(), &T, &any, msg,
                                  sizeof msg),
           nullptr, "every iteration of every fit");
    if (T != 8 || any) return printf("FAILED: T %d any %d\n", T, (int)any), 1;
    for (size_t i = 0; i < cf.size(); ++i) {
        if (cf[i] != 0) continue;
        const int32_t was = ci[i];
        ci[i] = 5;                          // fit 0 runs 4
        const int rc = em_stream_plan_refusal(n, max_iter, run.data(), nullptr, true, true, 8192, 8192, cf.data(), ci.data(), (int32_t)cf.size(), &T,
                                              &any, msg, sizeof msg);
        expect(rc, "iteration 5 of fit 0, which runs 4", "a chain beyond its fit's run_iters");
        ci[i] = was;
    }
    expect(em_stream_plan_refusal(n, max_iter, run.data(), fin.data(), false, true, 8192, 8192, nullptr, nullptr, 0, &T, &any, msg, sizeof msg),
           "final fits need their clamps", "final fits without clamps");
    expect(em_stream_plan_refusal(n, max_iter, run.data(), fin.data(), true, true, 8192, 8192, nullptr, nullptr, 0, &T, &any, msg, sizeof msg), nullptr,
           "the final round");
    printf("ok %d\n", g_checks);
    return 0;
}
