// What the windowed streams refuse before any launch (csrc/stream_checks.h), driven on the CPU under AddressSanitizer + UBSan: the
// cases of stream_cases.h over every window of files of up to 2^33 + 5 sites.  Runs the parts named on the command line, or all of
// them; prints "ok" and the number of checks; any surprise ends it with status 1.
#include <algorithm>

#include "stream_cases.h"

int main(int argc, char **argv)
{
    auto wanted = [&](const char *part) { return argc < 2 || std::any_of(argv + 1, argv + argc, [&](const char *a) { return !strcmp(a, part); }); };
    if (wanted("score")) score_cases(FILES, WINDOWS);
    if (wanted("em")) em_cases(FILES, WINDOWS);
    if (wanted("masked")) masked_cases({1, 2, 3, 8, 64, 1000}, {1, 2, 8, 64, 1000, 4096});
    if (wanted("loo")) loo_cases(FILES, WINDOWS);
    if (wanted("scored")) scored_cases(FILES, WINDOWS);
    if (wanted("fisher")) fisher_cases({1ll, 100ll, 8192ll, 8193ll, 8199ll, 8200ll, 8321ll, 20000ll, 16384ll, 24576ll, 3 * 8192ll + 63, (1ll << 33) + 5}, WINDOWS);
    printf("ok %d\n", g_checks);
    return 0;
}
