// Every message the windowed streams' pre-launch checks give (csrc/stream_checks.h), one line `stream<TAB>case<TAB>rc<TAB>message` per
// case of stream_cases.h over a small grid; a window is named file sites/window sites@sites pushed.  tests/golden/stream_refusals.tsv
// holds what the checks gave before they were folded into one header -- the same cases with the adapters of stream_cases.h bound to the
// functions of that commit -- and tests/test_stream_refusals_cpu.py compares this program's output with it byte for byte.
#include "stream_cases.h"

int main()
{
    g_dump = "";
    printf("# what commit ed5fb7f, the parent of the one that made csrc/stream_checks.h, refuses; the score stream's lines and the\n"
           "# fit and leave-one-out streams' `sites were pushed` by hand from its format strings, which were inline\n");
    const Sizes files = {1ll, 100ll, 8192ll, 8193ll, 16384ll, 20000ll, 3 * 8192ll + 63}, windows = {A, 2 * A};
    score_cases(files, windows);
    em_cases(files, windows);
    masked_cases({1, 8}, {1, 8});
    loo_cases(files, windows);
    scored_cases({}, {});                   // (no walk: the twin of a window is refused by what differs, wherever the window lies)
    fisher_cases(files, windows);
    return 0;
}
