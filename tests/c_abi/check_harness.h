// What the stand-alone check programs of csrc/stream_checks.h share: the expectations and their counter, the walk over every window of
// a file, the window rule's expectations at one window, and every single and double fault of a shape rule.  With g_dump set (the
// stream's name) every expectation also prints `stream<TAB>case<TAB>rc<TAB>message` (tests/c_abi/stream_refusals_dump.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <vector>

static int g_checks = 0;
static char msg[256];               // what the check under test says
static const char *g_dump = nullptr;
static char g_where[64];            // in a dump: the window a case belongs to, "file sites/window sites@sites pushed "

// rc and message of a refusal: acceptance (part == nullptr), or rc 2 with `part` in the message.  Any surprise ends the program.
static void expect(int rc, const char *part, const char *what)
{
    ++g_checks;
    if (g_dump) printf("%s\t%s%s\t%d\t%s\n", g_dump, g_where, what, rc, rc ? msg : "");
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

static const int64_t A = 8192;      // WGS_WINDOW_ALIGN
typedef std::initializer_list<int64_t> Sizes;
static const Sizes FILES = {1ll, 100ll, 8192ll, 8193ll, 20000ll, 16384ll, 3 * 8192ll + 63, (1ll << 33) + 5}, WINDOWS = {A, 2 * A, 1000 * A};

// visit(m_total, W, pushed, rows) at every window of every file of `files` sites cut into windows of each of `windows` sites, in file
// order; end(m_total, W) after a file's last window.
template <typename Visit, typename End>
static void walk_windows(Sizes files, Sizes windows, Visit visit, End end)
{
    for (int64_t m_total : files)
        for (int64_t W : windows) {
            for (int64_t pushed = 0; pushed < m_total; pushed += W) {
                if (g_dump) snprintf(g_where, sizeof g_where, "%lld/%lld@%lld ", (long long)m_total, (long long)W, (long long)pushed);
                visit(m_total, W, pushed, m_total - pushed < W ? m_total - pushed : W);
            }
            if (g_dump) snprintf(g_where, sizeof g_where, "%lld/%lld@%lld ", (long long)m_total, (long long)W, (long long)m_total);
            end(m_total, W);
            g_where[0] = 0;
        }
}

// The window rule at the window of `rows` sites after `pushed`: window(site0, rows) accepts it in its place and refuses it 8192 sites
// too far on, 100 sites on (unaligned and out of place at once), a site short (ragged) and, where fewer than W sites remain, at W
// sites (an overrun, and ragged at once).  refused: what a stream that takes no window at all says to each of them.
template <typename Window>
static void expect_window_rule(Window window, int64_t m_total, int64_t W, int64_t pushed, int64_t rows, const char *refused = nullptr)
{
    expect(window(pushed, rows), refused, "a window in its place");
    expect(window(pushed + A, rows), refused ? refused : "sites were pushed so far", "a window too far on");
    expect(window(pushed + 100, rows), refused ? refused : "not a multiple of 8192", "an unaligned window");
    if (rows > 1 && pushed + rows - 1 < m_total && (rows - 1) % A)
        expect(window(pushed, rows - 1), refused ? refused : "not the last one", "a ragged middle window");
    if (m_total - pushed < W) expect(window(pushed, W), refused ? refused : "exceed the", "an overrun");
}

// A shape rule's faults, in the order the rule tests them: its name, what the message says, and what it says where the next fault,
// which shares its test, is there too.
struct ShapeFault {
    const char *name, *part, *with_next = nullptr;
};

// shape(mask) has fault f where bit f of mask is set: no fault is accepted; every single fault, and every pair of them, is refused
// with the message of the one the rule tests first.
template <typename Shape>
static void expect_shape_faults(const std::vector<ShapeFault> &faults, Shape shape)
{
    const int n = (int)faults.size();
    char what[96];
    expect(shape(0u), nullptr, "a good window");
    for (int a = 0; a < n; ++a) {
        expect(shape(1u << a), faults[a].part, faults[a].name);
        for (int b = a + 1; b < n; ++b) {
            snprintf(what, sizeof what, "%s + %s", faults[a].name, faults[b].name);
            expect(shape(1u << a | 1u << b), b == a + 1 && faults[a].with_next ? faults[a].with_next : faults[a].part, what);
        }
    }
}
