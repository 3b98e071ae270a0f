// wgs_em_fit's bookkeeping (wgsassign_amd/csrc/em_fit_ledger.h) on the CPU: a driver that does with EmFitLedger what wgs_em_fit does
// -- sweep t enqueued before the decisions of sweep t-1 are read -- against a model of the device, for scripted fits whose right
// answer is the literal loop of emMAF.py:20-26.  Also prints em_classify / em_chain_converged for tests/test_em_fit_ledger_cpu.py to
// compare with device.py.  Built with -fsanitize=address,undefined; includes nothing of the project but that header.
//   em_fit_ledger_check [<carry bits, hex> <n> <tole>]...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <array>
#include <random>
#include <string>

#include "em_fit_ledger.h"

// what iteration k of a scripted fit gives: the class of its float64 sum and, where that is undecided, the exact chain's verdict
enum Class { GO, CONV, UNDEC_YES, UNDEC_NO, NANSUM, N_CLASSES };
static const EmBand BAND = {1.0, 2.0};
static double sum_of(Class c) { return c == GO ? 3.0 : c == CONV ? 0.5 : c == NANSUM ? NAN : 1.5; }

struct Case {
    int max_iter = 0;
    int fuse_from = 0;                                 // the sweep from which two iterations per sweep are agreed (0: never)
    std::vector<std::vector<Class>> script;            // [fit][k - 1]
    std::vector<uint8_t> active;                       // preset
    std::string text() const
    {
        std::string s = "max_iter " + std::to_string(max_iter) + " fuse_from " + std::to_string(fuse_from);
        for (size_t j = 0; j < script.size(); ++j) {
            s += active[j] ? " | " : " | (inactive) ";
            for (Class c : script[j]) s += "GCYNX"[c];
        }
        return s;
    }
};

static const Case *g_case = nullptr;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "FAILED %s (line %d): ", #cond, __LINE__);          \
            fprintf(stderr, __VA_ARGS__);                                       \
            fprintf(stderr, "\n  case: %s\n", g_case ? g_case->text().c_str() : "-"); \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

// emMAF.py:20-26: the first k <= max_iter that is converged, or undecided with a "yes" from the chain; 0: exhausted
static int expected_iters(const std::vector<Class> &script, int max_iter)
{
    for (int k = 1; k <= max_iter; ++k)
        if (script[k - 1] == CONV || script[k - 1] == UNDEC_YES) return k;
    return 0;
}

// The device: per fit a state, three buffers labelled with the iteration whose result they hold (-1: nothing), the sums of the
// sweep last run.  The driver calls its methods in enqueue order, so each takes effect at its place in that order.
struct Model {
    const Case &c;
    int n;
    std::vector<int32_t> state;
    std::vector<std::array<int, 3>> label;
    std::vector<double> ssq, ssq2;
    std::vector<int> iterations_run, stop_at, listed_after_finish;
    std::vector<char> finished;
    std::vector<int32_t> h_state[2];                   // the read-backs, one per slot
    std::vector<double> h_ssq2[2];

    Model(const Case &cs, const std::vector<int32_t> &init)
        : c(cs), n((int)cs.script.size()), state(init), label(n, {0, -1, -1}), ssq(n, 0.0), ssq2(n, 0.0), iterations_run(n, 0), stop_at(n),
          listed_after_finish(n, 0), finished(n, 0)
    {
        for (int j = 0; j < n; ++j) {
            const int e = expected_iters(c.script[j], c.max_iter);
            stop_at[j] = e ? e : c.max_iter;
        }
    }

    // one listed fit of a sweep and of the decision kernel behind it
    void sweep(int j, int f_old, int f_new, int f_new2, int fuse)
    {
        if (finished[j]) CHECK(++listed_after_finish[j] <= 1, "fit %d listed again after it had finished", j);
        if (state[j] != EM_ACTIVE) return;
        const int k0 = label[j][f_old];
        CHECK(k0 >= 0 && f_new != f_old, "fit %d sweeps from buffer %d, which holds nothing", j, f_old);
        CHECK(k0 + fuse <= c.max_iter, "fit %d runs iteration %d of %d", j, k0 + fuse, c.max_iter);
        label[j][f_new] = k0 + 1;
        ssq[j] = ssq2[j] = sum_of(c.script[j][k0]);
        if (fuse == 2) {
            CHECK(f_new2 != f_old && f_new2 != f_new, "fit %d: the second iteration overwrites a buffer the sweep reads", j);
            label[j][f_new2] = k0 + 2;
            ssq2[j] = sum_of(c.script[j][k0 + 1]);
        } else {
            CHECK(f_new2 == f_new, "fit %d: f_new2 of a one-iteration sweep", j);
        }
        iterations_run[j] += fuse;
        CHECK(iterations_run[j] <= c.max_iter, "fit %d ran %d iterations", j, iterations_run[j]);
        if (k0 + fuse >= stop_at[j]) finished[j] = 1;
        state[j] = em_decide(ssq[j], ssq2[j], fuse, BAND);
    }
    void read_back(int slot)
    {
        h_state[slot] = state;
        h_ssq2[slot] = ssq2;
    }
};

struct Result {
    std::vector<int32_t> iters;
    EmClosing closing;
    int sweeps;                                        // enqueued
};

// What wgs_em_fit does with the ledger (and em_write_descs with the rotation), the device replaced by the model.
static Result run(const Case &c)
{
    g_case = &c;
    const int n = (int)c.script.size();
    std::vector<uint8_t> cur(n, 0), prev(n, 1), pend_cur(n, 0), pend_prev(n, 1), fuse_used(n, 1), active = c.active;     // as wgs_em_create
    Result r;
    r.iters.assign(n, -1);
    EmFitLedger ledger({cur, prev, pend_cur, pend_prev, fuse_used, active}, c.max_iter, r.iters.data());
    Model dev(c, ledger.initial_states());
    std::vector<char> conv;
    r.sweeps = 0;
    for (int t = 1;; ++t) {
        CHECK(t <= 2 * c.max_iter + 3, "sweep %d: the fit does not end", t);
        const int slot = t & 1;
        const bool read_back = ledger.in_flight();
        const std::vector<int32_t> &L = ledger.begin(t);
        CHECK(ledger.in_flight() == !L.empty(), "in_flight");
        if (ledger.in_flight()) {
            // a rank says "I could" once it has the third buffer; the ranks are heard one sweep later and act one sweep after that
            const int nb = c.fuse_from > 0 && t >= c.fuse_from - 2 ? 3 : 2;
            const bool fusing = c.fuse_from > 0 && t >= c.fuse_from;
            int32_t iterations = 0;
            for (int32_t j : L) {
                const int fuse = fusing && ledger.may_fuse()[j] >= 2 ? 2 : 1;
                const EmBuffers first = em_rotate(cur[j], nb, 1), last = em_rotate(cur[j], nb, fuse);
                fuse_used[j] = (uint8_t)fuse;
                pend_cur[j] = last.cur;
                pend_prev[j] = last.prev;
                iterations += fuse;
                dev.sweep(j, cur[j], first.cur, last.cur, fuse);
            }
            CHECK(ledger.iterations_listed() == iterations, "iterations_listed");
            dev.read_back(slot);
            ++r.sweeps;
        }
        if (read_back) {
            const int ps = slot ^ 1;
            ledger.read(dev.h_state[ps].data(), dev.h_ssq2[ps].data(), BAND);
            int batches = 0;
            while (!ledger.batch().empty()) {
                CHECK(++batches <= 2, "a third chain batch");
                const std::vector<int32_t> &B = ledger.batch();
                const bool first_of_two = batches == 1 && dev.h_state[ps][B[0]] == EM_UNDECIDED_A;      // that batch comes first
                CHECK(ledger.batch_iteration() == 2 * t + (first_of_two ? 0 : 1), "batch_iteration %d at sweep %d", ledger.batch_iteration(), t);
                conv.assign(B.size(), 0);
                for (size_t i = 0; i < B.size(); ++i) {
                    const int j = B[i], k = dev.label[j][cur[j]];
                    CHECK(k >= 1 && dev.label[j][prev[j]] == k - 1, "fit %d: the chain is asked about iterations (%d, %d)", j, k,
                          dev.label[j][prev[j]]);
                    const Class cls = c.script[j][k - 1];
                    CHECK(cls == UNDEC_YES || cls == UNDEC_NO, "fit %d: the chain is asked about iteration %d, which is decided", j, k);
                    conv[i] = cls == UNDEC_YES;
                }
                for (const EmStateWrite &w : ledger.resolved(conv)) dev.state[w.fit] = w.state;
            }
        }
        if (!ledger.in_flight()) break;
    }
    ledger.freeze_converged();
    for (int j = 0; j < n; ++j) {
        const int want = c.active[j] ? expected_iters(c.script[j], c.max_iter) : 0;
        CHECK(r.iters[j] == want, "fit %d: %d iterations, the reference's loop has %d", j, r.iters[j], want);
        const int end = !c.active[j] ? 0 : want ? want : c.max_iter;
        CHECK(dev.label[j][cur[j]] == end, "fit %d ends with the frequencies of iteration %d, not %d", j, dev.label[j][cur[j]], end);
        CHECK(active[j] == (c.active[j] && want == 0), "fit %d: active = %d at the end", j, active[j]);
    }
    r.closing = ledger.closing();
    return r;
}

// Two ledgers fed the same case close alike; ledgers whose iteration counts differ close differently (against the case before).
static Result g_before;
static void run_twice(const Case &c)
{
    const Result a = run(c), b = run(c);
    CHECK(a.iters == b.iters && a.closing.sum == b.closing.sum && a.closing.mix == b.closing.mix, "two ledgers, two results");
    if (!g_before.iters.empty() && g_before.iters.size() == a.iters.size() && g_before.iters != a.iters)
        CHECK(g_before.closing.sum != a.closing.sum || g_before.closing.mix != a.closing.mix, "different iterations, same closing pair");
    g_before = a;
}

static long exhaustive_single_fit()
{
    long cases = 0;
    for (int max_iter = 1; max_iter <= 5; ++max_iter) {
        long count = 1;
        for (int k = 0; k < max_iter; ++k) count *= N_CLASSES;
        for (long code = 0; code < count; ++code) {
            Case c;
            c.max_iter = max_iter;
            c.active = {1};
            c.script.assign(1, {});
            for (long k = 0, v = code; k < max_iter; ++k, v /= N_CLASSES) c.script[0].push_back((Class)(v % N_CLASSES));
            c.fuse_from = 0;
            const int sweeps = run(c).sweeps;              // every sweep the fit can reach
            for (c.fuse_from = 0; c.fuse_from <= sweeps; ++c.fuse_from, ++cases) run_twice(c);
        }
    }
    return cases;
}

// Five fits: one preset inactive, one that runs straight into the fused sweeps with an odd number of iterations left (so that it
// ends with a one-iteration sweep unless it stops before), the others random.
static long batches()
{
    std::mt19937 rng(20240607u);
    const Class weighted[10] = {GO, GO, GO, GO, GO, UNDEC_NO, UNDEC_NO, UNDEC_YES, CONV, NANSUM};
    for (int i = 0; i < 2000; ++i) {
        Case c;
        c.max_iter = 7 + (i & 1);
        c.fuse_from = (int)(rng() % 7);
        c.active.assign(5, 1);
        c.active[i % 5] = 0;
        c.script.assign(5, {});
        for (auto &s : c.script)
            for (int k = 0; k < c.max_iter; ++k) s.push_back(weighted[rng() % 10]);
        if (c.fuse_from > 0) {
            if ((c.max_iter - (c.fuse_from - 1)) % 2 == 0) ++c.fuse_from;
            std::vector<Class> &odd = c.script[(i + 1) % 5];
            for (int k = 0; k < c.fuse_from - 1; ++k) odd[k] = GO;
        }
        run_twice(c);
    }
    return 2000;
}

static void print_classify_grid()
{
    const int64_t ms[] = {1, 10000, 10000000, 17000000, 60000000};
    const double toles[] = {0.0, NAN, 1e-4}, guards[] = {0.0, 0.25, 1e9};
    for (int64_t m : ms)
        for (double tole : toles)
            for (double guard : guards) {
                const EmBand b = em_band(tole, m, guard);
                std::vector<double> sums = {0.0, 1e-30, 1.0, NAN, INFINITY};
                for (double edge : {b.lo, b.hi})
                    if (edge > 0 && edge < INFINITY)           // (a sum of squares is never negative)
                        for (double v : {nextafter(edge, 0.0), edge, nextafter(edge, INFINITY), edge * 0.5, edge * 2.0}) sums.push_back(v);
                for (double s : sums) printf("classify %lld %a %a %a %d\n", (long long)m, tole, guard, s, em_classify(s, b));
            }
}

int main(int argc, char **argv)
{
    print_classify_grid();
    for (int i = 1; i + 2 < argc; i += 3) {
        const uint32_t bits = (uint32_t)strtoul(argv[i], nullptr, 16);
        float carry;
        memcpy(&carry, &bits, sizeof carry);
        const long long n = atoll(argv[i + 1]);
        const double tole = strtod(argv[i + 2], nullptr);
        printf("chain %s %lld %s %d\n", argv[i], n, argv[i + 2], em_chain_converged(carry, n, tole) ? 1 : 0);
    }
    const long single = exhaustive_single_fit();
    const long batch = batches();
    printf("ledger: %ld single-fit cases and %ld batches of five agree with the reference's loop\n", single, batch);
    return 0;
}
