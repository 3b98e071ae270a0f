"""The EM fit in site windows, the parts that need no GPU: the round scheme of wgsassign_amd/windowed_fit.py driven by a CPU
stand-in (the oracle's own float32 EM update per window, NumPy's serial float32 sum for the chain) gives the oracle's emMAF on the
WHOLE matrix bit for bit -- frequencies and iteration counts; the decision walk on hand-made tables; the fit's byte count per site;
the command line's routing; the new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

import synth
from conftest import ROOT

W = 8192
M, N, K = 20000, 6, 3           # three windows: 8192, 8192, 3616 (the shapes of test_gpu_windowed.py)


class WindowStandIn:
    """windowed_fit's backend on the CPU: S and C as wgs_em_stream keeps them, every window reset to 0.25 and run with
    oracle.emMAF_update, the chain as emMAF_cy.pyx:30-31 continues it (float32, site order) from the carry of the window before."""

    def __init__(self, orc, L, IDs, maf_iter, window=W):
        self.orc, self.maf_iter, self.W = orc, maf_iter, window
        pops = np.unique(IDs[:, 1])
        self.m = L.shape[0]
        self.slabs = [orc.gather(L, np.flatnonzero(IDs[:, 1] == p), 2) for p in pops]
        self.counts = [int(np.sum(IDs[:, 1] == p)) for p in pops]
        self.S = np.zeros((maf_iter, len(pops)))
        self.af = np.full((self.m, len(pops)), np.nan, dtype=np.float32)
        self.plans = []
        self.writes = np.zeros(len(pops), dtype=int)

    def run_round(self, plan):
        self.plans.append(plan)
        C = np.zeros((self.maf_iter, len(self.slabs)), dtype=np.float32)
        chains = set(plan.chains)
        for lo in range(0, self.m, self.W):
            hi = min(self.m, lo + self.W)
            for k, slab in enumerate(self.slabs):
                rows = np.ascontiguousarray(slab[lo:hi])
                f = np.full(hi - lo, 0.25, dtype=np.float32)
                for t in range(1, int(plan.run_iters[k]) + 1):
                    prev = f.copy()
                    self.orc.emMAF_update(rows, f, 2)
                    d = f - prev
                    sq = d * d
                    if plan.add_sums:
                        self.S[t - 1][k] += float(np.sum(sq.astype(np.float64)))
                    if (k, t) in chains:
                        with np.errstate(all="ignore"):
                            C[t - 1][k] = np.cumsum(np.concatenate(([C[t - 1][k]], sq)).astype(np.float32), dtype=np.float32)[-1]
                if plan.final[k]:
                    self.af[lo:hi, k] = self.orc.clamp(f, self.counts[k])
                    self.writes[k] += 1
        return self.S, C


@pytest.fixture(scope="module")
def data(oracle):
    L, IDs = synth.make_beagle(M, N, K, seed=4100 + N)
    ref = {}

    def whole(maf_iter, tole):
        if (maf_iter, tole) not in ref:
            _, af, _, iters = oracle.fit_reference_af(L, IDs, maf_iter, tole, t=2)
            af.setflags(write=False)
            ref[(maf_iter, tole)] = (af, iters)
        return ref[(maf_iter, tole)]
    return L, IDs, whole


def run(oracle, data, maf_iter, tole, guard=0.0, lookahead=None):
    from wgsassign_amd import windowed_fit
    L, IDs, whole = data
    cpu = WindowStandIn(oracle, L, IDs, maf_iter)
    iters, scheme = windowed_fit.fit(cpu, K, maf_iter, tole, M, guard, lookahead)
    af_o, iters_o = whole(maf_iter, tole)
    assert list(iters) == list(iters_o), (list(iters), list(iters_o))
    assert cpu.af.tobytes() == af_o.tobytes()
    assert list(cpu.writes) == [3] * K                      # every column written once per window, never twice
    return scheme, cpu, iters_o


def test_default_band_takes_two_rounds(oracle, data):
    scheme, cpu, iters_o = run(oracle, data, 200, 1e-4)
    assert all(iters_o > 0)
    assert scheme.rounds == 2 and scheme.chain_iterations == 0
    assert cpu.plans[0].add_sums and cpu.plans[0].T == 200 and not cpu.plans[0].chains and not cpu.plans[0].final.any()
    assert not cpu.plans[1].add_sums and list(cpu.plans[1].run_iters) == list(iters_o) and cpu.plans[1].final.all()


def test_every_decision_through_the_chain(oracle, data):
    """GUARD = 1e9: no sum decides, every iteration up to the stopping one is settled by the exact chain, eight per round."""
    from wgsassign_amd import windowed_fit
    scheme, cpu, iters_o = run(oracle, data, 200, 1e-4, guard=1e9)
    t = int(max(iters_o))
    assert scheme.rounds == 1 + -(-t // windowed_fit.CHAIN_LOOKAHEAD) + 1
    assert windowed_fit.CHAIN_LOOKAHEAD == 8 and len(cpu.plans[1].chains) == 8 * K and cpu.plans[1].T == 8
    assert scheme.chain_iterations >= sum(iters_o)
    # one candidate per round: as many chain rounds as the slowest fit has iterations
    scheme1, cpu1, _ = run(oracle, data, 200, 1e-4, guard=1e9, lookahead=1)
    assert scheme1.rounds == 1 + t + 1 and scheme1.rounds > 3
    assert all(len(p.chains) <= K for p in cpu1.plans)


def test_exhausted_fit_reports_zero_and_keeps_the_last_iteration(oracle, data):
    scheme, cpu, iters_o = run(oracle, data, 3, 1e-4)
    assert list(iters_o) == [0] * K and scheme.stop == [3] * K and scheme.rounds == 2
    scheme, _, _ = run(oracle, data, 3, 1e-4, guard=1e9)
    assert scheme.stop == [3] * K and scheme.rounds == 3     # the three iterations' chains all say "goes on"


def test_tolerance_zero_never_converges(oracle, data):
    scheme, cpu, iters_o = run(oracle, data, 5, 0.0)
    assert list(iters_o) == [0] * K and scheme.stop == [5] * K and scheme.rounds == 2 and scheme.chain_iterations == 0


def test_the_decision_walk_edge_for_edge():
    from wgsassign_amd import device, windowed_fit
    from wgsassign_amd.windowed_fit import ACTIVE, CONVERGED, UNDECIDED, RoundPlan, RoundScheme
    m, tole, guard = 100000, 1e-3, 0.25
    thresh = tole * tole * m
    g = device.guard_band(m, guard)
    lo, hi = thresh * (1 - g), thresh * (1 + g)
    # the three classes at the band's edges, as em_classify has them
    assert windowed_fit.classify(np.nextafter(lo, 0), m, tole, guard) == CONVERGED
    assert windowed_fit.classify(lo, m, tole, guard) == UNDECIDED
    assert windowed_fit.classify(np.nextafter(hi, 0), m, tole, guard) == UNDECIDED
    assert windowed_fit.classify(hi, m, tole, guard) == ACTIVE
    assert windowed_fit.classify(float("nan"), m, tole, guard) == ACTIVE
    assert windowed_fit.classify(0.0, m, 0.0, guard) == ACTIVE
    A, U, Cv = 10 * hi, thresh, lo / 10
    yes = np.float32(thresh * 0.5)       # a carry whose chain_diff is below tole
    no = np.float32(thresh * 2.0)
    assert device.chain_diff(yes, m) < tole <= device.chain_diff(no, m)
    T = 12

    def scheme(cols, lookahead=None):
        s = RoundScheme(len(cols), T, tole, m, guard, lookahead)
        S = np.array(cols, dtype=np.float64).T.copy()
        p = s.plan()
        assert p.add_sums and p.T == T and p.number == 1
        s.after_round(p, S, np.zeros((T, len(cols)), dtype=np.float32))
        return s, S
    # fit 0: the sums decide (stop 4); fit 1: undecided at 3, then candidates 3, 4 (5 is ruled out by its sum), 6, 7 = first converged;
    # fit 2: never below the band: exhausted; fit 3: undecided from 2 on: eight candidates 2..9
    cols = [[A, A, A, Cv] + [Cv] * 8,
            [A, A, U, U, A, U, Cv] + [Cv] * 5,
            [A] * T,
            [A] + [U] * 11]
    s, S = scheme(cols)
    assert s.stop == [4, None, T, None] and list(s.iters) == [4, 0, 0, 0]
    assert s.ruled_out[:2] == [3, 2] and s.ruled_out[3] == 1
    assert s.chain == [[], [3, 4, 6, 7], [], [2, 3, 4, 5, 6, 7, 8, 9]]
    p = s.plan()
    assert list(p.run_iters) == [4, 7, T, 9] and list(p.final) == [1, 0, 1, 0] and not p.add_sums
    assert p.chains == [(3, 2), (1, 3), (3, 3), (1, 4), (3, 4), (3, 5), (1, 6), (3, 6), (1, 7), (3, 7), (3, 8), (3, 9)]
    # round 2: fit 1's chains say no at 3, yes at 4 (6 and 7 are never looked at); fit 3's say no eight times
    C = np.full((T, 4), np.nan, dtype=np.float32)
    C[2][1], C[3][1] = no, yes
    C[1:9, 3] = no
    s.after_round(p, S, C)
    assert s.written == [True, False, True, False]
    assert s.stop == [4, 4, T, None] and list(s.iters) == [4, 4, 0, 0]
    assert s.ruled_out[3] == 9 and s.chain[3] == [10, 11, 12] and s.chain_iterations == 12
    p = s.plan()
    assert list(p.run_iters) == [0, 4, 0, 12] and list(p.final) == [0, 1, 0, 0] and p.chains == [(3, 10), (3, 11), (3, 12)]
    # round 3: the walk of fit 3 passes maf_iter without a stop
    C = np.full((T, 4), np.nan, dtype=np.float32)
    C[9:12, 3] = no
    s.after_round(p, S, C)
    assert s.stop == [4, 4, T, T] and list(s.iters) == [4, 4, 0, 0] and not s.done()
    p = s.plan()
    assert list(p.run_iters) == [0, 0, 0, T] and list(p.final) == [0, 0, 0, 1] and not p.chains
    s.after_round(p, S, C)
    assert s.done() and s.rounds == 4
    # a lookahead of one: only the first undecided iteration
    s1, _ = scheme(cols, lookahead=1)
    assert s1.chain == [[], [3], [], [2]]
    # an undecided iteration that was chained and converged stops the fit although a LATER sum says converged too
    s2, S2 = scheme([[A, U, Cv] + [Cv] * 9])
    assert s2.chain == [[2, 3]]
    C = np.zeros((T, 1), dtype=np.float32)
    C[1][0] = yes
    s2.after_round(s2.plan(), S2, C)
    assert s2.stop == [2] and list(s2.iters) == [2]
    # maf_iter 0: nothing to decide, one round writes 0.25 clamped
    s0 = RoundScheme(2, 0, tole, m)
    p = s0.plan()
    assert list(p.run_iters) == [0, 0] and list(p.final) == [1, 1] and not p.add_sums
    s0.after_round(p, np.zeros((0, 2)), np.zeros((0, 2), dtype=np.float32))
    assert s0.done() and list(s0.iters) == [0, 0]
    assert isinstance(p, RoundPlan)


def test_fit_bytes_per_site_on_made_up_numbers():
    from wgsassign_amd import windows
    n, K = 200, 5
    counts = [40] * 5
    per_site = 16 * 100 + 8 * 5 + 1 + (1 + 2032 + 8) + 8 * 50 + 5 * 2033
    assert windows.fit_site_bytes(n, K, counts) == per_site == 14247
    assert windows.fit_site_bytes(n, K) == per_site + 16 * 2 + 8 * 3          # the worst split: (n + K) // 2 pairs, (n + 3K) // 4 quads
    assert windows.fit_site_bytes(7, 3, [3, 2, 2]) == 16 * 4 + 24 + 1 + 2041 + 8 * 3 + 3 * 2033
    assert windows.fit_site_bytes(n, K, counts) > windows.site_bytes(n, K)     # a fit needs more than scoring
    GiB = 1 << 30
    fits = 76 * GiB // per_site
    assert windows.plan_fit(fits, n, K, 100 * GiB, {}, counts) is None
    Wf = windows.plan_fit(fits + 1, n, K, 100 * GiB, {}, counts)
    assert Wf == 76 * GiB // (2 * per_site) // 8192 * 8192 and Wf % 8192 == 0
    assert 2 * Wf * per_site <= 76 * GiB < 2 * (Wf + 8192) * per_site
    assert windows.plan_fit(10, n, K, 1 << 40, {windows.ENV: "20000"}) == 16384
    with pytest.raises(MemoryError, match="two windows of 8192 sites"):
        windows.plan_fit(10_000_000, n, K, 64 << 20, {})
    # scoring's own numbers are as they were
    assert windows.site_bytes(n, K) == 3861 and windows.plan(1_000_000, n, K, 100 * GiB, {}) is None


def _args(*argv):
    from wgsassign_amd import WGSassign
    return WGSassign.parser.parse_args(list(argv))


def test_command_line_routing():
    from wgsassign_amd import WGSassign
    from wgsassign_amd.WGSassign import windowed_candidate, windowed_fit_candidate
    base = ("--beagle", "x.beagle.gz", "--pop_af_IDs", "ids.txt", "--get_reference_af")
    assert windowed_fit_candidate(_args(*base), 1)
    assert windowed_fit_candidate(_args(*base, "--threads", "8", "--out", "y", "--maf_iter", "50", "--maf_tole", "1e-5"), 1)
    assert not windowed_fit_candidate(_args(*base), 2)
    assert not windowed_fit_candidate(_args("--beagle", "x.beagle.gz"), 1)
    for other in (("--loo",), ("--ne_obs",), ("--get_pop_like", "--pop_af_file", "a.npy"), ("--get_assignment_z_score",),
                  ("--get_reference_z_score",), ("--loo", "--loo_downsampled_beagle", "d.beagle.gz")):
        assert not windowed_fit_candidate(_args(*base, *other), 1), other
        assert not windowed_candidate(_args(*base, *other), 1), other
    # scoring's routing answers as before
    assert not windowed_candidate(_args(*base), 1)
    score = ("--beagle", "x.beagle.gz", "--pop_af_file", "x.npy", "--get_pop_like")
    assert windowed_candidate(_args(*score), 1) and not windowed_fit_candidate(_args(*score), 1)
    assert "fit the file in site windows" in WGSassign.SET_WINDOW_SITES_FIT and "score the file" in WGSassign.SET_WINDOW_SITES
    assert WGSassign.WINDOWS_ONLY == "windowed scoring (WGSASSIGN_WINDOW_SITES) covers --get_pop_like on one rank only"


def test_the_variable_routes_the_fit_and_a_missing_id_file_does_not(monkeypatch, tmp_path):
    from wgsassign_amd import WGSassign

    class OneRank:
        world = 1
    ids = tmp_path / "ids.txt"
    ids.write_text("a\tp\nb\tq\n")
    monkeypatch.setenv("WGSASSIGN_WINDOW_SITES", "20000")
    assert WGSassign._fit_window_sites(_args("--beagle", "x.gz", "--pop_af_IDs", str(ids), "--get_reference_af"), OneRank(), None) == 16384
    assert WGSassign._fit_window_sites(_args("--beagle", "x.gz", "--pop_af_IDs", str(ids), "--get_reference_af", "--loo"), OneRank(), None) is None
    assert WGSassign._fit_window_sites(_args("--beagle", "x.gz", "--pop_af_IDs", str(tmp_path / "no.txt"), "--get_reference_af"), OneRank(), None) is None
    monkeypatch.setenv("WGSASSIGN_WINDOW_SITES", "100")
    with pytest.raises(SystemExit, match="WGSASSIGN_WINDOW_SITES"):
        WGSassign._fit_window_sites(_args("--beagle", "x.gz", "--pop_af_IDs", str(ids), "--get_reference_af"), OneRank(), None)


def test_new_symbols_are_declared_bound_and_exported():
    from wgsassign_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wgsassign_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wgs_[a-z0-9_]+)\s*\(", text))
    build.build()
    lib = _lib.load()
    for name in ("wgs_em_stream_create", "wgs_em_stream_push", "wgs_em_stream_read", "wgs_em_stream_move_window", "wgs_em_stream_destroy"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name


def test_push_checks_under_the_sanitizers(tmp_path):
    """csrc/stream_checks.h is host-only: the `em` part of tests/c_abi/stream_checks_check.cpp drives what wgs_em_stream_push refuses,
    under AddressSanitizer + UBSan, as a program of its own."""
    import sanitized
    r = sanitized.run(tmp_path, "stream_checks_check.cpp", "em")
    assert r.returncode == 0 and r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 100, (r.stdout[-2000:], r.stderr[-3000:])
