"""The leave-one-out run in site windows, the parts that need no GPU: the round scheme of wgsassign_amd/windowed_fit.py with per-fit
horizons and held-back finals, driven by a CPU stand-in (the oracle's own float32 EM update per window, NumPy's serial float32 sum for
the chains, np.sum's running float64 total per 8192 sites, serial float32 partition carries), gives oracle.loo on the WHOLE matrix bit
for bit -- log-likelihoods, partition sums and iteration counts; the horizon walk on hand-made tables; the byte count per site; the
command line's routing; the new C-ABI symbols and the host-only push checks."""
import os
import re

import numpy as np
import pytest

import synth
from conftest import ROOT

W = 8192
M, N, K, P = 20000, 6, 3, 3         # three windows: 8192, 8192, 3616; populations interleaved in file order


class LooStandIn:
    """windowed_fit's backend on the CPU for the n re-fits: S as wgs_em_stream keeps it (zeroed once, sums added above sums_from),
    every window reset to 0.25 and run with oracle.emMAF_update; in a round whose fits are final the window is scored as
    wgs_loo_stream_push scores it."""

    def __init__(self, orc, L, IDs, af, maf_iter, window=W):
        self.orc, self.L, self.af, self.maf_iter, self.W = orc, L, af, maf_iter, window
        pops = np.unique(IDs[:, 1])
        self.group_of = np.searchsorted(pops, IDs[:, 1])
        self.n, self.m = len(self.group_of), L.shape[0]
        self.slabs, self.counts = [], []
        for i in range(self.n):
            others = np.flatnonzero((self.group_of == self.group_of[i]) & (np.arange(self.n) != i))
            self.slabs.append(orc.gather(L, others, 2))
            self.counts.append(len(others))
        self.S = np.zeros((maf_iter, self.n))
        self.entered = np.zeros((-(-self.m // window), maf_iter, self.n), dtype=int)
        self.total = np.zeros((self.n, K))
        self.parts = np.zeros((self.n, P, K), dtype=np.float32)
        self.plans = []
        self.finals = np.zeros((self.entered.shape[0], self.n), dtype=int)

    def run_round(self, plan):
        self.plans.append(plan)
        C = np.zeros((self.maf_iter, self.n), dtype=np.float32)
        chains = set(plan.chains)
        for w, lo in enumerate(range(0, self.m, self.W)):
            hi = min(self.m, lo + self.W)
            fits = []
            for k, slab in enumerate(self.slabs):
                rows = np.ascontiguousarray(slab[lo:hi])
                f = np.full(hi - lo, 0.25, dtype=np.float32)
                for t in range(1, int(plan.run_iters[k]) + 1):
                    prev = f.copy()
                    self.orc.emMAF_update(rows, f, 2)
                    d = f - prev
                    sq = d * d
                    if plan.add_sums and t > plan.sums_from[k]:
                        self.S[t - 1][k] += float(np.sum(sq.astype(np.float64)))
                        self.entered[w][t - 1][k] += 1
                    if (k, t) in chains:
                        with np.errstate(all="ignore"):
                            C[t - 1][k] = np.cumsum(np.concatenate(([C[t - 1][k]], sq)).astype(np.float32), dtype=np.float32)[-1]
                if plan.final[k]:
                    fits.append(self.orc.clamp(f, self.counts[k]))
                    self.finals[w][k] += 1
            if plan.final.any():
                assert plan.final.all()
                self.score(lo, hi, fits)
        return self.S, C

    def score(self, lo, hi, fits):
        """glassy.py:87-109 on the window's rows: the sticky overwrite, np.sum's total continued chunk by chunk, the partition sums
        continued serially in float32 with labels from the window's first site."""
        rows = np.ascontiguousarray(self.L[lo:hi])
        cur = np.ascontiguousarray(self.af[lo:hi]).copy()
        labels = (lo + np.arange(hi - lo)) % P
        with np.errstate(all="ignore"):
            for i in range(self.n):
                cur[:, self.group_of[i]] = fits[i]
                for k in range(K):
                    vec = np.zeros(hi - lo, dtype=np.float32)
                    self.orc.loglike(rows, cur, vec, 2, i, k)
                    for c in range(0, hi - lo, 8192):
                        self.total[i, k] += np.sum(vec[c:c + 8192], dtype=float)
                    carry = self.parts[i, :, k].copy()
                    np.add.at(carry, labels, vec)
                    self.parts[i, :, k] = carry


@pytest.fixture(scope="module")
def data(oracle):
    L, IDs = synth.make_beagle(M, N, K, seed=4100 + N, interleave=True)
    assert len(set(IDs[:3, 1])) == 3                    # interleaved: the sticky columns matter
    ref = {}

    def whole(maf_iter, tole):
        if (maf_iter, tole) not in ref:
            _, af, _, pop_iters = oracle.fit_reference_af(L, IDs, maf_iter, tole, t=2)
            af.setflags(write=False)
            logl, parts = oracle.loo(L, af.copy(), IDs, 2, maf_iter, tole, num_partitions=P)
            iters = []
            for i in range(N):
                others = np.flatnonzero((IDs[:, 1] == IDs[i, 1]) & (np.arange(N) != i))
                iters.append(int(oracle.emMAF(oracle.gather(L, others, 2), maf_iter, tole, 2)[1]))
            ref[(maf_iter, tole)] = (af, pop_iters, logl, parts, iters)
        return ref[(maf_iter, tole)]
    return L, IDs, whole


def run(oracle, data, maf_iter=200, tole=1e-4, guard=0.0, first_iters=None):
    from wgsassign_amd import windowed_fit
    L, IDs, whole = data
    af, pop_iters, logl_o, parts_o, iters_o = whole(maf_iter, tole)
    if callable(first_iters):
        first_iters = first_iters(pop_iters, iters_o)
    cpu = LooStandIn(oracle, L, IDs, af, maf_iter)
    iters, scheme = windowed_fit.fit(cpu, N, maf_iter, tole, M, guard, first_iters=first_iters, hold_final=True)
    with np.errstate(over="ignore"):
        logl = cpu.total.astype(np.float32)
    assert list(iters) == iters_o, (list(iters), iters_o)
    assert logl.tobytes() == logl_o.tobytes()
    assert cpu.parts.reshape(N * P, K).tobytes() == parts_o.tobytes()
    # the scheme, whatever the order of the fits: every sum entered S once, nothing final before the last round, final once per window
    for k in range(N):
        assert (cpu.entered[:, :scheme.summed[k], k] == 1).all() and (cpu.entered[:, scheme.summed[k]:, k] == 0).all(), k
    assert all(not p.final.any() for p in cpu.plans[:-1]) and cpu.plans[-1].final.all()
    assert (cpu.finals == 1).all()
    return scheme, cpu, iters_o


def test_whole_first_round(oracle, data):
    """first_iters=None: round 1 runs maf_iter iterations, the sums decide, one more round scores."""
    scheme, cpu, iters_o = run(oracle, data)
    assert all(i > 0 for i in iters_o)
    assert scheme.rounds == 2 and scheme.chain_iterations == 0 and scheme.extension_rounds == 0
    assert scheme.iterations_round1 == 200 * N and list(cpu.plans[0].run_iters) == [200] * N
    assert list(cpu.plans[1].run_iters) == iters_o


def test_horizons_at_the_exact_stops(oracle, data):
    scheme, cpu, iters_o = run(oracle, data, first_iters=lambda pop, own: own)
    assert scheme.rounds == 2 and scheme.extension_rounds == 0 and scheme.iterations_round1 == sum(iters_o)


def test_horizons_from_the_population_fits(oracle, data):
    """What glassy.loo_windowed does with pop_iters: the population's stop plus the margin."""
    from wgsassign_amd import glassy
    L, IDs, whole = data
    group_of = np.searchsorted(np.unique(IDs[:, 1]), IDs[:, 1])
    assert glassy.LOO_MARGIN >= 1
    assert glassy.loo_first_iters([0, 1, 1], [12, 0], 50, margin=4) == [16, 50, 50]
    assert glassy.loo_first_iters([0, 1], [48, 7], 50, margin=4) == [50, 11]
    scheme, cpu, iters_o = run(oracle, data, first_iters=lambda pop, own: glassy.loo_first_iters(group_of, pop, 200))
    print("population stops", list(whole(200, 1e-4)[1]), "re-fit stops", iters_o, "rounds", scheme.rounds, "extension rounds", scheme.extension_rounds)
    assert scheme.iterations_round1 < 200 * N
    assert scheme.rounds == 2 + scheme.extension_rounds


def test_horizons_of_one_force_extension_rounds(oracle, data):
    scheme, cpu, iters_o = run(oracle, data, first_iters=[1] * N)
    assert scheme.extension_rounds > 0 and scheme.iterations_round1 == N
    # 1, 2, 4, ... until the horizon covers the stop
    assert scheme.extension_rounds == int(np.ceil(np.log2(max(iters_o))))
    assert all(p.add_sums for p in cpu.plans[:-1]) and not cpu.plans[-1].add_sums
    assert list(cpu.plans[1].sums_from) == [1] * N and list(cpu.plans[1].run_iters) == [2] * N


def test_every_decision_through_the_chain(oracle, data):
    scheme, cpu, iters_o = run(oracle, data, guard=1e9)
    assert scheme.chain_iterations >= sum(iters_o) and scheme.rounds == 1 + -(-max(iters_o) // 8) + 1
    # chains and horizons together: the candidates stay inside the horizon, the rest follows in extension rounds
    scheme, cpu, _ = run(oracle, data, guard=1e9, first_iters=[5] * N)
    assert scheme.extension_rounds > 0 and scheme.chain_iterations >= sum(iters_o)
    for p in cpu.plans:
        assert all(t <= p.run_iters[k] for k, t in p.chains)


def test_exhausted(oracle, data):
    scheme, cpu, iters_o = run(oracle, data, maf_iter=3)
    assert iters_o == [0] * N and scheme.stop == [3] * N and scheme.rounds == 2
    scheme, cpu, iters_o = run(oracle, data, maf_iter=3, first_iters=[1] * N)
    assert scheme.stop == [3] * N and scheme.extension_rounds == 2         # horizons 1, 2, 3 (capped)


def test_the_horizon_walk_edge_for_edge():
    from wgsassign_amd import device
    from wgsassign_amd.windowed_fit import RoundScheme
    m, tole, guard = 100000, 1e-3, 0.25
    thresh = tole * tole * m
    g = device.guard_band(m, guard)
    lo, hi = thresh * (1 - g), thresh * (1 + g)
    A, U, Cv = 10 * hi, thresh, lo / 10
    yes, no = np.float32(thresh * 0.5), np.float32(thresh * 2.0)
    T = 12
    NaN = float("nan")          # cells no round has summed: never looked at
    # fit 0 converges AT its horizon 4; fit 1 is undecided at its horizon 3 (the candidates do not reach past it);
    # fit 2 is active at its horizon 5: extension to 10, then 12 (capped), then exhausted; fit 3 stops inside its horizon
    s = RoundScheme(4, T, tole, m, guard, first_iters=[4, 3, 5, 6], hold_final=True)
    assert s.iterations_round1 == 18
    p = s.plan()
    assert list(p.run_iters) == [4, 3, 5, 6] and p.add_sums and list(p.sums_from) == [0] * 4 and not p.final.any() and not p.chains
    S = np.full((T, 4), NaN)
    S[:4, 0] = [A, A, A, Cv]
    S[:3, 1] = [A, A, U]
    S[:5, 2] = [A] * 5
    S[:6, 3] = [A, Cv, Cv, Cv, Cv, Cv]
    s.after_round(p, S, np.zeros((T, 4), dtype=np.float32))
    assert s.stop == [4, None, None, 2] and s.summed == [4, 3, 5, 6]
    assert s.chain == [[], [3], [], []] and s.extend == [False, False, True, False] and s.horizon[2] == 10
    p = s.plan()        # nothing final yet; fit 1 chained to 3 without sums, fit 2 summed above 5
    assert list(p.run_iters) == [0, 3, 10, 0] and not p.final.any() and p.chains == [(1, 3)] and p.add_sums
    assert list(p.sums_from) == [0, 3, 5, 0]
    S[5:10, 2] = [A] * 5
    C = np.full((T, 4), NaN, dtype=np.float32)
    C[2][1] = no
    s.after_round(p, S, C)
    assert s.extension_rounds == 1 and s.summed == [4, 3, 10, 6]
    assert s.stop == [4, None, None, 2] and s.extend == [False, True, True, False] and s.horizon[1:3] == [6, 12]      # past its chain: extension
    p = s.plan()
    assert list(p.run_iters) == [0, 6, 12, 0] and list(p.sums_from) == [0, 3, 10, 0] and not p.chains and not p.final.any()
    S[3:6, 1] = [U, Cv, Cv]
    S[10:12, 2] = [A, A]
    s.after_round(p, S, C)
    assert s.stop == [4, None, T, 2] and list(s.iters) == [4, 0, 0, 2] and s.chain[1] == [4, 5] and s.extension_rounds == 2
    p = s.plan()
    assert list(p.run_iters) == [0, 5, 0, 0] and p.chains == [(1, 4), (1, 5)] and not p.add_sums and not p.final.any()
    C[3][1] = yes
    s.after_round(p, S, C)
    assert s.stop == [4, 4, T, 2] and not s.done()
    p = s.plan()
    assert list(p.run_iters) == [4, 4, T, 2] and p.final.all() and not p.add_sums and not p.chains
    s.after_round(p, S, C)
    assert s.done() and s.rounds == 5 and list(s.iters) == [4, 4, 0, 2]


def test_no_horizons_reproduce_the_plans_of_the_population_scheme():
    from wgsassign_amd.windowed_fit import RoundScheme
    m, tole, T = 100000, 1e-3, 12
    thresh = tole * tole * m
    A, U, Cv = 100 * thresh, thresh, thresh / 100
    cols = [[A, A, A, Cv] + [Cv] * 8, [A, A, U, U, A, U, Cv] + [Cv] * 5, [A] * T, [A] + [U] * 11]
    S = np.array(cols, dtype=np.float64).T.copy()
    C = np.full((T, 4), np.float32(thresh * 2.0), dtype=np.float32)
    old, new = RoundScheme(4, T, tole, m, 0.25), RoundScheme(4, T, tole, m, 0.25, first_iters=None, hold_final=False)
    rounds = 0
    while not old.done():
        po, pn = old.plan(), new.plan()
        assert (list(po.run_iters), list(po.final), po.chains, po.add_sums, po.number) == (list(pn.run_iters), list(pn.final), pn.chains, pn.add_sums, pn.number)
        assert list(pn.sums_from) == [0] * 4
        old.after_round(po, S, C), new.after_round(pn, S, C)
        rounds += 1
    assert new.done() and rounds == 4 and new.extension_rounds == 0 and new.summed == [T] * 4
    # first_iters = maf_iter everywhere is the same scheme too
    full = RoundScheme(4, T, tole, m, 0.25, first_iters=[T] * 4)
    assert list(full.plan().run_iters) == [T] * 4


def test_loo_bytes_per_site_on_made_up_numbers():
    from wgsassign_amd import windows
    n, K = 200, 5
    counts = [40] * 5
    fit = windows.fit_site_bytes(n, K, counts)
    assert fit == 14247
    cells = n * K
    per_site = fit - 8 * K - 1 + 8 * n + 25 + 4 * K + 2 + 1 + 1
    assert (8 * cells + 4095) // 4096 == 2 and (8 * cells + 8191) // 8192 == 1 and (4 * cells + 4095) // 4096 == 1
    assert windows.loo_site_bytes(n, K, counts) == per_site == 15855
    assert windows.loo_site_bytes(n, K, counts, P=5) == per_site + 4
    assert windows.loo_site_bytes(n, K, counts) > windows.fit_site_bytes(n, K, counts)
    assert windows.loo_site_bytes(n, K) > windows.fit_site_bytes(n, K)
    GiB = 1 << 30
    fits = 76 * GiB // fit          # the resident run needs the matrix only: it batches its re-fits by what is left
    assert windows.plan_loo(fits, n, K, 100 * GiB, {}, counts) is None
    Wl = windows.plan_loo(fits + 1, n, K, 100 * GiB, {}, counts)
    assert Wl == 76 * GiB // (2 * per_site) // 8192 * 8192 and Wl % 8192 == 0
    assert 2 * Wl * per_site <= 76 * GiB < 2 * (Wl + 8192) * per_site
    assert windows.plan_loo(10, n, K, 1 << 40, {windows.ENV_LOO: "20000"}) == 16384
    assert windows.plan_loo(10, n, K, 1 << 40, {windows.ENV: "20000"}) is None          # the fit's variable routes no leave-one-out run
    with pytest.raises(MemoryError, match="two windows of 8192 sites"):
        windows.plan_loo(10_000_000, n, K, 64 << 20, {})


def _args(*argv):
    from wgsassign_amd import WGSassign
    return WGSassign.parser.parse_args(list(argv))


def test_command_line_routing():
    from wgsassign_amd.WGSassign import windowed_candidate, windowed_fit_candidate, windowed_loo_candidate
    base = ("--beagle", "x.beagle.gz", "--pop_af_IDs", "ids.txt", "--get_reference_af", "--loo")
    assert windowed_loo_candidate(_args(*base), 1)
    assert windowed_loo_candidate(_args(*base, "--partition_sites", "7", "--threads", "8", "--maf_iter", "50"), 1)
    assert not windowed_loo_candidate(_args(*base), 2)
    assert not windowed_loo_candidate(_args(*base[:-1]), 1)                                       # no --loo: the fit's own route
    assert not windowed_loo_candidate(_args("--beagle", "x.beagle.gz", "--loo"), 1)               # no --get_reference_af
    for other in (("--ne_obs",), ("--get_pop_like", "--pop_af_file", "a.npy"), ("--get_assignment_z_score",), ("--get_reference_z_score",),
                  ("--loo_downsampled_beagle", "d.beagle.gz")):
        assert not windowed_loo_candidate(_args(*base, *other), 1), other
    # the two routes before this one answer as they did
    assert not windowed_fit_candidate(_args(*base), 1) and not windowed_candidate(_args(*base), 1)
    assert windowed_fit_candidate(_args(*base[:-1]), 1)


def test_only_its_own_variable_routes_the_run(monkeypatch, tmp_path):
    from wgsassign_amd import WGSassign

    class OneRank:
        world = 1
    ids = tmp_path / "ids.txt"
    ids.write_text("a\tp\nb\tq\n")
    argv = ("--beagle", "x.gz", "--pop_af_IDs", str(ids), "--get_reference_af", "--loo")
    monkeypatch.delenv("WGSASSIGN_LOO_WINDOW_SITES", raising=False)
    monkeypatch.setenv("WGSASSIGN_WINDOW_SITES", "20000")
    assert WGSassign._fit_window_sites(_args(*argv), OneRank(), None) is None
    monkeypatch.setattr(WGSassign.os.path, "getsize", lambda p: 1)                  # (the first look: a file that surely fits)

    class Ctx:
        def mem_info(self):
            return 100 << 30, 100 << 30
    assert WGSassign._loo_window_sites(_args(*argv), OneRank(), Ctx()) is None      # WGSASSIGN_WINDOW_SITES alone routes nothing
    monkeypatch.setenv("WGSASSIGN_LOO_WINDOW_SITES", "20000")
    assert WGSassign._loo_window_sites(_args(*argv), OneRank(), None) == 16384
    assert WGSassign._loo_window_sites(_args(*argv, "--ne_obs"), OneRank(), None) is None
    assert WGSassign._loo_window_sites(_args(*argv[:-1]), OneRank(), None) is None
    assert WGSassign._loo_window_sites(_args("--beagle", "x.gz", "--pop_af_IDs", str(tmp_path / "no.txt"), "--get_reference_af", "--loo"), OneRank(), None) is None
    monkeypatch.setenv("WGSASSIGN_LOO_WINDOW_SITES", "100")
    with pytest.raises(SystemExit, match="WGSASSIGN_LOO_WINDOW_SITES"):
        WGSassign._loo_window_sites(_args(*argv), OneRank(), None)


def test_new_symbols_are_declared_bound_and_exported():
    from wgsassign_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wgsassign_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wgs_[a-z0-9_]+)\s*\(", text))
    build.build()
    lib = _lib.load()
    for name in ("wgs_loo_stream_create", "wgs_loo_stream_push", "wgs_loo_stream_finish", "wgs_loo_stream_destroy", "wgs_em_stream_push_keep"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name


def test_push_checks_under_the_sanitizers(tmp_path):
    """csrc/stream_checks.h is host-only: the `loo` part of tests/c_abi/stream_checks_check.cpp drives what wgs_loo_stream_push refuses
    (and the sums-above-a-horizon check of wgs_em_stream_push_keep) under AddressSanitizer + UBSan, as a program of its own."""
    import sanitized
    r = sanitized.run(tmp_path, "stream_checks_check.cpp", "loo")
    assert r.returncode == 0 and r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 100, (r.stdout[-2000:], r.stderr[-3000:])
