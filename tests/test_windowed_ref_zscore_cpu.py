"""--get_reference_z_score in site windows, the parts that need no GPU: the rounds of the masked fits (windowed_fit.ChainScheme) driven
by a NumPy stand-in -- a per-site float32 EM update and, as the masked chain, the serial float32 sum over an individual's kept sites
carried from window to window -- against the decision taken over one matrix; the byte count per site and the plan it gives; the
command line's routing and messages; the order of the printed lines; the new C-ABI symbol and the refusal checks under the
sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

F32 = np.float32


# ---------------------------------------------------------------- the stand-in
def em_update(L, f):
    """One EM update of emMAF_cy.pyx's kind, per site and in float32 throughout: every operation is elementwise over the sites, so a
    site's value does not depend on which rows it is computed with."""
    n = L.shape[1] // 2
    acc = np.zeros_like(f)
    one, two = F32(1), F32(2)
    for i in range(n):
        g0, g1 = L[:, 2 * i], L[:, 2 * i + 1]
        p0 = ((one - f) * (one - f)) * g0
        p1 = ((two * f) * (one - f)) * g1
        p2 = (f * f) * ((one - g0) - g1)
        acc = acc + (p1 + two * p2) / ((p0 + p1) + p2)
    return acc / F32(2 * n)


def serial_chain(carry, a, b):
    """emMAF_cy.pyx:30-31 continued from `carry`: one float32 addition per site, site order."""
    d = a - b
    acc = np.cumsum(np.concatenate(([F32(carry)], d * d)).astype(F32), dtype=F32)
    return F32(acc[-1])


class Problem:
    """n_fits fits over m sites, each with its own columns of L and its own kept sites; windows cut the sites at `cuts`."""

    def __init__(self, seed, m, cuts, n_fits=5, empty=((1, 0), (2, 1), (3, 2))):
        rng = np.random.default_rng(seed)
        self.m, self.n_fits = m, n_fits
        self.edges = [0] + list(cuts) + [m]
        self.L = []
        for k in range(n_fits):
            n = 1 + k % 3
            freq = rng.random(m) * 0.8 + 0.1
            geno = rng.binomial(2, freq[:, None], size=(m, n))
            depth = 0.3 + 0.5 * k
            L = np.empty((m, 2 * n), dtype=F32)
            for i in range(n):
                reads = rng.poisson(depth, size=m)
                alt = rng.binomial(reads, np.where(geno[:, i] == 0, 0.01, np.where(geno[:, i] == 1, 0.5, 0.99)))
                like = np.stack([0.99 ** (reads - alt) * 0.01 ** alt, 0.5 ** reads, 0.01 ** (reads - alt) * 0.99 ** alt], axis=1)
                like /= like.sum(axis=1, keepdims=True)
                L[:, 2 * i], L[:, 2 * i + 1] = like[:, 0], like[:, 1]
            self.L.append(L)
        self.keep = [rng.random(m) < (0.15 + 0.17 * k) for k in range(n_fits)]
        for k, w in empty:                                  # fit k keeps nothing in window w
            if k < n_fits and w + 1 < len(self.edges) and len(self.edges) > 2:
                self.keep[k][self.edges[w]:self.edges[w + 1]] = False
        self.kept_total = np.array([int(x.sum()) for x in self.keep], dtype=np.int64)

    def windows(self):
        return list(zip(self.edges[:-1], self.edges[1:]))

    def one_matrix(self, maf_iter, tole):
        """What wgs_em_fit_masked decides on the whole matrix: (iters, stop, frequencies at the stop)."""
        from wgsassign_amd.device import chain_diff
        iters, stop, freq = [], [], []
        for k in range(self.n_fits):
            f = np.full(self.m, 0.25, dtype=F32)
            it = 0
            for t in range(1, maf_iter + 1):
                prev, f = f, em_update(self.L[k], f)
                if chain_diff(serial_chain(0, f[self.keep[k]], prev[self.keep[k]]), self.kept_total[k]) < tole:
                    it = t
                    break
            iters.append(it), stop.append(it or maf_iter), freq.append(f)
        return iters, stop, freq


class StandIn:
    """fit_masked's backend: every round is a pass over the windows in order; the carries start at zero when a round begins, as the
    device's table does; a fit that keeps nothing in a window leaves its carry alone.  walked counts every (window, iteration, fit)."""

    def __init__(self, problem, maf_iter):
        self.p, self.maf_iter = problem, maf_iter
        self.walked = {}
        self.plans = []
        self.final = None

    def run_round(self, plan):
        p = self.p
        self.plans.append(plan)
        C = np.zeros((self.maf_iter, p.n_fits), dtype=F32)
        chains = set(plan.chains)
        assert len(chains) == len(plan.chains) and plan.chains == sorted(plan.chains, key=lambda c: (c[1], c[0]))
        final = [np.empty(p.m, dtype=F32) for _ in range(p.n_fits)]
        for w, (lo, hi) in enumerate(p.windows()):
            for k in range(p.n_fits):
                f = np.full(hi - lo, 0.25, dtype=F32)
                keep = p.keep[k][lo:hi]
                for t in range(1, int(plan.run_iters[k]) + 1):
                    prev, f = f, em_update(p.L[k][lo:hi], f)
                    if (k, t) in chains:
                        self.walked[w, t, k] = self.walked.get((w, t, k), 0) + 1
                        if keep.any():
                            C[t - 1, k] = serial_chain(C[t - 1, k], f[keep], prev[keep])
                final[k][lo:hi] = f
        if plan.final:
            self.final = final
        return C, p.kept_total


def settle(problem, maf_iter, tole, horizon):
    from wgsassign_amd import windowed_fit
    backend = StandIn(problem, maf_iter)
    iters, scheme = windowed_fit.fit_masked(backend, problem.n_fits, maf_iter, tole, horizon)
    return iters, scheme, backend


CASES = [(3, 300, (100, 200)), (4, 257, (64,)), (5, 200, (8, 9, 150)), (6, 120, ())]


@pytest.mark.parametrize("seed, m, cuts", CASES)
@pytest.mark.parametrize("horizon", [1, 2, 200])
def test_decisions_are_those_of_one_matrix(seed, m, cuts, horizon):
    """Windows of unequal kept counts, zero among them, against the decision over the whole matrix: the iteration of every fit, its
    frequencies, and every (window, iteration, fit) chain walked exactly once over all extension rounds."""
    maf_iter, tole = 200, 2e-3
    p = Problem(seed, m, cuts)
    per_window = np.array([[int(p.keep[k][lo:hi].sum()) for lo, hi in p.windows()] for k in range(p.n_fits)])
    if len(cuts) >= 2:
        assert (per_window == 0).any() and len(set(per_window.ravel())) > 3 and (p.kept_total > 0).all()
    want_iters, want_stop, want_f = p.one_matrix(maf_iter, tole)
    assert len(set(want_iters)) > 1 and all(want_iters)
    iters, scheme, backend = settle(p, maf_iter, tole, horizon)
    assert list(iters) == want_iters and list(scheme.stop) == want_stop
    for k in range(p.n_fits):
        assert backend.final[k].tobytes() == want_f[k].tobytes()
    # every chain once: iterations 1 .. the horizon at which the fit was decided, in every window
    assert set(backend.walked.values()) == {1}
    for k in range(p.n_fits):
        ts = sorted({t for (w, t, kk) in backend.walked if kk == k})
        assert ts == list(range(1, len(ts) + 1)) and ts[-1] >= want_stop[k]
        assert all((w, t, k) in backend.walked for w in range(len(p.windows())) for t in ts)
        if horizon == 1:
            assert ts[-1] < 2 * want_stop[k]                              # the horizon doubles: never twice what was needed
    if horizon == 200:
        assert scheme.fit_rounds == 1 and scheme.horizons == [200]
    else:
        assert scheme.fit_rounds >= 2 and scheme.horizons[0] == horizon and scheme.horizons == sorted(scheme.horizons)
    assert backend.plans[-1].final and not any(pl.final for pl in backend.plans[:-1]) and len(backend.plans) == scheme.fit_rounds + 1
    assert list(backend.plans[-1].run_iters) == want_stop and backend.plans[-1].chains == []
    assert scheme.chain_iterations * len(p.windows()) == len(backend.walked)


@pytest.mark.parametrize("horizon", [1, 2, 3, 7, 50])
def test_exhausted_fits(horizon):
    """maf_iter between the stops: the fits beyond it are exhausted -- frequencies of maf_iter, iteration count 0 -- the others stop."""
    p = Problem(3, 300, (100, 200))
    full, _, _ = p.one_matrix(200, 2e-3)
    maf_iter = sorted(full)[len(full) // 2]                              # (at least one fit stops exactly there, the larger ones do not)
    want_iters, want_stop, want_f = p.one_matrix(maf_iter, 2e-3)
    assert 0 in want_iters and any(want_iters) and maf_iter in want_iters
    iters, scheme, backend = settle(p, maf_iter, 2e-3, horizon)
    assert list(iters) == want_iters and list(scheme.stop) == want_stop
    assert all(backend.final[k].tobytes() == want_f[k].tobytes() for k in range(p.n_fits))
    assert set(backend.walked.values()) == {1} and max(t for (_, t, _) in backend.walked) == maf_iter
    assert max(scheme.horizons) == maf_iter or horizon >= maf_iter


def test_no_iterations_at_all():
    """maf_iter 0: emMAF.py never enters its loop -- f = 0.25, nothing walked, the final round alone."""
    p = Problem(6, 120, ())
    iters, scheme, backend = settle(p, 0, 1e-4, 32)
    assert list(iters) == [0] * p.n_fits and scheme.fit_rounds == 0 and not backend.walked and len(backend.plans) == 1
    assert all((f == F32(0.25)).all() for f in backend.final)


def test_decided_fits_rest_in_later_rounds():
    p = Problem(3, 300, (100, 200))
    iters, scheme, backend = settle(p, 200, 2e-3, 2)
    for before, after in zip(backend.plans[:-2], backend.plans[1:-1]):
        for k in range(p.n_fits):
            assert after.run_iters[k] in (0, 2 * before.run_iters[k]) or after.run_iters[k] == 200
            if after.run_iters[k]:
                assert [t for kk, t in after.chains if kk == k] == list(range(before.run_iters[k] + 1, after.run_iters[k] + 1))
            else:
                assert iters[k] and iters[k] <= before.run_iters[k] or before.run_iters[k] == 0


def test_first_horizon_default_keyword_and_variable():
    from wgsassign_amd import zscore
    assert zscore.ZREF_FIRST_HORIZON == 32 and zscore.zref_first_horizon(None, {}) == 32
    assert zscore.zref_first_horizon(None, {"WGSASSIGN_ZREF_HORIZON": "7"}) == 7 and zscore.zref_first_horizon(5, {"WGSASSIGN_ZREF_HORIZON": "7"}) == 5
    assert zscore.zref_first_horizon(None, {"WGSASSIGN_ZREF_HORIZON": " "}) == 32
    with pytest.raises(ValueError, match="WGSASSIGN_ZREF_HORIZON must be a number of iterations"):
        zscore.zref_first_horizon(None, {"WGSASSIGN_ZREF_HORIZON": "many"})
    with pytest.raises(ValueError, match="at least 1 iteration"):
        zscore.zref_first_horizon(0, {})


# ---------------------------------------------------------------- the plan
def test_zref_site_bytes_against_hand_sums():
    from wgsassign_amd import windows
    # 200 individuals in 5 populations of 40, all in the batch: slabs 16 x 100 pairs, depths 400, mask words 12 x 200 / 64 rounded up,
    # statistics 2400, two frequency buffers 1600, per-tile sums 8 x 200 / 64, compacted pairs 1600
    assert windows.zref_site_bytes(200, 5, 200, [40] * 5) == 1600 + 400 + 38 + 2400 + 1600 + 25 + 1600
    # odd populations take a pair more each; unknown populations the worst split
    assert windows.zref_site_bytes(8, 3, 8, [3, 3, 2]) == 16 * 5 + 16 + 2 + 96 + 64 + 1 + 64
    assert windows.zref_site_bytes(8, 3, 8) == windows.zref_site_bytes(8, 3, 8, [3, 3, 2]) == 16 * ((8 + 3) // 2) + 243
    assert windows.zref_site_bytes(8, 3, 1, [3, 3, 2]) == 80 + 16 + 1 + 12 + 8 + 1 + 8
    # against z_site_bytes: the frequency file's columns go, the slabs replace the one slab, the fits and their compacted pairs come
    n, K, count, counts = 200, 5, 64, [39, 41, 40, 37, 43]
    pairs = sum((c + 1) // 2 for c in counts)
    assert windows.zref_site_bytes(n, K, count, counts) == (windows.z_site_bytes(n, K, count) - 4 * K - 16 * 100 + 16 * pairs
                                                            + 8 * count + (8 * count + 63) // 64 + 8 * count)
    assert windows.zref_state_bytes(10, 200) == windows.z_state_bytes(10) + 12 * 200 * 10
    assert windows.ENV_ZREF == "WGSASSIGN_ZREF_WINDOW_SITES" and windows.ENV_ZREF not in (windows.ENV, windows.ENV_LOO, windows.ENV_NE, windows.ENV_Z)


def test_plan_zref():
    from wgsassign_amd import windows
    free = 100 << 30
    budget = windows.budget(free)
    n, K, count, counts = 200, 5, 200, [40] * 5
    resident = windows.zref_site_bytes(n, K, 64, counts)
    m_fits = budget // resident
    assert windows.plan_zref(m_fits, n, K, count, free, environ={}, counts=counts) is None
    assert windows.fits_resident_zref(m_fits, n, K, count, free, counts) and not windows.fits_resident_zref(m_fits + 1, n, K, count, free, counts)
    W, batch = windows.plan_zref(m_fits + 1, n, K, count, free, environ={}, counts=counts)
    per_site = windows.zref_site_bytes(n, K, count, counts) + 16 * 100 + 8 * count + (8 * count + 63) // 64      # the second matrix and its fits
    state = windows.zref_state_bytes(count, 200)
    assert batch == count and W % 8192 == 0 and W == (budget - state) // per_site // 8192 * 8192
    assert state + W * per_site <= budget < state + (W + 8192) * per_site
    # its own variable forces windows whatever fits; no other variable does
    assert windows.plan_zref(1000, n, K, count, free, environ={"WGSASSIGN_ZREF_WINDOW_SITES": "20000"}, counts=counts) == (16384, count)
    for other in ("WGSASSIGN_WINDOW_SITES", "WGSASSIGN_LOO_WINDOW_SITES", "WGSASSIGN_NE_WINDOW_SITES", "WGSASSIGN_Z_WINDOW_SITES"):
        assert windows.plan_zref(1000, n, K, count, free, environ={other: "20000"}, counts=counts) is None
    with pytest.raises(ValueError, match="WGSASSIGN_ZREF_WINDOW_SITES=100 is below 8192"):
        windows.plan_zref(1000, n, K, count, free, environ={"WGSASSIGN_ZREF_WINDOW_SITES": "100"})
    # rounds of individuals: the batch is halved until a window of 8192 sites fits beside the state
    small = 1 << 30
    W, batch = windows.plan_zref(10 ** 7, 2000, 5, 2000, small, environ={})
    assert batch in (500, 1000) and W >= 8192 and 2000 // batch * batch == 2000

    def need(b, sites):
        return windows.zref_state_bytes(b, 200) + sites * (windows.zref_site_bytes(2000, 5, b) + 16 * ((2000 + 5) // 2) + 8 * b + (8 * b + 63) // 64)
    assert need(batch, W) <= windows.budget(small) < need(2 * batch, 8192)
    assert windows.zref_batch(8192, 2000, 5, 2000, small) == batch and windows.zref_batch(8192, 8, 3, 8, free, counts=[3, 3, 2]) == 8
    with pytest.raises(MemoryError, match="windowed reference z-scores need two windows of 8192 sites"):
        windows.plan_zref(10 ** 7, 200000, 5, 10, 1 << 30, environ={})


# ---------------------------------------------------------------- the command line
def _args(*argv):
    from wgsassign_amd import WGSassign
    return WGSassign.parser.parse_args(list(argv))


BASE = ("--beagle", "x.beagle.gz", "--pop_af_IDs", "ids.txt", "--pop_names", "p.txt", "--ind_ad_file", "ad.txt", "--get_reference_z_score")
OTHERS = (("--get_reference_af",), ("--get_reference_af", "--loo"), ("--get_reference_af", "--ne_obs"), ("--get_pop_like",),
          ("--get_assignment_z_score",), ("--get_reference_af", "--loo", "--loo_downsampled_beagle", "d.gz"))
# every argv the older routing tests hold the older candidates to (tests/test_windowed_zscore_cpu.py and its siblings)
Z_BASE = ("--beagle", "x.beagle.gz", "--pop_af_file", "a.npy", "--pop_af_IDs", "ids.txt", "--pop_names", "p.txt", "--ind_ad_file", "ad.txt",
          "--get_assignment_z_score")
OLDER_ARGV = [Z_BASE, Z_BASE[:-1] + ("--get_reference_z_score",), Z_BASE + ("--get_reference_z_score",), Z_BASE + ("--get_pop_like",),
              ("--beagle", "x.beagle.gz", "--get_pop_like", "--pop_af_file", "a.npy"), ("--beagle", "x.gz", "--pop_af_IDs", "i.txt", "--get_reference_af"),
              ("--beagle", "x.gz", "--pop_af_IDs", "i.txt", "--get_reference_af", "--loo"),
              ("--beagle", "x.gz", "--pop_af_IDs", "i.txt", "--get_reference_af", "--ne_obs"),
              ("--beagle", "x.gz", "--pop_af_IDs", "i.txt", "--get_reference_af", "--ne_obs", "--loo")]


def test_the_new_candidate_is_the_option_alone_on_one_rank():
    from wgsassign_amd.WGSassign import windowed_zref_candidate
    assert windowed_zref_candidate(_args(*BASE), 1)
    assert windowed_zref_candidate(_args(*BASE, "--single_read_threshold", "--ind_start", "2", "--ind_end", "5", "--maf_iter", "50", "--maf_tole",
                                         "1e-5", "--allele_count_threshold", "3", "--threads", "8"), 1)
    assert windowed_zref_candidate(_args(*BASE[:-3], "--ind_counts_file", "c.gz", "--ind_majmin_file", "m.txt", BASE[-1]), 1)
    assert not windowed_zref_candidate(_args(*BASE), 2) and not windowed_zref_candidate(_args(*BASE), 8)
    assert not windowed_zref_candidate(_args(*BASE[:-1]), 1)
    for other in OTHERS:
        assert not windowed_zref_candidate(_args(*BASE, *other), 1), other


def test_the_older_candidates_answer_as_before():
    """What the five older candidates answered for every argv of the existing routing tests, written out: the new route is additive."""
    from wgsassign_amd import WGSassign
    names = ("windowed_candidate", "windowed_fit_candidate", "windowed_loo_candidate", "windowed_ne_candidate", "windowed_z_candidate")
    want = [(0, 0, 0, 0, 1), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0),
            (0, 0, 0, 1, 0)]
    for argv, row in zip(OLDER_ARGV, want):
        assert tuple(int(getattr(WGSassign, nm)(_args(*argv), 1)) for nm in names) == row, argv
        assert not any(getattr(WGSassign, nm)(_args(*argv), 2) for nm in names)
    for candidate in names:
        assert not getattr(WGSassign, candidate)(_args(*BASE), 1), candidate
    assert [int(WGSassign.windowed_zref_candidate(_args(*argv), 1)) for argv in OLDER_ARGV] == [0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert WGSassign.WINDOWS_ONLY == "windowed scoring (WGSASSIGN_WINDOW_SITES) covers --get_pop_like on one rank only"


class OneRank:
    world = 1


class TwoRanks:
    world = 2


class Ctx:
    def mem_info(self):
        return 100 << 30, 100 << 30


def test_only_its_own_variable_routes_the_run(monkeypatch, tmp_path):
    from wgsassign_amd import WGSassign
    ids = tmp_path / "ids.txt"
    ids.write_text("".join("s%d\tp%d\n" % (i, i % 2) for i in range(6)))
    argv = ("--beagle", "x.gz", "--pop_af_IDs", str(ids), "--get_reference_z_score")
    monkeypatch.delenv("WGSASSIGN_ZREF_WINDOW_SITES", raising=False)
    for name in ("WGSASSIGN_WINDOW_SITES", "WGSASSIGN_LOO_WINDOW_SITES", "WGSASSIGN_NE_WINDOW_SITES", "WGSASSIGN_Z_WINDOW_SITES"):
        monkeypatch.setenv(name, "20000")
    monkeypatch.setattr(WGSassign.os.path, "getsize", lambda p: 1)                  # (the first look: a file that surely fits)
    assert WGSassign._zref_window_sites(_args(*argv), OneRank(), Ctx()) is None      # none of the older variables routes this option
    for older in (WGSassign._window_sites, WGSassign._fit_window_sites, WGSassign._loo_window_sites, WGSassign._ne_window_sites,
                  WGSassign._z_window_sites):
        assert older(_args(*argv), OneRank(), None) is None                          # ... and it is none of their candidates
    monkeypatch.setenv("WGSASSIGN_ZREF_WINDOW_SITES", "20000")
    assert WGSassign._zref_window_sites(_args(*argv), OneRank(), None) == (16384, None)
    assert WGSassign._zref_window_sites(_args(*argv), TwoRanks(), None) is None
    assert WGSassign._zref_window_sites(_args(*argv, "--get_assignment_z_score"), OneRank(), None) is None
    assert WGSassign._zref_window_sites(_args(*argv, "--get_reference_af"), OneRank(), None) is None
    assert WGSassign._zref_window_sites(_args("--beagle", "x.gz", "--pop_af_IDs", str(tmp_path / "no.txt"), argv[-1]), OneRank(), None) is None
    for value, text in (("eight", "WGSASSIGN_ZREF_WINDOW_SITES must be a number of sites"), ("100", "WGSASSIGN_ZREF_WINDOW_SITES=100 is below 8192")):
        monkeypatch.setenv("WGSASSIGN_ZREF_WINDOW_SITES", value)
        with pytest.raises(SystemExit, match=text):
            WGSassign._zref_window_sites(_args(*argv), OneRank(), None)
    # its variable routes nothing else
    monkeypatch.setenv("WGSASSIGN_ZREF_WINDOW_SITES", "20000")
    for name in ("WGSASSIGN_WINDOW_SITES", "WGSASSIGN_LOO_WINDOW_SITES", "WGSASSIGN_NE_WINDOW_SITES", "WGSASSIGN_Z_WINDOW_SITES"):
        monkeypatch.delenv(name)
    af = tmp_path / "a.npy"
    np.save(af, np.zeros((4, 2), dtype=np.float32))
    assert WGSassign._z_window_sites(_args("--beagle", "x.gz", "--pop_af_file", str(af), "--get_assignment_z_score"), OneRank(), Ctx()) is None
    assert WGSassign._fit_window_sites(_args("--beagle", "x.gz", "--pop_af_IDs", str(ids), "--get_reference_af"), OneRank(), Ctx()) is None


def test_both_answers_of_the_hint():
    from wgsassign_amd import WGSassign
    e = RuntimeError("wgsassign_amd HIP call failed: hipMalloc of 123 bytes for population slab 0 failed")
    args = _args(*BASE)
    old = WGSassign.with_windows_hint(e, WGSassign.windowed_candidate(args, 1), WGSassign.windowed_z_candidate(args, 1))
    assert str(old) == str(e) + ": " + WGSassign.WINDOWS_ONLY                        # without the keyword: today's message
    new = WGSassign.with_windows_hint(e, WGSassign.windowed_candidate(args, 1), WGSassign.windowed_z_candidate(args, 1),
                                      zref_candidate=WGSassign.windowed_zref_candidate(args, 1))
    assert str(new) == str(e) + ": " + WGSassign.SET_WINDOW_SITES_ZREF and "WGSASSIGN_ZREF_WINDOW_SITES" in str(new)
    two = WGSassign.with_windows_hint(e, False, False, zref_candidate=WGSassign.windowed_zref_candidate(args, 2))
    assert str(two) == str(e) + ": " + WGSassign.WINDOWS_ONLY                        # several ranks keep it too
    assert str(WGSassign.with_windows_hint(e, False, True, zref_candidate=False)) == str(e) + ": " + WGSassign.SET_WINDOW_SITES_Z
    other = RuntimeError("something else")
    assert WGSassign.with_windows_hint(other, zref_candidate=True) is other


# ---------------------------------------------------------------- the printed lines
def test_lines_come_in_the_resident_runs_blocks():
    """130 individuals from ind_start 3: the resident run prints per batch of 64 first the converged lines of the batch's fits, then
    each individual's six lines.  The list is built the resident way and compared with what resident_order gives for results that
    arrived in rounds of 50."""
    from wgsassign_amd import zscore
    lo, hi = 3, 133
    rng = np.random.default_rng(2)
    iters = rng.integers(0, 40, size=hi - lo)
    iters[rng.random(hi - lo) < 0.2] = 0
    assert (iters[:64] == 0).any() and (iters[64:128] == 0).any() and iters[128:].any()

    def six_of(i):
        out = []
        zscore._finish_sums(i, 100 + i, F32(-3.5 * i), F32(-3.0 * i), F32(2.0 + i), out.append)
        return out
    want = []
    for i0, count in zscore._batches(lo, hi, 64):                        # reference_z_scores' own loop
        for j in range(count):
            if iters[i0 + j - lo]:
                want.append("EM (MAF) converged at iteration: " + str(int(iters[i0 + j - lo])))
        for j in range(count):
            zscore._finish_sums(i0 + j, 100 + i0 + j, F32(-3.5 * (i0 + j)), F32(-3.0 * (i0 + j)), F32(2.0 + i0 + j), want.append)
    converged, six = [None] * (hi - lo), [None] * (hi - lo)
    for r0, rc in zscore._batches(lo, hi, 50):                           # the windowed function's rounds
        for i in range(r0, r0 + rc):
            six[i - lo] = six_of(i)
            if iters[i - lo]:
                converged[i - lo] = "EM (MAF) converged at iteration: " + str(int(iters[i - lo]))
    got = zscore.resident_order(lo, hi, converged, six)
    assert got == want and len(got) == 6 * 130 + int((iters > 0).sum())
    assert got[0].startswith("EM (MAF)") and want.index("Finished individual 3") == int((iters[:64] > 0).sum())


# ---------------------------------------------------------------- the C ABI
def test_the_new_symbol_is_declared_bound_and_exported():
    from wgsassign_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "wgsassign_hip.h")).read()
    assert re.search(r"#define WGS_ABI_VERSION 4\b", text)
    assert re.search(r"\bint wgs_em_stream_push_masked\s*\(", text) and "wgs_em_stream_push_masked" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wgs_em_stream_push_masked"][1]) == 11
    build.build()
    lib = _lib.load()
    assert lib.wgs_version() == 4 and hasattr(lib, "wgs_em_stream_push_masked")


def test_masked_push_checks_under_the_sanitizers(tmp_path):
    """csrc/stream_checks.h is host-only: the `masked` part of tests/c_abi/stream_checks_check.cpp drives what
    wgs_em_stream_push_masked refuses, under AddressSanitizer + UBSan, as a program of its own."""
    import sanitized
    r = sanitized.run(tmp_path, "stream_checks_check.cpp", "masked")
    assert r.returncode == 0 and r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 100, (r.stdout[-2000:], r.stderr[-3000:])
