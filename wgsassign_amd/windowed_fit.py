"""The EM fit in site windows: which iteration each fit stops at, found in rounds over the file.
Host-only and free of the GPU: pure decision logic over the sums and carries a round brings back, so a CPU stand-in drives
it in the tests as tests/cpu_standin.py drives device.run_em.

The EM update is per site (emMAF_cy.pyx:10-23): site s of fit k follows f_0 = 0.25, f_1, f_2, ... whatever the other sites
do.  Only the stopping test couples the sites: the reference's result is f_t* with t* the first t <= maf_iter at which its
serial float32 rmse1d(f_t, f_t-1) < tole, or f_maf_iter (iteration count 0, nothing printed) when there is none.  So t* is
found from per-iteration sums gathered over ALL windows, and every window is then run for exactly t* iterations.

A ROUND is one pass over the file in windows.  Every window resets every fit to 0.25 and runs it for as long as the round's
plan says.  Round 1 runs maf_iter iterations and adds each window's float64 sum of squared differences of iteration t to
S[t][k]; the order of that addition does not matter, because the sum only decides outside the band of
device.guard_band / decide_converged (= em_band / em_classify of csrc/em_fit_ledger.h), where any float64 rounding is
far inside the band's margin, and inside the band the exact chain decides: the reference's own serial float32 sum, walked
over the windows in file order with a float32 carry C[t][k], as it is walked over SNP shards.  A chain needs another round,
because which iterations need one is known only once all windows have added to S.  A fit whose stopping iteration was known
when a round began is run to it, clamped and written out in that round.

Per fit k:  ruled_out[k]  iterations known not to stop the fit
            stop[k]       None, or the iteration its frequencies are taken from
            iters[k]      what the reference would report: stop[k], or 0 when maf_iter was exhausted
            chain[k]      iterations whose exact chain the next round walks
Two rounds when the sums decide every fit, three when a chain is needed and its first batch of candidates settles it.

Leave-one-out re-fits (glassy.loo_windowed) are n fits of the same kind, with two differences, both optional here:
  first_iters   a per-fit HORIZON: round 1 runs fit k for first_iters[k] iterations instead of maf_iter and gathers sums only for
                those; the decision walk stops at the horizon (summed[k]: the iterations of fit k whose sums S holds).  A fit
                neither stopped nor exhausted there gets a further sums round with a doubled horizon, capped at maf_iter, whose
                plan says through sums_from[k] = summed[k] that only the iterations above the old horizon are added: S is zeroed
                once, when the stream is made, and every (window, iteration, fit) sum enters it exactly once;
  hold_final    no fit is final before every stop is known: scoring individual i needs its own re-fit and other individuals'
                re-fits in the same window at the same time, so one last round runs every fit to its stop.
"""
import numpy as np

from .device import chain_diff, decide_converged

CHAIN_LOOKAHEAD = 8         # iterations of one fit a round walks the exact chain for, at most

ACTIVE, CONVERGED, UNDECIDED = 0, 1, 2      # = EM_ACTIVE, EM_CONVERGED, EM_UNDECIDED of csrc/em_fit_ledger.h


def classify(ssq, m_total, tole, guard=0.0):
    """em_classify(ssq, em_band(tole, m_total, guard)) through device.decide_converged, which tests hold to it edge for edge."""
    d = decide_converged(float(ssq), m_total, tole, guard)
    return CONVERGED if d > 0 else ACTIVE if d < 0 else UNDECIDED


class RoundPlan:
    """What one round does in every window: run_iters[k] iterations of fit k from 0.25; final[k]: that is its stopping
    iteration, clamp and write it; chains: (fit, iteration) pairs sorted by iteration; add_sums: the sums join S -- those of
    iteration t of fit k for t > sums_from[k] (zeros unless the round extends a horizon)."""

    def __init__(self, number, run_iters, final, chains, add_sums, sums_from=None):
        self.number = int(number)
        self.run_iters = np.ascontiguousarray(run_iters, dtype=np.int32)
        self.final = np.ascontiguousarray(final, dtype=np.int32)
        self.chains = sorted(((int(k), int(t)) for k, t in chains), key=lambda c: (c[1], c[0]))
        self.add_sums = bool(add_sums)
        self.sums_from = np.zeros(len(self.run_iters), dtype=np.int32) if sums_from is None else np.ascontiguousarray(sums_from, dtype=np.int32)

    @property
    def T(self):
        return int(self.run_iters.max()) if len(self.run_iters) else 0


class RoundScheme:
    def __init__(self, n_fits, maf_iter, tole, m_total, guard=0.0, lookahead=None, first_iters=None, hold_final=False):
        self.n_fits, self.maf_iter, self.tole, self.m_total, self.guard = int(n_fits), max(0, int(maf_iter)), float(tole), int(m_total), float(guard)
        self.lookahead = max(1, int(CHAIN_LOOKAHEAD if lookahead is None else lookahead))
        self.ruled_out = [0] * self.n_fits
        self.stop = [None] * self.n_fits
        self.iters = np.zeros(self.n_fits, dtype=np.int32)
        self.chain = [[] for _ in range(self.n_fits)]
        self.written = [False] * self.n_fits
        self.rounds = 0
        self.chain_iterations = 0           # (fit, iteration) chains walked over the file so far
        self.have_sums = False
        self.hold_final = bool(hold_final)
        if first_iters is None:
            self.horizon = [self.maf_iter] * self.n_fits
        else:
            if len(first_iters) != self.n_fits:
                raise ValueError("first_iters must have one entry per fit")
            self.horizon = [min(self.maf_iter, max(1, int(h))) for h in first_iters]
        self.iterations_round1 = int(sum(self.horizon))
        self.summed = [0] * self.n_fits         # iterations of every fit whose sums S holds
        self.extend = [False] * self.n_fits     # the walk reached the horizon: the next round runs the fit to its doubled horizon
        self.extension_rounds = 0
        if self.maf_iter == 0:              # emMAF.py:20 never enters its loop: f = 0.25, nothing to decide
            self.stop = [0] * self.n_fits
            self.have_sums = True

    def done(self):
        return all(self.written)

    def plan(self):
        """The next round."""
        if not self.have_sums:
            return RoundPlan(self.rounds + 1, list(self.horizon), [0] * self.n_fits, [], True)
        hold = self.hold_final and any(s is None for s in self.stop)
        run, final, chains, sums_from = [], [], [], []
        for k in range(self.n_fits):
            if self.written[k]:
                run.append(0), final.append(0)
            elif self.stop[k] is not None:
                run.append(0 if hold else self.stop[k]), final.append(0 if hold else 1)
            elif self.extend[k]:
                run.append(self.horizon[k]), final.append(0)
            else:
                run.append(max(self.chain[k])), final.append(0)
                chains.extend((k, t) for t in self.chain[k])
            sums_from.append(self.summed[k] if self.extend[k] else run[-1])
        add = any(self.extend)
        return RoundPlan(self.rounds + 1, run, final, chains, add, sums_from if add else None)

    def _class(self, S, t, k):
        return classify(S[t - 1][k], self.m_total, self.tole, self.guard)

    def after_round(self, plan, S, C):
        """The decisions a round allows.  S[t-1][k]: the float64 sum of iteration t over all sites; C[t-1][k]: the float32
        carry after the last window of the chains this round walked (other cells are not looked at)."""
        self.rounds += 1
        self.have_sums = True
        self.chain_iterations += len(plan.chains)
        if plan.add_sums:
            self.extension_rounds += 1 if plan.number > 1 else 0
            for k in range(self.n_fits):
                if plan.sums_from[k] < plan.run_iters[k]:
                    self.summed[k] = max(self.summed[k], int(plan.run_iters[k]))
        for k in range(self.n_fits):
            if plan.final[k]:
                self.written[k] = True
        chained = [set() for _ in range(self.n_fits)]
        for k, t in plan.chains:
            chained[k].add(t)
        for k in range(self.n_fits):
            if self.stop[k] is not None:
                continue
            self.chain[k] = []
            self.extend[k] = False
            t = self.ruled_out[k] + 1
            while True:
                if t > self.maf_iter:                   # exhausted: f_maf_iter, the reference prints nothing
                    self.stop[k], self.iters[k] = self.maf_iter, 0
                    break
                if t > self.summed[k]:                  # the horizon: nothing is known of iteration t yet -- a further sums round
                    self.horizon[k] = min(self.maf_iter, max(2 * self.horizon[k], t))
                    self.extend[k] = True
                    break
                c = self._class(S, t, k)
                if c == UNDECIDED and t in chained[k]:
                    c = CONVERGED if chain_diff(C[t - 1][k], self.m_total) < self.tole else ACTIVE
                if c == ACTIVE:
                    self.ruled_out[k] = t
                    t += 1
                elif c == CONVERGED:
                    self.stop[k], self.iters[k] = t, t
                    break
                else:                                   # the sum cannot say, and no chain of this iteration was walked: next round
                    self.chain[k] = self._candidates(S, t, k)
                    break

    def _candidates(self, S, t, k):
        """t and the following iterations that are not ruled out by their sums, lookahead of them at most, ending with the
        first one whose sum says converged (the fit stops there at the latest); none past the fit's horizon."""
        out = [t]
        u = t + 1
        while len(out) < self.lookahead and u <= self.summed[k] and self._class(S, out[-1], k) != CONVERGED:
            c = self._class(S, u, k)
            if c != ACTIVE:
                out.append(u)
            if c == CONVERGED:
                break
            u += 1
        return out


def fit(backend, n_fits, maf_iter, tole, m_total, guard=0.0, lookahead=None, first_iters=None, hold_final=False):
    """Rounds until every fit is written.  backend.run_round(plan) -> (S, C) runs the plan in every window of the file, in
    file order, and writes the final fits.  Returns (iters (n_fits,) int32, the scheme -- rounds, chain_iterations, stop).
    first_iters, hold_final: the horizons and the one last round of the leave-one-out re-fits (see above)."""
    scheme = RoundScheme(n_fits, maf_iter, tole, m_total, guard, lookahead, first_iters, hold_final)
    # (a horizon doubles: at most log2(maf_iter) + 1 extension rounds between the chain rounds)
    limit = scheme.maf_iter + 2 + (0 if first_iters is None else 2 * (scheme.maf_iter.bit_length() + 1))
    while not scheme.done():
        plan = scheme.plan()
        S, C = backend.run_round(plan)
        scheme.after_round(plan, S, C)
        if scheme.rounds > limit:
            raise RuntimeError("the windowed fit did not settle in %d rounds" % scheme.rounds)
    return scheme.iters.copy(), scheme


class ChainPlan:
    """What one round of masked fits does in every window: run_iters[k] iterations of fit k from 0.25; final: every fit is run to its
    stopping iteration and clamped; chains: (fit, iteration) pairs sorted by iteration."""

    def __init__(self, number, run_iters, final, chains):
        self.number = int(number)
        self.run_iters = np.ascontiguousarray(run_iters, dtype=np.int32)
        self.final = bool(final)
        self.chains = sorted(((int(k), int(t)) for k, t in chains), key=lambda c: (c[1], c[0]))


class ChainScheme:
    """The rounds of fits whose stopping test runs over a site subset of the fit's own (zscore.reference_z_scores_windowed): fit k
    stops at the first t <= maf_iter with chain_diff(carry of iteration t over ITS kept sites of all windows, kept_total[k]) < tole
    -- em_chain_converged, what wgs_em_fit_masked decides with every iteration -- or is exhausted (frequencies of maf_iter,
    iteration count 0).  No sum decides anything here, so there is no band and no chain round: a FIT ROUND walks the exact chain of
    EVERY iteration above walked[k] up to the fit's horizon, for every fit not yet decided, and one read of the carries decides all
    of them.  A pass over the files costs about ten times what the fits of a window cost, so walking chains
    that turn out not to be needed is the cheap side: the design that never needs a second pass merely to decide is the right one.
    A fit neither stopped nor exhausted at its horizon gets another round with the horizon doubled, capped at maf_iter; that round
    runs the fit from 0.25 again but walks only the iterations above the old horizon -- the carries of the earlier ones are final
    (they said "not converged"), so every (window, iteration, fit) chain is walked exactly once.  When every fit is decided, one
    FINAL round runs each to its stop.

        horizon[k]  iterations the next fit round runs fit k for        walked[k]  iterations whose carries were read and decided
        stop[k]     None, or the iteration the frequencies are taken from        iters[k]   stop[k], or 0 when exhausted"""

    def __init__(self, n_fits, maf_iter, tole, first_horizon):
        self.n_fits, self.maf_iter, self.tole = int(n_fits), max(0, int(maf_iter)), float(tole)
        h = min(self.maf_iter, max(1, int(first_horizon)))
        self.horizon = [h] * self.n_fits
        self.walked = [0] * self.n_fits
        self.stop = [None] * self.n_fits
        self.iters = np.zeros(self.n_fits, dtype=np.int32)
        self.fit_rounds = 0
        self.horizons = []                  # the largest horizon of every fit round
        self.chain_iterations = 0
        self.finished = False
        if self.maf_iter == 0:              # emMAF.py:20 never enters its loop: f = 0.25, nothing to decide
            self.stop = [0] * self.n_fits

    def decided(self):
        return all(s is not None for s in self.stop)

    def plan(self):
        """The next round: a fit round while a fit is undecided (the decided ones rest), else the final round."""
        if self.decided():
            return ChainPlan(self.fit_rounds + 1, list(self.stop), True, [])
        run = [0 if self.stop[k] is not None else self.horizon[k] for k in range(self.n_fits)]
        chains = [(k, t) for k in range(self.n_fits) if self.stop[k] is None for t in range(self.walked[k] + 1, self.horizon[k] + 1)]
        return ChainPlan(self.fit_rounds + 1, run, False, chains)

    def after_round(self, plan, C, kept_total):
        """C[t-1][k]: the float32 carry of iteration t after the last window, for the chains this round walked (other cells are not
        looked at); kept_total[k]: the sites fit k's individual kept over ALL windows (> 0)."""
        if plan.final:
            self.finished = True
            return
        self.fit_rounds += 1
        self.horizons.append(int(plan.run_iters.max()))
        self.chain_iterations += len(plan.chains)
        for k in range(self.n_fits):
            if self.stop[k] is not None:
                continue
            for t in range(self.walked[k] + 1, self.horizon[k] + 1):
                if chain_diff(C[t - 1][k], kept_total[k]) < self.tole:
                    self.stop[k], self.iters[k] = t, t
                    break
            else:
                self.walked[k] = self.horizon[k]
                if self.horizon[k] >= self.maf_iter:            # exhausted: f_maf_iter, the reference prints nothing
                    self.stop[k], self.iters[k] = self.maf_iter, 0
                else:
                    self.horizon[k] = min(self.maf_iter, 2 * self.horizon[k])


def fit_masked(backend, n_fits, maf_iter, tole, first_horizon):
    """Rounds until every fit has run its final round.  backend.run_round(plan) -> (C, kept_total) runs the plan in every window of the
    files, in file order (C may be None for the final round).  Returns (iters (n_fits,) int32, the scheme)."""
    scheme = ChainScheme(n_fits, maf_iter, tole, first_horizon)
    while not scheme.finished:
        plan = scheme.plan()
        C, kept_total = backend.run_round(plan)
        scheme.after_round(plan, C, kept_total)
        if scheme.fit_rounds > scheme.maf_iter.bit_length() + 2:
            raise RuntimeError("the masked fits did not settle in %d rounds" % scheme.fit_rounds)
    return scheme.iters.copy(), scheme
