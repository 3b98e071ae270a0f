"""EM allele-frequency driver: drop-in for the reference's `emMAF.py`."""
import numpy as np

from .device import DeviceBeagle, EMBatch


def emMAF(L, iter, tole, t=1):
    """emMAF.py:15-27: start at f = 0.25, update until rmse(f, f_prev) < tole or `iter` updates.

    L is the (m, 2*n_pop) float32 matrix of one population.  It is uploaded once, the whole loop
    runs on the device, and only the convergence sums cross to the host each iteration.
    Returns the UNclamped float32 frequencies; prints the reference's convergence line.
    """
    L = np.asarray(L)
    m = L.shape[0]
    if m == 0:
        return np.empty(0, dtype=np.float32)
    if L.shape[1] // 2 == 0:
        # emMAF_cy.pyx:17,23 with no individuals: tmp/(float)0 = NaN for every SNP, never converges
        return np.full(m, np.nan, dtype=np.float32)
    beagle = DeviceBeagle.from_host(L)
    em = EMBatch(beagle, [0])
    iters = em.run(iter, tole)
    if iters[0] > 0:
        print("EM (MAF) converged at iteration: " + str(int(iters[0])))
    f = em.get_f(0)
    em.close()
    beagle.close()
    return f


def emMAF_populations(L, IDs, iter, tole, beagle=None, comm=None):
    """The per-population loop of WGSassign.py:211-242 as ONE batch of EM chains.

    The reference gathers each population's columns on the host and runs emMAF on the copy;
    here L is permuted once into population slabs on the device and all K fits advance together,
    each freezing at its own convergence iteration.  Returns (pops sorted, af (m, K) float32
    clamped per WGSassign.py:236-240, iters (K,)).  Prints one convergence line per population,
    in population order, like the reference does.
    """
    L = np.asarray(L) if L is not None else None
    IDs = np.asarray(IDs)
    pops = np.unique(IDs[:, 1])
    group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
    counts = np.bincount(group_of, minlength=len(pops))
    own = beagle is None
    if own:
        beagle = DeviceBeagle.from_host(L, group_of, len(pops))
    em = EMBatch(beagle, np.arange(len(pops), dtype=np.int32))
    iters = em.run(iter, tole, comm=comm)
    try:        # (sweeps enqueued, exact-chain resolutions, wall seconds, sweep-kernel ms) of the one-call fit, for whoever asks
        emMAF_populations.last_stats = em.fit_stats()
    except Exception:
        emMAF_populations.last_stats = None
    af = np.empty((beagle.m, len(pops)), dtype=np.float32)
    for k in range(len(pops)):
        if iters[k] > 0:
            print("EM (MAF) converged at iteration: " + str(int(iters[k])))
        em.clamp(k, int(counts[k]))
        af[:, k] = em.get_f(k)
    em.close()
    if own:
        beagle.close()
    return pops, af, iters


class _DeviceRounds:
    """windowed_fit's backend on the device: a round is one pass of reader_cy.stream_windows, every window pushed through the
    EMBatch of its matrix into one device.EMStream."""

    def __init__(self, windows, stream, counts, af, stats):
        self.windows, self.stream, self.af, self.stats = windows, stream, af, stats
        lo = 1 / (2 * (np.asarray(counts, dtype=np.float64) + 1))          # WGSassign.py:236-240, as EMBatch.clamp forms them
        self.lo, self.hi = lo.astype(np.float32), (1 - lo).astype(np.float32)
        self.batches = {}
        self.stage = None
        self.want_more = False

    def again(self):
        return self.want_more

    def run_round(self, plan):
        import time
        t0 = time.perf_counter()
        K = self.stream.n_fits
        final = np.flatnonzero(plan.final)
        pushed = 0
        for b in self.windows:
            em = self.batches.get(id(b))
            if em is None:          # one EMBatch per window matrix, made once and kept for every window and round
                em = self.batches[id(b)] = EMBatch(b, np.arange(K, dtype=np.int32))
                b.window_em = em
            if len(final) and (self.stage is None or self.stage.shape[1] < b.m):
                self.stage = np.empty((K, b.m), dtype=np.float32)
            self.stream.push(em, plan.run_iters, plan.final, self.lo, self.hi, plan.chains, plan.add_sums,
                             self.stage if len(final) else None)
            for k in final:
                self.af[b.site0:b.site0 + b.m, k] = self.stage[k, :b.m]
            pushed += b.m
            if pushed >= self.stream.m_total:
                break
        S, C = self.stream.read()
        self.stats["round_seconds"].append(time.perf_counter() - t0)
        self.want_more = True       # asked by stream_windows when the next round takes its first window
        return S, C


def emMAF_windowed(path, IDs, maf_iter, tole, window_sites=None, out=None, ctx=None, keep=None):
    """emMAF_populations for a Beagle FILE whose matrix need not fit the device: the sites are fitted in consecutive windows of
    `window_sites` sites (a multiple of 8192, rounded down; None: WGSASSIGN_WINDOW_SITES, else what windows.plan_fit derives from
    the free device memory), in rounds over the file (windowed_fit.py: the stopping iteration of every fit from sums and chains
    gathered over all windows, then every window run to exactly that iteration).  Returns (af, iters): af the (m, K) float32
    frequencies clamped per WGSassign.py:236-240 -- an np.lib.format.open_memmap at `out` when given, so the host holds one
    window of them -- and iters (K,), bit for bit what emMAF_populations gives on the resident matrix.  Prints nothing.
    emMAF_windowed.stats: rounds, windows, window_sites, chain_iterations, largest_matrix_bytes, matrices, seconds,
    round_seconds, iterations_round1 (EM iterations round 1 ran per site, all fits) against iterations_needed (the sum of the
    fits' stopping iterations);
    emMAF_windowed.info: n, m, sample_names, site_names (the first and last four), pops.
    keep (a bool array over the file's rows): the fits run over the KEPT sites, numbered as stream_to_device(path, keep=keep) numbers
    them -- m, the rows of af, the windows and the names are those of kept sites (reader_cy.stream_windows)."""
    import time

    from . import reader_cy, utils, windowed_fit, windows
    from .device import EMStream, get_context
    ctx = ctx or get_context()
    t0 = time.perf_counter()
    pops, group_of, counts = utils.population_groups(np.asarray(IDs))
    K = len(pops)
    index, _, m = reader_cy.ensure_index(path)
    if keep is not None:
        keep = np.asarray(keep, dtype=bool)
        if keep.ndim != 1 or len(keep) != m:
            raise ValueError("the site mask has %d entries, %s holds %d sites" % (keep.size, path, m))
        m = int(np.count_nonzero(keep))
    if m <= 0:
        raise ValueError("%s holds no sites" % path)
    if window_sites is None:
        W = windows.env_window_sites()
        if W is None:
            W = windows.plan_fit(m, len(group_of), K, ctx.mem_info()[0]) or windows.whole_file_window(m)
    else:
        W = windows.explicit_window(window_sites)
    groups = utils.checked_groups(group_of, K)
    af = np.empty((m, K), dtype=np.float32) if out is None else np.lib.format.open_memmap(out, mode="w+", dtype=np.float32, shape=(m, K))
    info, stats = {}, {"round_seconds": []}
    stream = EMStream(K, maf_iter, m, ctx)
    rounds = _DeviceRounds(None, stream, counts, af, stats)
    gen = reader_cy.stream_windows(path, W, ctx=ctx, info=info, group_of=groups, n_groups=K, again=rounds.again, keep=keep)
    rounds.windows = gen
    try:
        iters, scheme = windowed_fit.fit(rounds, K, maf_iter, tole, m, EMBatch.GUARD)
    finally:
        rounds.want_more = False
        gen.close()
        for em in rounds.batches.values():
            em.close()
        stream.close()
    if out is not None:
        af.flush()
    stats.update(rounds=scheme.rounds, windows=info["windows"], window_sites=W, chain_iterations=scheme.chain_iterations,
                 largest_matrix_bytes=info["largest_matrix_bytes"], matrices=info["matrices"], seconds=time.perf_counter() - t0,
                 iterations_round1=int(max(0, maf_iter)) * K, iterations_needed=int(sum(scheme.stop)))
    emMAF_windowed.stats = stats
    emMAF_windowed.info = dict({k: info[k] for k in ("n", "m", "sample_names", "site_names")}, pops=pops)
    return af, iters
