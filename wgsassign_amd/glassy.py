"""Assignment log-likelihoods and leave-one-out: drop-in for the reference's `glassy.py`."""
import numpy as np

import os

from .device import MAX_BLOCK_PARALLEL_PARTS, AFSet, DeviceBeagle, EMBatch, Score, assign, partition_sums_exact


def assignLL(L, af, t=1):
    """glassy.py:18-44: (n, K) float32 matrix of summed per-site log-likelihoods.

    One sweep over the device-resident matrix produces all n*K sums (the reference rescans L
    once per pair); sums are accumulated in float64 like np.sum(..., dtype=float) (glassy.py:38)
    and stored as float32 (glassy.py:42).
    """
    L = np.asarray(L)
    af = np.ascontiguousarray(af, dtype=np.float32)
    n = L.shape[1] // 2
    k = af.shape[1]
    print(str(n) + " individuals to assign to " + str(k) + " populations")
    if n == 0 or L.shape[0] == 0:
        return np.zeros((n, k), dtype=np.float32)
    beagle = DeviceBeagle.from_host(L)
    afset = AFSet.from_host(af[:L.shape[0]])
    out, _ = assign(beagle, afset)
    afset.close()
    beagle.close()
    with np.errstate(over="ignore"):
        return out.astype(np.float32)


def assignLL_windowed(path, A, window_sites=None, ctx=None, mode=None):
    """The (n, K) float64 sums of assignLL for a Beagle FILE whose matrix need not fit the device: its sites are scored in
    consecutive windows of `window_sites` sites (a multiple of 8192, rounded down; None: WGSASSIGN_WINDOW_SITES, else what
    windows.plan derives from the free device memory -- one window when everything fits).  A: the (m, K) frequencies, an array
    or an np.load(..., mmap_mode="r") view; rows [lo, hi) are uploaded per window.  Two window matrices exist at most
    (reader_cy.stream_windows), np.sum's running total stays on the device between the windows (device.ScoreStream): the result
    equals device.assign on the resident matrix bit for bit.
    assignLL_windowed.stats: windows, window_sites, largest_matrix_bytes, matrices (created), seconds, sweep_ms (per window);
    assignLL_windowed.info: n, m, sample_names, site_names (the first and last four)."""
    import time

    from . import reader_cy, windows
    from .device import ScoreStream, get_context
    ctx = ctx or get_context()
    t0 = time.perf_counter()
    if A.ndim != 2:
        raise ValueError("the allele frequencies must be an (m, K) matrix")
    K = A.shape[1]
    if window_sites is None:
        W = windows.env_window_sites()
        if W is None:
            index, _, m = reader_cy.ensure_index(path)
            with reader_cy.BeagleStream(path, threads=1, index=index, first_row=0) as st:
                n = st.n
            W = windows.plan(m, n, K, ctx.mem_info()[0]) or windows.whole_file_window(m)
    else:
        W = windows.explicit_window(window_sites)
    info, stream = {}, None
    gen = reader_cy.stream_windows(path, W, ctx=ctx, info=info)
    try:
        for b in gen:
            if stream is None:
                if A.shape[0] != info["m"]:
                    raise ValueError("the allele frequency file has %d sites, the Beagle file %d" % (A.shape[0], info["m"]))
                stream = ScoreStream(b.n, K, info["m"], ctx)
            afs = AFSet.from_host(np.ascontiguousarray(A[b.site0:b.site0 + b.m], dtype=np.float32), ctx=ctx)
            try:
                stream.push(b, afs, mode)
            finally:
                afs.close()
        if stream is None:
            raise ValueError("%s holds no sites" % path)
        out = stream.finish()
        sweep_ms = list(stream.sweep_ms)
    finally:
        gen.close()
        if stream is not None:
            stream.close()
    assignLL_windowed.stats = {"windows": info["windows"], "window_sites": W, "largest_matrix_bytes": info["largest_matrix_bytes"],
                               "matrices": info["matrices"], "seconds": time.perf_counter() - t0, "sweep_ms": sweep_ms}
    assignLL_windowed.info = {k: info[k] for k in ("n", "m", "sample_names", "site_names")}
    return out


def loo(L, af, IDs, t, maf_iter, maf_tole, downsampled_L=None, num_partitions=1, need_parts=True):
    """glassy.py:47-112: leave-one-out assignment log-likelihoods.

    Semantics kept from the reference:
      * individual i's own population column is re-estimated without i (glassy.py:65-78) and
        clamped with n_pop = |pop| - 1 (glassy.py:80-85);
      * that column OVERWRITES af[:, pop_col] and is never restored (glassy.py:87-89), so when i
        is scored every other column holds the leave-one-out estimate of the most recent earlier
        individual of that population (or the full-population estimate if there was none);
        `af` is mutated in place and ends up holding each population's LAST re-fit;
      * scoring uses downsampled_L when given (glassy.py:96-98);
      * per-partition sums use labels = site index % num_partitions (utils.py:147).
    All n re-fits run as one batch of EM chains on the device; one scoring sweep follows.
    Returns (logl_mat (n, K) float32, logl_parts_mat (n*P, K) float32).  The partition sums are the
    reference's serial float32 accumulations, bit for bit (WGSASSIGN_PARTS=fast: float64 sums, ~1e-5).
    need_parts=False with num_partitions == 1 skips that chain (the reference's CLI never writes the
    one-partition matrix) and returns the totals in its place.
    """
    L = np.asarray(L)
    IDs = np.asarray(IDs)
    m = L.shape[0]
    n = L.shape[1] // 2
    k = af.shape[1]
    P = int(num_partitions)
    print(str(n) + " individuals to assign to " + str(k) + " populations")
    if downsampled_L is not None:
        print("Using downsampled GLs for likelihood evaluation in LOO assignment.")
    if m == 0 or n == 0:
        # glassy.py:65-109 over no SNPs: every re-fit and every per-site vector is empty, np.sum([]) = 0.0
        return np.zeros((n, k), dtype=np.float32), np.zeros((n * P, k), dtype=np.float32)
    pops = np.unique(IDs[:, 1])
    group_of = np.searchsorted(pops, IDs[:n, 1]).astype(np.int32)
    beagle = DeviceBeagle.from_host(L, group_of, len(pops))
    scored = DeviceBeagle.from_host(np.asarray(downsampled_L), group_of, len(pops)) if downsampled_L is not None else beagle
    logl, logl_parts = loo_device(beagle, scored, af, group_of, maf_iter, maf_tole, P, need_parts=need_parts)
    if scored is not beagle:
        scored.close()
    beagle.close()
    return logl, logl_parts


def loo_column_table(afset, em, group_of, i0, i1):
    """(n, K) table of device addresses for scoring individuals [i0, i1): individual i is scored against
    its own re-fit (fit i - i0 of `em`) and, for every other population, the re-fit of the most recent
    earlier individual of that population, else the column of `afset` (glassy.py:87-105, the sticky
    overwrite).  Rows outside [i0, i1) hold valid placeholders."""
    n, k = len(group_of), afset.K
    cur = [afset.col_dev(j) for j in range(k)]
    colptr = np.empty((n, k), dtype=np.uint64)
    colptr[:] = cur
    for i in range(i0, i1):
        cur[group_of[i]] = em.f_dev(i - i0)
        colptr[i] = cur
    return colptr


def score_loo_batch(scored, afset, em, group_of, i0, i1, P=1, exact_parts=True, comm=None, timings=None):
    """Scoring step of glassy.py:92-109 for individuals [i0, i1) whose converged, clamped re-fits are the
    fits of `em`: returns (sums (n, K) float64, partition sums (n*P, K) or None).  Only rows [i0, i1) are
    computed (a batch scores its own individuals); the other rows are 0."""
    colptr = loo_column_table(afset, em, group_of, i0, i1)
    if not exact_parts:
        if P == 1:
            sc = Score(scored, afset, colptr, rows=(i0, i1))
            o = sc.sums(comm=comm)
            sc.close()
            return o, None
        return assign(scored, afset, colptr=colptr, P=P, comm=comm)      # float64 partition sums (WGSASSIGN_PARTS=fast)
    # sums over all sites in float64 (np.sum(dtype=float), glassy.py:101); partition sums literally as
    # utils.py:147-149 accumulates them (serial float32) -- for P == 1 too (glassy.py:108-109)
    from ._lib import MODE_EXACT
    if P > MAX_BLOCK_PARALLEL_PARTS:
        o, _ = assign(scored, afset, colptr=colptr, P=1, comm=comm)
        return o, partition_sums_exact(scored, afset, colptr=colptr, P=P, comm=comm)
    sc = Score(scored, afset, colptr, rows=(i0, i1))
    o = sc.sums(MODE_EXACT, comm)
    pr = sc.parts_exact(P, comm)
    if timings is not None:
        for k, v in sc.ms.items():
            timings[k + "_ms"] = timings.get(k + "_ms", 0.0) + v
        timings["serial_blocks"] = sc.serial_blocks()
    sc.close()
    return o, pr


def loo_device(beagle, scored, af, group_of, maf_iter, maf_tole, P=1, comm=None, verbose=True, timings=None,
               need_parts=True, inspect=None):
    """The body of loo() on device-resident matrices: `beagle` holds the GLs the frequencies are
    re-estimated from, `scored` the GLs that are scored (the same object unless a downsampled
    matrix is given), both with population slabs `group_of`.  `af` (m, K) float32 is mutated like
    glassy.py:87-89 does.  With `comm`, SNPs are sharded over ranks (af is this rank's shard).
    inspect(em, i0, i1), if given, is called with each batch's converged and clamped fits."""
    import time
    n, k = beagle.n, af.shape[1]
    counts = np.bincount(group_of, minlength=k)
    exact_parts = os.environ.get("WGSASSIGN_PARTS", "exact") != "fast" and (need_parts or P > 1)
    handle = getattr(comm, "handle", None) if comm is not None and comm.world > 1 else None
    one_call = (comm is None or comm.world == 1 or handle is not None) and inspect is None \
        and (exact_parts or P == 1) and P <= MAX_BLOCK_PARALLEL_PARTS and os.environ.get("WGSASSIGN_LOO", "c") != "python"
    if one_call:
        # the whole of glassy.py:65-109 behind one C entry (wgs_loo); the Python orchestration below does the
        # same through the step-wise entry points and serves the other communicators (gloo / socket)
        import ctypes
        from . import _lib
        from .device import default_em_mode, default_mode
        t0 = time.perf_counter()
        afset = AFSet.from_host(np.ascontiguousarray(af, dtype=np.float32))
        m_total = int(comm.allreduce_sum(np.array([float(beagle.m)]))[0]) if handle is not None else beagle.m
        out = np.zeros((n, k), dtype=np.float64)
        parts = np.zeros((n * P, k), dtype=np.float32) if exact_parts else None
        iters = np.zeros(n, dtype=np.int32)
        _lib.check(_lib.load().wgs_loo(beagle.handle, scored.handle if scored is not beagle else None, afset.handle,
                                       int(maf_iter), float(maf_tole), m_total, handle, P,
                                       int(os.environ.get("WGSASSIGN_LOO_BATCH", 0)), default_em_mode(), default_mode(), _lib.f64p(out),
                                       _lib.f32p(parts) if parts is not None else None, _lib.i32p(iters)))
        if verbose:
            for i in range(n):
                if iters[i] > 0:
                    print("EM (MAF) converged at iteration: " + str(int(iters[i])))
        af[:, :] = afset.to_host()
        afset.close()
        if timings is not None:
            st = (ctypes.c_double * 7)()
            _lib.check(_lib.load().wgs_loo_stats(st))
            timings.update(seconds=time.perf_counter() - t0, iters=iters, one_call=True, em_seconds=st[0], score_seconds=st[1],
                           chain_seconds=st[2], em_sweep_kernel_ms=st[3], em_batches=int(st[4]), em_chain_resolutions=int(st[5]),
                           em_iterations_enqueued=int(st[6]))
        with np.errstate(over="ignore"):
            logl = out.astype(np.float32)
        return logl, (parts if parts is not None else logl.copy())
    # The n re-fits need 2 float32 vectors + the per-tile partial sums each (~8.2 bytes per SNP and fit).
    # They run as ONE batch when that fits the free device memory, else in file-order batches: the
    # "current" columns (afset) carry the sticky overwrite from batch to batch.
    batch = loo_batch_size(beagle, n, comm)
    afset = AFSet.from_host(np.ascontiguousarray(af, dtype=np.float32))
    out = np.zeros((n, k), dtype=np.float64)
    parts = np.zeros((n * P, k), dtype=np.float64 if not exact_parts else np.float32) if (P > 1 or exact_parts) else None
    iters = np.zeros(n, dtype=np.int32)
    t_em = t_score = 0.0
    for i0 in range(0, n, batch):
        i1 = min(n, i0 + batch)
        t0 = time.perf_counter()
        em = EMBatch(beagle, group_of[i0:i1], np.arange(i0, i1, dtype=np.int32))
        iters[i0:i1] = em.run(maf_iter, maf_tole, comm=comm)
        beagle.ctx.sync()
        t1 = time.perf_counter()
        for i in range(i0, i1):
            if verbose and iters[i] > 0:
                print("EM (MAF) converged at iteration: " + str(int(iters[i])))
            em.clamp(i - i0, int(counts[group_of[i]]) - 1)
        if inspect is not None:
            inspect(em, i0, i1)
        o, pr = score_loo_batch(scored, afset, em, group_of, i0, i1, P, exact_parts, comm, timings)
        out[i0:i1] = o[i0:i1]
        if parts is not None and pr is not None:
            parts[i0 * P:i1 * P] = pr[i0 * P:i1 * P]
        # the last re-fit of each population in this batch becomes the current column
        last = {int(g): i for i, g in zip(range(i0, i1), group_of[i0:i1])}
        for g, i in last.items():
            afset.set_column_from_em(g, em, i - i0)
        beagle.ctx.sync()
        em.close()
        t_em += t1 - t0
        t_score += time.perf_counter() - t1
    af[:, :] = afset.to_host()           # glassy.py:89: the caller's af ends up holding each population's last re-fit
    afset.close()
    if timings is not None:
        timings.update(em_seconds=t_em, score_seconds=t_score, iters=iters, batch=batch)
    with np.errstate(over="ignore"):
        logl = out.astype(np.float32)
        logl_parts = parts.astype(np.float32) if parts is not None else logl.copy()
    return logl, logl_parts


# Iterations a re-fit's first horizon lies beyond the stopping iteration of its population's full fit: the largest t*_i - t*_pop(i)
# tools/measure_loo_margin.py found on the resident --loo at 2M x 500 x K=8 and 5M x 180 x K=5 (0 for every
# re-fit at depth 2 and 8, +1 for 36 of 180 at depth 0.5).  A re-fit that stops later than that costs one extension round.
LOO_MARGIN = 1


def loo_first_iters(group_of, pop_iters, maf_iter, margin=None):
    """The first horizon of every leave-one-out re-fit (windowed_fit.RoundScheme): the stopping iteration of its population's
    full fit plus LOO_MARGIN, maf_iter where that fit was exhausted (pop_iters[k] == 0).  Only the number of rounds depends on
    it, never the result."""
    margin = LOO_MARGIN if margin is None else int(margin)
    pop_iters = np.asarray(pop_iters)
    return [int(maf_iter) if pop_iters[g] <= 0 else min(int(maf_iter), int(pop_iters[g]) + margin) for g in group_of]


class _LooRounds:
    """windowed_fit's backend for the leave-one-out re-fits: a round is one pass of reader_cy.stream_windows, every window pushed
    through the EMBatch of its matrix (n re-fits, kept for every window and round) into one device.EMStream; in the last round --
    every fit final -- the batch stays on the device and the window is scored into one device.LooStream.  scored (optional): a second
    reader_cy.stream_windows, over the file whose likelihoods are scored; it is advanced in the last round only, one window beside
    every re-fit batch, so that file is read once."""

    def __init__(self, windows, stream, loo, group_of, counts, af, stats, mode, scored=None):
        self.windows, self.stream, self.loo, self.group_of, self.af, self.stats, self.mode = windows, stream, loo, group_of, af, stats, mode
        self.scored, self.scored_passes = scored, 0
        lo = 1 / (2 * (np.asarray(counts, dtype=np.float64)[group_of] - 1 + 1))        # glassy.py:80-85 with n_pop = |pop| - 1, as EMBatch.clamp forms them
        self.lo, self.hi = lo.astype(np.float32), (1 - lo).astype(np.float32)
        self.batches = {}
        self.want_more = False

    def again(self):
        return self.want_more

    def run_round(self, plan):
        import time
        t0 = time.perf_counter()
        n = self.stream.n_fits
        final = bool(plan.final.any())
        if final and not plan.final.all():
            raise RuntimeError("a leave-one-out window is scored with every re-fit final, or not at all")
        pushed = 0
        for b in self.windows:
            em = self.batches.get(id(b))
            if em is None:          # one EMBatch per window matrix, made once and kept for every window and round
                em = self.batches[id(b)] = EMBatch(b, self.group_of, np.arange(n, dtype=np.int32))
                b.window_em = em
            self.stream.push_keep(em, plan.run_iters, plan.final if final else None, self.lo, self.hi, plan.chains,
                                  plan.sums_from if plan.add_sums else None)
            if final:
                afs = AFSet.from_host(np.ascontiguousarray(self.af[b.site0:b.site0 + b.m], dtype=np.float32), ctx=self.stream.ctx)
                try:
                    sb = None
                    if self.scored is not None:
                        sb = next(self.scored, None)    # the downsampled file's window of the same kept sites
                        if sb is None:
                            raise RuntimeError("the scored file ran out of windows before the fitted one")
                        if sb.site0 == 0:
                            self.scored_passes += 1
                    self.loo.push(em, afs, self.mode, scored=sb)
                finally:
                    afs.close()
            pushed += b.m
            if pushed >= self.stream.m_total:
                break
        S, C = self.stream.read()
        self.stats["round_seconds"].append(time.perf_counter() - t0)
        self.want_more = True       # asked by stream_windows when the next round takes its first window
        return S, C


def loo_windowed(path, af, IDs, maf_iter, maf_tole, window_sites=None, num_partitions=1, need_parts=True, pop_iters=None,
                 first_iters=None, ctx=None, keep=None, scored_path=None, scored_keep=None):
    """loo_device for a Beagle FILE whose matrix need not fit the device: (logl (n, K) float32, parts (n*P, K) float32, iters (n,)),
    bit for bit what loo_device returns on the resident matrix of the same file.  The sites are taken in consecutive windows of
    `window_sites` sites (a multiple of 8192, rounded down; None: WGSASSIGN_LOO_WINDOW_SITES, else what windows.plan_loo derives
    from the free device memory), in rounds over the file (windowed_fit.py): the n re-fits of a window are ONE EM batch
    (WGSASSIGN_LOO_BATCH does not apply), their stopping iterations are found from sums and chains gathered over all windows, and
    one last round runs every re-fit to its stop, clamps it with n_pop - 1 and scores the window (device.LooStream) -- the re-fits
    never leave the device.
    af: the (m, K) full-population estimates, an array or an np.load(..., mmap_mode="r") view; rows [lo, hi) are uploaded per
    window.  Unlike loo(), af is NOT mutated.  pop_iters (K,): the iteration counts of the full fits, from which the re-fits' first
    horizons are taken (loo_first_iters); first_iters (n,) gives them outright; neither: round 1 runs maf_iter iterations.
    Prints nothing.
    keep (a bool array over the file's rows): the run is over the KEPT sites, numbered as stream_to_device(path, keep=keep) numbers
    them (partition labels, np.sum's chunks, the rows of af, the windows: reader_cy.stream_windows).  scored_path: a second Beagle
    file whose likelihoods are SCORED in place of those the re-fits are made from (--loo_downsampled_beagle; loo_device's `scored`),
    under its own mask scored_keep (None: unfiltered); window w of both files holds the same kept sites.  The rounds before the
    last stream `path` alone; the last round advances the second stream beside the first, so the second file is read once
    (stats: scored_passes == 1).  The sample names and the kept counts of the two files must agree.  With scored_path and
    window_sites=None, WGSASSIGN_LOO_DS_WINDOW_SITES and windows.plan_loo_ds stand in for the variable and the plan named above.
    loo_windowed.stats: rounds, windows, window_sites, chain_iterations, largest_matrix_bytes, matrices, seconds, round_seconds,
    iterations_round1 (the sum of the first horizons) against iterations_needed (the sum of the stopping iterations),
    extension_rounds, refit_bytes_to_host (0: no re-fit frequencies cross to the host), scored_passes (passes over scored_path;
    matrices and largest_matrix_bytes count both files' matrices: at most four);
    loo_windowed.info: n, m, sample_names, site_names (the first and last four), pops."""
    import time

    from . import reader_cy, utils, windowed_fit, windows
    from .device import EMStream, LooStream, default_mode, get_context
    ctx = ctx or get_context()
    t0 = time.perf_counter()
    pops, group_of, counts = utils.population_groups(np.asarray(IDs))
    n, K, P = len(group_of), len(pops), int(num_partitions)
    if af.ndim != 2 or af.shape[1] != K:
        raise ValueError("the allele frequencies must be an (m, %d) matrix" % K)
    if P < 1:
        raise ValueError("partition count must be >= 1")
    exact_parts = os.environ.get("WGSASSIGN_PARTS", "exact") != "fast" and (need_parts or P > 1)
    if P > 1 and not exact_parts:
        raise ValueError("WGSASSIGN_PARTS=fast (float64 partition sums) is not provided in site windows")
    if scored_keep is not None and scored_path is None:
        raise ValueError("scored_keep is the site mask of scored_path: it cannot be given without that file")

    def kept_sites(file, mask):
        m_file = reader_cy.ensure_index(file)[2]
        if mask is None:
            return None, m_file
        mask = np.asarray(mask, dtype=bool)
        if mask.ndim != 1 or len(mask) != m_file:
            raise ValueError("the site mask has %d entries, %s holds %d sites" % (mask.size, file, m_file))
        return mask, int(np.count_nonzero(mask))

    keep, m = kept_sites(path, keep)
    if m <= 0:
        raise ValueError("%s holds no sites" % path)
    if scored_path is not None:
        # the resident route's checks (WGSassign.py:172-198), before anything is fitted
        with reader_cy.BeagleStream(path, threads=1) as st, reader_cy.BeagleStream(scored_path, threads=1) as st_scored:
            if list(st.sample_names) != list(st_scored.sample_names):
                raise ValueError("Sample names in downsampled Beagle file do not match original.")
        scored_keep, m_scored = kept_sites(scored_path, scored_keep)
        if m_scored != m:
            raise ValueError("Site names in full and downsampled Beagle do not match after filtering.")
    if af.shape[0] != m:
        raise ValueError("the allele frequency file has %d sites, the Beagle file %d" % (af.shape[0], m))
    if window_sites is None:
        W = windows.env_window_sites(name=windows.ENV_LOO_DS if scored_path is not None else windows.ENV_LOO)
        if W is None:
            planned = (windows.plan_loo_ds if scored_path is not None else windows.plan_loo)(m, n, K, ctx.mem_info()[0], counts=counts, P=P)
            W = planned or windows.whole_file_window(m)
    else:
        W = windows.explicit_window(window_sites)
    if first_iters is None and pop_iters is not None:
        first_iters = loo_first_iters(group_of, pop_iters, maf_iter)
    groups = utils.checked_groups(group_of, K)
    info, info_scored, stats = {}, {}, {"round_seconds": []}
    stream = EMStream(n, maf_iter, m, ctx)
    loo_stream = LooStream(n, K, m, P if exact_parts else 0, ctx)
    gen_scored = None
    if scored_path is not None:     # (a generator: nothing is opened before the last round takes its first window)
        gen_scored = reader_cy.stream_windows(scored_path, W, ctx=ctx, info=info_scored, group_of=groups, n_groups=K, keep=scored_keep)
    rounds = _LooRounds(None, stream, loo_stream, group_of, counts, af, stats, default_mode(), scored=gen_scored)
    gen = reader_cy.stream_windows(path, W, ctx=ctx, info=info, group_of=groups, n_groups=K, again=rounds.again, keep=keep)
    rounds.windows = gen
    try:
        iters, scheme = windowed_fit.fit(rounds, n, maf_iter, maf_tole, m, EMBatch.GUARD, first_iters=first_iters, hold_final=True)
        out, parts = loo_stream.finish()
    finally:
        rounds.want_more = False
        gen.close()
        if gen_scored is not None:
            gen_scored.close()
        for em in rounds.batches.values():
            em.close()
        loo_stream.close()
        stream.close()
    stats.update(rounds=scheme.rounds, windows=info["windows"], window_sites=W, chain_iterations=scheme.chain_iterations,
                 largest_matrix_bytes=max(info["largest_matrix_bytes"], info_scored.get("largest_matrix_bytes", 0)),
                 matrices=info["matrices"] + info_scored.get("matrices", 0), seconds=time.perf_counter() - t0,
                 iterations_round1=scheme.iterations_round1, iterations_needed=int(sum(scheme.stop)),
                 extension_rounds=scheme.extension_rounds, refit_bytes_to_host=0, scored_passes=rounds.scored_passes)
    loo_windowed.stats = stats
    loo_windowed.info = dict({k: info[k] for k in ("n", "m", "sample_names", "site_names")}, pops=pops)
    with np.errstate(over="ignore"):
        logl = out.astype(np.float32)
    return logl, (parts if parts is not None else logl.copy()), iters


def loo_batch_size(beagle, n, comm=None):
    """Number of leave-one-out re-fits per EM batch: what fits the free device memory (or
    WGSASSIGN_LOO_BATCH), agreed across SNP-shard ranks -- every rank must build batches of the same
    fits or the per-iteration all-reduces stop matching -- by taking the minimum over ranks."""
    free_bytes, _ = beagle.ctx.mem_info()
    per_fit = int(beagle.m * 8.2) + 4096
    batch = int(os.environ.get("WGSASSIGN_LOO_BATCH", max(1, min(n, int(0.8 * free_bytes) // per_fit))))
    batch = max(1, min(n, batch))
    if comm is not None and comm.world > 1:
        slots = np.zeros(comm.world)
        slots[comm.rank] = batch
        batch = int(np.min(comm.allreduce_sum(slots)))
    return batch
