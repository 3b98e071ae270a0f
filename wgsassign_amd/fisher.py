"""Observed Fisher information / effective sample sizes: drop-in for the reference's `fisher.py`
(`--ne_obs`), on the device slabs."""
import numpy as np

from . import _lib
from .device import AFSet, DeviceBeagle


def _slabs(L, IDs):
    pops = np.unique(IDs[:, 1])
    group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
    return DeviceBeagle.from_host(np.asarray(L), group_of, len(pops)), pops


def fisher_obs(L, af, IDs, t=1, beagle=None):
    """fisher.py:11-44: (f_obs, ne_obs), both (m, K) float32 -- per population the per-SNP sum over
    its individuals of the observed-information term (serial float32, file order) and
    0.5 * f * a * (1 - a)."""
    own = beagle is None
    if own:
        beagle, _ = _slabs(L, np.asarray(IDs))
    afs = AFSet.from_host(np.ascontiguousarray(af, dtype=np.float32), ctx=beagle.ctx)
    f_obs = np.empty((beagle.m, afs.K), dtype=np.float32)
    ne_obs = np.empty((beagle.m, afs.K), dtype=np.float32)
    _lib.check(_lib.load().wgs_fisher_obs(beagle.handle, afs.handle, _lib.f32p(f_obs), _lib.f32p(ne_obs)))
    afs.close()
    if own:
        beagle.close()
    return f_obs, ne_obs


def fisher_obs_ind(L, af, IDs, t=1, beagle=None, comm=None, m_total=None, exact_budget_bytes=8 << 30, host_mean=False):
    """fisher.py:46-60: per individual the mean over SNPs of its effective-sample-size term under
    its own population's frequencies.

    Single shard (default): the per-site float32 terms are computed on the device in batches of
    individuals and np.mean of each row is formed there exactly as NumPy forms it (pairwise float32
    summation, float64 division; csrc/em_kernels.hip: pairwise_leaf_kernel) -- bit-identical to the
    reference without moving n x m floats over PCIe; host_mean=True downloads the rows and calls np.mean
    itself (the cross-check).  SNP-sharded (comm given): the same running float32 total continued from shard to
    shard in SNP order (wgs_fisher_ind_sums) -- bit-identical as well."""
    own = beagle is None
    if own:
        beagle, _ = _slabs(L, np.asarray(IDs))
    afs = AFSet.from_host(np.ascontiguousarray(af, dtype=np.float32), ctx=beagle.ctx)
    lib = _lib.load()
    if comm is not None and comm.world > 1:
        # np.mean's running float32 total handed from shard to shard in SNP order (shards start at multiples of NumPy's
        # 8192-element chunks: comm.shard_range); the batches must be the same on every rank
        from .comm import SHARD_ALIGN, relay, shard_range
        out = np.zeros(beagle.n, dtype=np.float32)
        group_of = beagle.group_of
        aligned = m_total // comm.world >= SHARD_ALIGN          # else the shards cut through NumPy's summation tree
        batch = int(max(1, min(256, exact_budget_bytes // max(1, 4 * (m_total // comm.world + 8192)))))
        if not aligned:
            batch = int(max(1, min(batch, (64 << 20) // max(1, 8 * m_total))))
        lo, hi = shard_range(m_total, comm.rank, comm.world)
        i = 0
        while i < beagle.n:
            j = i + 1
            while j < beagle.n and j - i < batch and group_of[j] == group_of[i]:
                j += 1
            if not aligned:
                # few sites (< 8192 per rank): the rows themselves are small -- every rank contributes its columns of the
                # (individuals x all sites) matrix and np.mean is applied to whole rows, as on one shard
                rows = np.empty((j - i, beagle.m), dtype=np.float32)
                _lib.check(lib.wgs_fisher_ind_sites(beagle.handle, afs.handle, i, j - i, _lib.f32p(rows)))
                full = np.zeros((j - i, m_total), dtype=np.float64)
                full[:, lo:hi] = rows
                full = comm.allreduce_sum(full).astype(np.float32)             # float32 values: exact in float64
                for r in range(j - i):
                    out[i + r] = out[i + r] + np.mean(full[r])                  # fisher.py:59
                i = j
                continue

            def step(run):
                mine = np.zeros(j - i, dtype=np.float32)
                _lib.check(lib.wgs_fisher_ind_sums(beagle.handle, afs.handle, i, j - i, _lib.f32p(run) if run is not None else None,
                                                   _lib.f32p(mine)))
                return mine
            run = relay(comm, step, (j - i,), np.float32)
            out[i:j] = (run.astype(np.float64) / m_total).astype(np.float32)      # np.mean: float64 division, float32 result
            i = j
    else:
        out = np.zeros(beagle.n, dtype=np.float32)
        m, group_of = beagle.m, beagle.group_of
        budget = min(exact_budget_bytes, 1 << 30) if host_mean else exact_budget_bytes       # host rows vs device workspace
        batch = int(max(1, min(256, budget // max(1, 4 * m))))
        i = 0
        while i < beagle.n:
            j = i + 1
            while j < beagle.n and j - i < batch and group_of[j] == group_of[i]:
                j += 1
            if host_mean:
                rows = np.empty((j - i, m), dtype=np.float32)
                _lib.check(lib.wgs_fisher_ind_sites(beagle.handle, afs.handle, i, j - i, _lib.f32p(rows)))
                for r in range(j - i):
                    out[i + r] = out[i + r] + np.mean(rows[r])        # fisher.py:59
            else:
                means = np.empty(j - i, dtype=np.float32)
                _lib.check(lib.wgs_fisher_ind_means(beagle.handle, afs.handle, i, j - i, _lib.f32p(means)))
                out[i:j] = out[i:j] + means                           # 0 + np.mean(...)
            i = j
    afs.close()
    if own:
        beagle.close()
    return out


def continue_column_sum(running, rows):
    """np.add.reduce(a, axis=0) of an (m, K) float32 array, continued: `running` is the reduce over the rows before `rows` (None:
    there are none).  NumPy forms that reduce as a serial float32 chain down each column, row after row, so the chain goes on
    from `running` over the new rows as it would have inside one call.  ONE column is a contiguous vector, which NumPy sums as
    fisher_obs_ind's rows are summed (csrc/api.hip: PairwisePlan): pairwise within every 8192 elements, those sums added to the
    running total in order -- so `rows` then begins at a multiple of 8192 rows, as every window does."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.shape[1] == 1:
        for lo in range(0, rows.shape[0], 8192):
            chunk = np.add.reduce(rows[lo:lo + 8192], axis=0)
            running = chunk if running is None else running + chunk
        return running
    if running is None:
        return np.add.reduce(rows, axis=0)
    return np.add.reduce(np.concatenate([running[None], rows]), axis=0)


def column_mean(total, m):
    """np.mean(a, axis=0)'s last step on the column sums of m rows: the very call NumPy makes (for m > 2**24 the divisor rounds
    to float32 there, too)."""
    total = np.array(total, dtype=np.float32, copy=True)
    return np.true_divide(total, m, out=total, casting="unsafe")


def fisher_obs_windowed(path, af, IDs, window_sites=None, out=None, ctx=None):
    """fisher_obs, np.mean(ne_obs, axis=0) and fisher_obs_ind for a Beagle FILE whose matrix need not fit the device, from ONE pass
    over the file in consecutive windows of `window_sites` sites (a multiple of 8192, rounded down; None: WGSASSIGN_NE_WINDOW_SITES,
    else what windows.plan_ne derives from the free device memory -- one window when everything fits).  af: the (m, K) fitted
    frequencies, an array or an np.load(..., mmap_mode="r") view; rows [lo, hi) are uploaded per window.  Per window one fused sweep
    (csrc/em_kernels.hip: fisher_window_kernel) gives its rows of f_obs and ne_obs and the leaf sums of NumPy's pairwise float32 sum
    of every individual's per-site terms; the running totals stay on the device (device.FisherStream).  Returns
    (f_obs, ne_obs, ne_obs_mean, ne_ind): f_obs, ne_obs (m, K) float32 -- np.lib.format.open_memmap files out + ".fisher_obs.npy" /
    ".ne_obs.npy" when `out` is given, written window by window, so the host holds one window's rows --, ne_obs_mean (K,) float32 =
    np.mean(ne_obs, axis=0) and ne_ind (n,) float32, all bit for bit what the resident functions give.
    fisher_obs_windowed.stats: windows, window_sites, largest_matrix_bytes, matrices, seconds, sweep_ms (per window);
    fisher_obs_windowed.info: n, m, sample_names, site_names (the first and last four), pops."""
    import time

    from . import reader_cy, utils, windows
    from .device import FisherStream, get_context
    ctx = ctx or get_context()
    t0 = time.perf_counter()
    pops, group_of, counts = utils.population_groups(np.asarray(IDs))
    K = len(pops)
    if af.ndim != 2 or af.shape[1] != K:
        raise ValueError("the allele frequencies must be an (m, %d) matrix" % K)
    index, _, m = reader_cy.ensure_index(path)
    if m <= 0:
        raise ValueError("%s holds no sites" % path)
    if af.shape[0] != m:
        raise ValueError("the allele frequencies have %d sites, the Beagle file %d" % (af.shape[0], m))
    if window_sites is None:
        W = windows.env_window_sites(name=windows.ENV_NE)
        if W is None:
            W = windows.plan_ne(m, len(group_of), K, ctx.mem_info()[0], counts=counts) or windows.whole_file_window(m)
    else:
        W = windows.explicit_window(window_sites)
    groups = utils.checked_groups(group_of, K)

    def result(suffix):
        if out is None:
            return np.empty((m, K), dtype=np.float32)
        return np.lib.format.open_memmap(out + suffix, mode="w+", dtype=np.float32, shape=(m, K))

    f_obs, ne_obs = result(".fisher_obs.npy"), result(".ne_obs.npy")
    info, stream, running = {}, None, None
    gen = reader_cy.stream_windows(path, W, ctx=ctx, info=info, group_of=groups, n_groups=K)
    try:
        for b in gen:
            if stream is None:
                stream = FisherStream(b.n, K, m, ctx)
            lo, hi = b.site0, b.site0 + b.m
            afs = AFSet.from_host(np.ascontiguousarray(af[lo:hi], dtype=np.float32), ctx=ctx)
            try:
                f_rows, ne_rows = stream.push(b, afs)
            finally:
                afs.close()
            f_obs[lo:hi] = f_rows
            ne_obs[lo:hi] = ne_rows
            running = continue_column_sum(running, ne_rows)        # np.mean(ne_obs, axis=0): WGSassign.py:401
        ne_ind = stream.finish()
        sweep_ms = list(stream.sweep_ms)
    finally:
        gen.close()
        if stream is not None:
            stream.close()
    if out is not None:
        f_obs.flush()
        ne_obs.flush()
    fisher_obs_windowed.stats = {"windows": info["windows"], "window_sites": W, "largest_matrix_bytes": info["largest_matrix_bytes"],
                                 "matrices": info["matrices"], "seconds": time.perf_counter() - t0, "sweep_ms": sweep_ms}
    fisher_obs_windowed.info = dict({k: info[k] for k in ("n", "m", "sample_names", "site_names")}, pops=pops)
    return f_obs, ne_obs, column_mean(running, m), ne_ind
