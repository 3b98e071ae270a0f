"""The reference's `zscore` module (zscore.py) on device-resident data: the z-score of an individual's observed log-likelihood
against its expectation under the population it is assigned to (WGSassign.py:311-446).

Everything that touches every site runs on the GPU, a batch of individuals per launch (csrc/zscore_kernels.hip): the depth-class
sweep (AD_summary's dictionary), the site mask (get_L_keep), the per-site statistic (zscore_cy.expected_W_l / variance_W_l) and,
for the reference flavour, the leave-one-out EM fits whose convergence test runs over the kept sites.  What is a few dozen numbers
per individual stays here in NumPy: the key filter, the tables, and the three float32 sums, which np.sum forms in its own pairwise
order from the compacted per-site arrays.  There is no CPU fallback.

Depth pairs come in two tiers.  Ar + Aa <= 21: the 253 classes of the class sweep, one per thread.  Deeper pairs, up to the 255
reads per allele the device table holds, are rare (collapsed repeats): the device lists those sites (wgs_zscore_deep_sites), their
dictionary entries are formed here, and both tiers merge into one dictionary in order of first appearance.  A deep depth survives
the key filter only with all its d + 1 classes; then its rows travel to the device in a table of their own (deep_tables) and the
mask and statistic sweeps read them there.  Data without deep sites launches nothing of this.  The host part is a loop over the
deep classes of an individual: fine for a few per thousand sites, slow where deep sites are the majority.

Several GPUs (comm with world > 1): every rank holds a contiguous SNP shard -- matrix, depth table, frequencies -- and calls the
drivers together.  What is defined over all sites of an individual crosses the ranks: the class sums as running values handed from
shard to shard (wgs_zscore_classes_sharded), the deep sites as lists put together in rank order, the masked fit's convergence chain
as a carry (wgs_em_fit_masked_sharded), and the per-site arrays themselves, which rank 0 receives and concatenates in rank order --
site order -- so that np.sum forms its pairwise sums over the same arrays as one process would.  Rank 0 prints and returns the
z-scores; the other ranks return None.

Site windows (assignment_z_scores_windowed): the assignment flavour for files whose matrix and depth table do
not fit the device, on one rank.  The same hand-overs in time: the class sums stay on the device from window to window (ZSum.classes),
and the three float32 sums are formed THERE in np.sum's own order -- serial over 8192-element chunks, each a pairwise tree -- from
device arrays that are never downloaded (KeepSet.stats_dev, ZSum.push); the depth file is read once per pass (DepthWindows).
reference_z_scores_windowed is the reference flavour in the same windows: beside those sums the convergence chain of every masked
leave-one-out fit is carried from window to window on the device (device.EMStream.push_masked), in rounds that
windowed_fit.ChainScheme keeps.
"""
import ctypes
import math
import os
import weakref

import numpy as np

from . import _lib
from ._lib import check, f32p, i32p
from .device import Handle, get_context

N_CLASSES = 253      # = WGS_Z_CLASSES: depth pairs (Ar, Aa) with Ar + Aa <= 21, class index d (d + 1) / 2 + Aa -- the dense tier
MAX_DENSE = 21       # = wgs_zscore_max_depth()
DEEP_MAX = 510       # = WGS_Z_DEEP_MAX: 255 reads per allele, what the device table's bytes hold -- the sparse second tier
DEEP_ROW = 8         # floats per row of a deep table (wgs_zkeep_create_deep)
E = 0.01


# ---------------------------------------------------------------- host side: a few dozen numbers per individual
def read_depths(path):
    """--ind_ad_file: text as the reference reads it (np.loadtxt, int32), or .npy as its README describes."""
    if str(path).endswith(".npy"):
        return np.ascontiguousarray(np.load(path), dtype=np.int32)
    return np.ascontiguousarray(np.atleast_2d(np.loadtxt(path, dtype=np.int32)))


def check_depths(AD, m, n):
    if AD.ndim != 2 or AD.shape[0] != m or AD.shape[1] < 2 * n:
        raise ValueError("allele depths have shape %s, the Beagle file has %d sites and %d individuals" % (AD.shape, m, n))
    if AD.size and (AD.min() < 0 or AD.max() > 255):
        raise ValueError("allele depths outside 0..255 do not fit the device table")


def read_majmin(path):
    """--ind_majmin_file: the second argument of the reference's allele_counts_beagle.py (:14) -- one header line, the selectors of
    the major and the minor allele (0..3 = A, C, G, T) in the columns at positions 1 and 2.  uint8 (m, 2)."""
    sel = np.atleast_2d(np.loadtxt(path, dtype="int", skiprows=1, usecols=(1, 2)))
    if sel.size and (sel.min() < 0 or sel.max() > 3):
        row = int(np.argwhere((sel < 0) | (sel > 3))[0][0])
        raise ValueError("%s, line %d: allele selector outside 0..3" % (path, row + 2))
    return np.ascontiguousarray(sel, dtype=np.uint8)


def stream_table(handle, m, path, counts=False, majmin=None, chunk_bytes=None, threads=None, row0=0, limit_rows=-1, first_row=None,
                 m_total=None):
    """The file `path` into the rows row0 .. of the wgs_depth `handle` on the device (wgs_depth_ingest_*).  Returns the stats of
    the ingest.  ValueError names the file's line for anything np.loadtxt would refuse or the table cannot hold, and both numbers
    when the file does not have exactly m - row0 (or limit_rows) data lines.  first_row (not None): the table's m rows are the
    file's data rows [first_row, first_row + m) -- a SNP shard; the whole file is still read and must have m_total data lines."""
    from .reader_cy import host_threads
    lib = _lib.load()
    r, g = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.wgs_reader_open_table(os.fsencode(path), int(threads or host_threads()), 1 if counts else 0, ctypes.byref(r)))
    try:
        sel = None
        if counts:
            sel = np.ascontiguousarray(majmin, dtype=np.uint8)
            if sel.shape != (m, 2):
                raise ValueError("the allele selectors have shape %s, the table %d sites" % (sel.shape, m))
        check(lib.wgs_depth_ingest_create(handle, r, 1 if counts else 0, sel.ctypes.data if counts else None, int(limit_rows),
                                          int(chunk_bytes or 0), ctypes.byref(g)))
        if first_row is not None:
            check(lib.wgs_depth_ingest_set_first_row(g, int(first_row)))
        lines, row = 0, int(row0)
        got, wrote = ctypes.c_int64(), ctypes.c_int64()
        while True:
            check(lib.wgs_depth_ingest_next(g, row, ctypes.byref(got), ctypes.byref(wrote)))
            if got.value == 0:
                break
            lines += got.value
            row += wrote.value
        want = (m - int(row0)) if limit_rows < 0 else int(limit_rows)
        if first_row is not None:
            want = int(m_total)
        if lines != want:
            raise ValueError("%s has %d data lines, %d sites were expected" % (path, lines, want))
        stats = np.zeros(8, dtype=np.float64)
        check(lib.wgs_depth_ingest_stats(g, stats.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return dict(zip(("host_peak_bytes", "device_ms", "host_lines", "text_bytes", "lines", "chunks", "members_on_device",
                         "tokenise_ms"), stats.tolist()))
    except ValueError as e:
        if str(path) not in str(e):
            raise ValueError("%s: %s" % (path, e)) from None
        raise
    finally:
        if g:
            lib.wgs_depth_ingest_destroy(g)
        lib.wgs_reader_close(r)


def key_filter(keys, counts, n_threshold, single_read_threshold):
    """zscore.AD_summary, lines 22-39: rows (Ar, Aa, depth, sites) of the classes that survive, in order of first appearance."""
    S = np.column_stack((keys[:, 0], keys[:, 1], keys[:, 0] + keys[:, 1], counts)).astype(np.int32)
    if single_read_threshold:
        AD_filtered = S[S[:, 2] == 1]
    else:
        AD_filtered = S[(S[:, 3] > n_threshold) & (S[:, 2] != 0)]
    assert (AD_filtered.shape[0] != 0), "No loci were kept! Too stringent filtering?"
    assert (AD_filtered.shape[0] != 1), "Not enough loci were kept! Too stringent filtering?"
    dl, dl_counts = np.unique(AD_filtered[:, 2], return_counts=True)
    return AD_filtered[np.isin(AD_filtered[:, 2], dl[dl < dl_counts])]


def get_factorials(AD_array, keys, means, e=E):
    """zscore.get_factorials (zscore.py:63-80): AD_factorial, AD_like, AD_index.  (keys, means: the dictionary.)"""
    where = {(int(a), int(b)): j for j, (a, b) in enumerate(keys)}
    AD_factorial = np.zeros((AD_array.shape[0], 3), dtype=np.float32)
    AD_like = np.zeros((AD_array.shape[0], 3), dtype=np.float32)
    AD_index = np.zeros((np.max(AD_array[:, 0]) + 1, np.max(AD_array[:, 1]) + 1), dtype=np.int32)
    for i in range(AD_array.shape[0]):
        Ar, Aa = int(AD_array[i, 0]), int(AD_array[i, 1])
        AD_index[Ar, Aa] = i
        ad_factorial = math.comb(Ar + Aa, Aa) / 1
        AD_factorial[i, :] = [ad_factorial * ((1.0 - e) ** Ar) * (e ** Aa), ad_factorial * ((0.5) ** (Ar + Aa)),
                              ad_factorial * ((1.0 - e) ** Aa) * (e ** Ar)]
        AD_like[i] = means[where[(Ar, Aa)]]
    return AD_factorial, AD_like, AD_index


def ind_range(n, ind_start, ind_end):
    """WGSassign.py:336-345 as it stands (--ind_start 0 is refused)."""
    if ind_start is not None:
        assert (ind_start > 0 and ind_start <= n), "Start individual index needs to be within range of number of individuals!"
    if ind_end is not None:
        assert (ind_end > 0 and ind_end <= n), "End individual index needs to be within range of number of individuals!"
    return (0 if ind_start is None else ind_start), (n if ind_end is None else ind_end)


def class_index(Ar, Aa):
    d = Ar + Aa
    return d * (d + 1) // 2 + Aa


# ---------------------------------------------------------------- device objects
class DepthTable(Handle):
    """The allele-depth table of a DeviceBeagle's SNP shard on the device (wgs_depth)."""

    _destroy, _at_exit = "wgs_depth_destroy", False       # (its matrix closes it)

    def __init__(self, beagle, AD=None, chunk_rows=None):
        self.b = beagle
        h = ctypes.c_void_p()
        check(_lib.load().wgs_depth_create(beagle.handle, ctypes.byref(h)))
        self._own(h, beagle)
        if AD is not None:
            check_depths(AD, beagle.m, beagle.n)
            step = chunk_rows or max(1, (64 << 20) // (8 * beagle.n))
            for r in range(0, beagle.m, step):
                self.upload_rows(AD[r:r + step], r)

    @classmethod
    def from_file(cls, beagle, path, counts=False, majmin=None, chunk_bytes=None, first_row=0, m_total=None):
        """A fresh table streamed from `path` on the device: allele depths as --ind_ad_file holds them (text, gzip or BGZF), or with
        counts=True ANGSD's counts with the (m, 2) selectors `majmin` (read_majmin).  Nothing of size m x 2n exists on the host;
        .ingest_stats tells what did.  .npy goes through the upload path.  ValueError (and no table) unless the file has exactly
        beagle.m data lines of at least 2n (4n) integers in 0..255.
        A SNP shard (m_total: the sites of all shards; beagle.m of them from first_row on are this one's): the table takes the
        file's data rows [first_row, first_row + beagle.m), `majmin` holds the selectors of those rows, and the file must have
        m_total data lines; every line before the range is still read, and a token np.loadtxt refuses there is still reported."""
        ranged = m_total is not None or first_row != 0
        m_total = beagle.m if m_total is None else int(m_total)
        if ranged and not (0 <= first_row and first_row + beagle.m <= m_total):
            raise ValueError("rows [%d, %d) of the depth file lie outside its %d sites" % (first_row, first_row + beagle.m, m_total))
        if str(path).endswith(".npy") and not counts:
            AD = read_depths(path)
            if ranged:
                if AD.ndim != 2 or AD.shape[0] != m_total:
                    raise ValueError("allele depths have shape %s, the Beagle file has %d sites" % (AD.shape, m_total))
                AD = AD[first_row:first_row + beagle.m]
            return cls(beagle, AD)
        t = cls(beagle)
        try:
            t.ingest_stats = stream_table(t._h, beagle.m, path, counts, majmin, chunk_bytes, first_row=first_row if ranged else None,
                                          m_total=m_total)
        except Exception:
            t.close()
            raise
        return t

    def upload_rows(self, rows, row0=0):
        rows = np.ascontiguousarray(rows[:, :2 * self.b.n], dtype=np.int32)
        check(_lib.load().wgs_depth_upload_rows(self._h, i32p(rows), int(row0), rows.shape[0]))

    def download_rows(self, row0=0, nrows=None):
        nrows = self.b.m - row0 if nrows is None else nrows
        out = np.empty((nrows, 2 * self.b.n), dtype=np.int32)
        check(_lib.load().wgs_depth_download_rows(self._h, i32p(out), int(row0), int(nrows)))
        return out


class KeepSet(Handle):
    """L_keep of individuals [i0, i0 + count) on the device (wgs_zkeep); .kept[j] = sites kept."""

    _destroy, _at_exit = "wgs_zkeep_destroy", False       # (its table's matrix closes it)

    def __init__(self, depth, i0, key_mean, key_comp, deep_map=None, deep_rows=None):
        count = key_mean.shape[0]
        self.depth, self.i0, self.count = depth, int(i0), count
        key_mean = np.ascontiguousarray(key_mean, dtype=np.float32)
        key_comp = np.ascontiguousarray(key_comp, dtype=np.int32)
        self.kept = np.zeros(count, dtype=np.int64)
        kept_p = self.kept.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        h = ctypes.c_void_p()
        if deep_map is None:
            check(_lib.load().wgs_zkeep_create(depth.handle, self.i0, count, f32p(key_mean), i32p(key_comp), kept_p, ctypes.byref(h)))
        else:                                             # (deep_tables: some individual kept a depth beyond the dense classes)
            deep_map = np.ascontiguousarray(deep_map, dtype=np.int32)
            deep_rows = np.ascontiguousarray(deep_rows, dtype=np.float32)
            assert deep_map.shape == (count, DEEP_MAX + 1) and deep_rows.ndim == 2 and deep_rows.shape[1] == DEEP_ROW
            check(_lib.load().wgs_zkeep_create_deep(depth.handle, self.i0, count, f32p(key_mean), i32p(key_comp), i32p(deep_map),
                                                    f32p(deep_rows), deep_rows.shape[0], kept_p, ctypes.byref(h)))
        self._own(h, depth.b)

    def sites(self, slot):
        out = np.empty(int(self.kept[slot]), dtype=np.int32)
        check(_lib.load().wgs_zkeep_sites(self._h, int(slot), i32p(out)))
        return out

    def stats(self, tables, freq_dev):
        """Per-site W_l_obs, W_l, var_W_l of every individual: three lists of float32 arrays (kept[j],)."""
        tables = np.ascontiguousarray(tables, dtype=np.float32)
        assert tables.shape == (self.count, N_CLASSES, 6)
        ptrs = (ctypes.c_void_p * self.count)(*[int(p) for p in freq_dev])
        total = int(self.kept.sum())
        out = [np.empty(total, dtype=np.float32) for _ in range(3)]
        check(_lib.load().wgs_zscore_stats(self._h, f32p(tables), ptrs, f32p(out[0]), f32p(out[1]), f32p(out[2])))
        cuts = np.cumsum(self.kept)[:-1]
        return [np.split(o, cuts) for o in out]

    def stats_dev(self, tables, freq_dev):
        """stats() that downloads nothing: (device pointer to [3][all] float32 owned by this set, all) -- what ZSum.push takes."""
        tables = np.ascontiguousarray(tables, dtype=np.float32)
        assert tables.shape == (self.count, N_CLASSES, 6)
        ptrs = (ctypes.c_void_p * self.count)(*[int(p) for p in freq_dev])
        dev, total = ctypes.c_void_p(), ctypes.c_int64()
        check(_lib.load().wgs_zscore_stats_dev(self._h, f32p(tables), ptrs, ctypes.byref(dev), ctypes.byref(total)))
        return dev, int(total.value)


# ---------------------------------------------------------------- the reference's functions, a batch of individuals at a time
def deep_classes(site, ad, g):
    """The dictionary entries of one individual's deep sites (site order): keys (nk, 2), counts, first sites, float32 sums (nk, 3)
    of (g0, g1, (1 - g0) - g1) -- the literal serial chain in site order, as the class sweep forms it for the dense tier."""
    code = ad[:, 0].astype(np.int64) * 256 + ad[:, 1]
    uniq, start, counts = np.unique(code, return_index=True, return_counts=True)
    order = np.argsort(code, kind="stable")                  # class by class, site order inside a class
    T = np.stack((g[:, 0], g[:, 1], (np.float32(1) - g[:, 0]) - g[:, 1]), axis=1)[order]
    sums = np.empty((len(uniq), 3), dtype=np.float32)
    for j, (lo, c) in enumerate(zip(np.cumsum(counts) - counts, counts)):
        sums[j] = np.cumsum(T[lo:lo + c], axis=0, dtype=np.float32)[-1]            # one float32 addition per site
    return np.column_stack((uniq // 256, uniq % 256)).astype(np.int64), counts.astype(np.int64), site[start], sums


def merge_tiers(dense, deep):
    """(keys, counts, first, sums) of the two tiers -> the reference's dictionary: keys, counts, means in order of first
    appearance (every site has one class, so the first sites are distinct)."""
    keys, counts, first, sums = (np.concatenate((a, b)) for a, b in zip(dense, deep))
    order = np.argsort(first, kind="stable")
    keys, counts, sums = keys[order], counts[order], sums[order]
    means = (sums.astype(np.float64) / counts[:, None]).astype(np.float32)     # np.mean: float32 sums, true_divide by the count
    return keys, counts, means


def sharded(comm):
    return comm is not None and comm.world > 1


def comm_handle(comm):
    """The wgs_comm of a communicator of several ranks: the class sweep and the masked fit hand their running values from shard to
    shard inside the library (RCCL, or the socket transport attached to it)."""
    h = getattr(comm, "handle", None)
    if h is None:
        raise ValueError("the z-scores over SNP shards need a communicator the library can use (WGSASSIGN_COMM=rccl or socket), not %s"
                         % type(comm).__name__)
    return h


def concat_deep(parts):
    """The deep-site lists of one individual from every shard, in rank order -- which is site order: (sites as GLOBAL numbers, (Ar, Aa),
    (g0, g1)), as deep_classes takes them.  parts: per rank (site, ad, g), whatever each rank's lists were serialised to."""
    site = np.concatenate([np.asarray(p[0], dtype=np.int64).reshape(-1) for p in parts])
    ad = np.concatenate([np.asarray(p[1], dtype=np.int32).reshape(-1, 2) for p in parts])
    g = np.concatenate([np.asarray(p[2], dtype=np.float32).reshape(-1, 2) for p in parts])
    return site, ad, g


def dictionaries(i0, cnt, first, sums, over, listed, n_threshold, single_read_threshold, deep):
    """The tail of AD_summary, the same for one shard and for many: per individual the dense tier's classes (cnt, first, sums as the
    class sweep reports them -- over ALL shards: counts added, first sites the smallest global number, sums after the last shard),
    merged with the dictionary entries of its deep sites (listed[j] = (site, ad, g) in site order; over[j] = how many there are)."""
    maxd = MAX_DENSE
    d_of = np.repeat(np.arange(maxd + 1), np.arange(maxd + 1) + 1)
    a_of = np.arange(N_CLASSES) - d_of * (d_of + 1) // 2
    out = []
    for j in range(cnt.shape[0]):
        if over[j] and not deep and not single_read_threshold:
            raise ValueError("individual %d has %d sites deeper than %d reads: the depth classes of this build end there "
                             "(--single_read_threshold needs depth 1 only and accepts such data)" % (i0 + j, int(over[j]), maxd))
        seen = np.flatnonzero(cnt[j] > 0)
        dense = (np.column_stack((d_of[seen] - a_of[seen], a_of[seen])).astype(np.int64), cnt[j, seen].astype(np.int64), first[j, seen],
                 sums[j, seen])
        if deep and over[j]:
            keys, counts, means = merge_tiers(dense, deep_classes(*listed[j]))
        else:
            keys, counts, means = merge_tiers(dense, (np.empty((0, 2), dtype=np.int64), np.empty(0, dtype=np.int64),
                                                     np.empty(0, dtype=first.dtype), np.empty((0, 3), dtype=np.float32)))
        out.append(dict(keys=keys, counts=counts, means=means, AD_array=key_filter(keys, counts, n_threshold, single_read_threshold)))
    return out


def list_deep_sites(depth, i0, count, over):
    """wgs_zscore_deep_sites: per individual (site, ad, g) of this table's sites deeper than 21 reads, in site order."""
    total = int(over.sum())
    site, ad, g = np.empty(total, dtype=np.int32), np.empty((total, 2), dtype=np.int32), np.empty((total, 2), dtype=np.float32)
    over = np.ascontiguousarray(over, dtype=np.int32)
    check(_lib.load().wgs_zscore_deep_sites(depth.handle, int(i0), int(count), i32p(over), i32p(site), i32p(ad), f32p(g)))
    cuts = np.cumsum(over)[:-1]
    return list(zip(np.split(site, cuts), np.split(ad, cuts), np.split(g, cuts)))


def AD_summary(depth, i0, count, n_threshold, single_read_threshold, deep=False, comm=None):
    """zscore.AD_summary (zscore.py:11-40) for individuals [i0, i0 + count): list of dict(keys, counts, means, AD_array) -- the
    dictionary in order of first appearance and the filtered classes.  One launch (wgs_zscore_classes); with deep=True one more
    group of launches (wgs_zscore_deep_sites) if an individual of the batch has sites deeper than 21 reads, whose classes then
    enter the dictionary like any other.  deep=False: such data is refused, except under single_read_threshold.
    comm with several ranks (collective): the table is a SNP shard; the class sweep goes from shard to shard
    (wgs_zscore_classes_sharded), every rank lists its own deep sites and receives everybody's, and every rank returns the same
    dictionaries, first sites in global numbers."""
    lib = _lib.load()
    cnt = np.empty((count, N_CLASSES), dtype=np.int32)
    sums = np.empty((count, N_CLASSES, 3), dtype=np.float32)
    if sharded(comm):
        first = np.empty((count, N_CLASSES), dtype=np.int64)
        over_by_rank = np.empty((comm.world, count), dtype=np.int32)
        check(lib.wgs_zscore_classes_sharded(depth.handle, int(i0), int(count), comm_handle(comm), i32p(cnt), f32p(sums),
                                             first.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), i32p(over_by_rank)))
        over = over_by_rank.sum(axis=0)
        listed = None
        if deep and over.any():                               # (every rank sees every rank's counts: all of them come here, or none)
            mine = over_by_rank[comm.rank]
            own = list_deep_sites(depth, i0, count, mine) if mine.any() else [(np.empty(0, dtype=np.int32),) * 3] * count
            wire = [[(site.astype(np.int64) + depth.b.site0).tolist(), ad.reshape(-1).tolist(), g.reshape(-1).astype(np.float64).tolist()]
                    for site, ad, g in own]
            everybody = comm.allgather_object(wire)           # [rank][individual]
            listed = [concat_deep([everybody[r][j] for r in range(comm.world)]) for j in range(count)]
        return dictionaries(i0, cnt, first, sums, over, listed, n_threshold, single_read_threshold, deep)
    first = np.empty((count, N_CLASSES), dtype=np.int32)
    over = np.empty(count, dtype=np.int32)
    check(lib.wgs_zscore_classes(depth.handle, int(i0), int(count), i32p(cnt), f32p(sums), i32p(first), i32p(over)))
    listed = list_deep_sites(depth, i0, count, over) if deep and over.any() else None
    return dictionaries(i0, cnt, first, sums, over, listed, n_threshold, single_read_threshold, deep)


def deep_tables(summaries):
    """The deep table of a batch (wgs_zkeep_create_deep): map int32 (count, 511) from depth to the first of its rows, rows float32
    (rows, 8) -- per kept depth d > 21 and a = 0 .. d: component and mean of class (d - a, a), then AD_like and AD_factorial at
    AD_index[a, d - a].  (None, None) when no individual kept a deep depth."""
    dmap = np.full((len(summaries), DEEP_MAX + 1), -1, dtype=np.int32)
    rows = []
    for j, s in enumerate(summaries):
        depths = np.unique(s["AD_array"][:, 2])
        depths = depths[depths > MAX_DENSE]
        if not len(depths):
            continue
        fac, like, index = get_factorials(s["AD_array"], s["keys"], s["means"], E)
        where = {(int(a), int(b)): r for r, (a, b) in enumerate(s["keys"])}
        for d in (int(x) for x in depths):
            dmap[j, d] = len(rows)
            for a in range(d + 1):
                mean = s["means"][where[(d - a, a)]]
                c = int(np.argwhere(mean == np.max(mean))[0][0])
                r = index[a, d - a]
                rows.append(np.concatenate(([np.float32(c), mean[c]], like[r], fac[r])).astype(np.float32))
    if not rows:
        return None, None
    return dmap, np.ascontiguousarray(np.stack(rows), dtype=np.float32)


def mask_tables(summaries):
    """Per individual and dense class what the mask sweep reads: the component at which the class mean is largest (-1: the class
    did not survive the key filter) and that mean."""
    count = len(summaries)
    key_mean = np.zeros((count, N_CLASSES), dtype=np.float32)
    key_comp = np.full((count, N_CLASSES), -1, dtype=np.int32)
    for j, s in enumerate(summaries):
        where = {(int(a), int(b)): r for r, (a, b) in enumerate(s["keys"])}
        for Ar, Aa in s["AD_array"][:, :2]:
            if int(Ar) + int(Aa) > MAX_DENSE:
                continue                                  # (a kept deep depth: deep_tables)
            mean = s["means"][where[(int(Ar), int(Aa))]]
            c = int(np.argwhere(mean == np.max(mean))[0][0])
            key_comp[j, class_index(int(Ar), int(Aa))] = c
            key_mean[j, class_index(int(Ar), int(Aa))] = mean[c]
    return key_mean, key_comp


def get_L_keep(depth, i0, summaries):
    """zscore.get_L_keep (zscore.py:43-61) for the batch: a KeepSet (the sites stay on the device)."""
    return KeepSet(depth, i0, *mask_tables(summaries), *deep_tables(summaries))


def stat_tables(summaries):
    """Per individual the rows the kernel reads: [class d (d + 1) / 2 + a] = AD_like[r], AD_factorial[r] with r = AD_index[a, d - a]
    (zscore_cy.pyx:28 reads the index transposed; only depths whose classes all survived are ever looked up).  The rows of kept
    depths beyond 21 are in the KeepSet's deep table."""
    tabs = np.zeros((len(summaries), N_CLASSES, 6), dtype=np.float32)
    parts = []
    for j, s in enumerate(summaries):
        fac, like, index = get_factorials(s["AD_array"], s["keys"], s["means"], E)
        parts.append((fac, like, index))
        for d in np.unique(s["AD_array"][:, 2]):
            if d > MAX_DENSE:
                continue
            for a in range(int(d) + 1):
                r = index[a, int(d) - a]
                tabs[j, class_index(int(d) - a, a)] = np.concatenate((like[r], fac[r]))
    return tabs, parts


def _finish(i, kept, wobs, wl, var, say):
    return _finish_sums(i, kept, np.sum(wobs, dtype=np.float32), np.sum(wl), np.sum(var), say)


def _finish_sums(i, kept, W_l_obs, z_mu, z_var, say):
    """z and the printed lines of an individual from its three float32 sums."""
    with np.errstate(divide="ignore", invalid="ignore"):
        z_tmp = (W_l_obs - z_mu) / np.sqrt(z_var)
    say("Finished individual " + str(i))
    say("z_mu: " + str(z_mu))
    say("z_var: " + str(z_var))
    say("z_obs: " + str(W_l_obs))
    say("Loci used: " + str(int(kept)))
    say("Z-score: " + str(z_tmp))
    return dict(W_l_obs=W_l_obs, z_mu=z_mu, z_var=z_var, z=z_tmp)


def _batches(lo, hi, batch):
    for i0 in range(lo, hi, batch):
        yield i0, min(batch, hi - i0)


class _ShardGather:
    """What crosses the ranks behind a batch's mask and statistic sweeps (collective).  kept[r][j]: sites rank r kept of individual
    j, from one tagged all-reduce; rows(...): rank 0 receives every rank's compacted arrays and cuts them per individual, rank order
    -- site order -- inside each; the other ranks get None."""

    def __init__(self, comm, keep, i0):
        self.comm, self.count = comm, keep.count
        mine = np.zeros((comm.world, keep.count))
        mine[comm.rank] = keep.kept
        self.kept = np.asarray(comm.allreduce_sum(mine, tag=(0, int(i0), keep.count, 0))).reshape(comm.world, keep.count).astype(np.int64)
        self.total = self.kept.sum(axis=0)

    def rows(self, per_individual):
        """per_individual: list (count) of this rank's arrays (kept[rank][j], columns...) -> on rank 0 the list of the whole arrays."""
        flat = np.concatenate(per_individual) if len(per_individual) else np.empty(0)
        got = self.comm.gather_rows(np.ascontiguousarray(flat))
        if got is None:
            return None
        starts = np.concatenate(([0], np.cumsum(self.kept.sum(axis=1))))      # where each rank's rows begin
        inside = np.cumsum(self.kept, axis=1) - self.kept                      # ... and each individual's inside them
        return [np.concatenate([got[starts[r] + inside[r, j]:starts[r] + inside[r, j] + self.kept[r, j]] for r in range(self.comm.world)])
                for j in range(self.count)]


def _finish_batch(comm, g, keep, i0, summ, parts, wobs, wl, var, say, z_out, ind_start, details, extra=None):
    """The three sums, z and the printed lines of a batch -- on rank 0 over the arrays of all shards (several ranks), which also
    fills z_out and `details` there.  extra(j, sites) -> more entries of an individual's `details` from this rank's shard, per-site
    arrays among them (these are gathered like the statistics).  g: the batch's _ShardGather (None: one shard)."""
    count = keep.count
    if not sharded(comm):
        for j in range(count):
            r = _finish(i0 + j, keep.kept[j], wobs[j], wl[j], var[j], say)
            z_out[i0 + j - ind_start, 0] = r["z"]
            if details is not None:
                sites = keep.sites(j)
                details.append(dict(summ[j], keep=sites, fac=parts[j][0], like=parts[j][1], index=parts[j][2], wobs=wobs[j], wl=wl[j],
                                    var=var[j], **(extra(j, sites) if extra else {}), **r))
        return
    stats = g.rows([np.stack((wobs[j], wl[j], var[j]), axis=1) for j in range(count)])
    more = None
    if details is not None:                                   # (every rank was asked for them, or none)
        local = [keep.sites(j) for j in range(count)]
        ext = [extra(j, local[j]) if extra else {} for j in range(count)]
        per_site = sorted(k for k, v in ext[0].items() if isinstance(v, np.ndarray))
        sites = g.rows([local[j].astype(np.int64) + keep.depth.b.site0 for j in range(count)])
        more = {k: g.rows([ext[j][k] for j in range(count)]) for k in per_site}
    if comm.rank != 0:
        return
    for j in range(count):
        w, l, v = (np.ascontiguousarray(stats[j][:, c]) for c in range(3))
        r = _finish(i0 + j, g.total[j], w, l, v, say)
        z_out[i0 + j - ind_start, 0] = r["z"]
        if details is not None:
            d = dict(summ[j], keep=sites[j], fac=parts[j][0], like=parts[j][1], index=parts[j][2], wobs=w, wl=l, var=v, **r)
            d.update({k: x for k, x in ext[j].items() if k not in per_site})
            d.update({k: more[k][j] for k in per_site})
            details.append(d)


def assignment_z_scores(beagle, depth, IDs, pops, afset, n_threshold=0, single_read_threshold=False, ind_start=0, ind_end=None,
                        batch=64, say=print, details=None, deep=True, comm=None):
    """--get_assignment_z_score (WGSassign.py:395-446): z of individuals [ind_start, ind_end) against column k of `afset`, k = the
    position of the individual's population in `pops`.  float32 (n_sub, 1).  details (a list) receives per individual the
    intermediate arrays (tests).  deep: as for AD_summary -- sites deeper than 21 reads are computed with, as the reference does.
    comm with several ranks (collective): beagle, depth and afset hold this rank's SNP shard.  Rank 0 prints (`say`), fills
    `details` -- kept sites in global numbers, the per-site arrays of all shards -- and returns the z-scores; the other ranks return
    None."""
    ind_end = beagle.n if ind_end is None else ind_end
    z_out = np.empty((ind_end - ind_start, 1), dtype=np.float32)
    for i0, count in _batches(ind_start, ind_end, batch):
        summ = AD_summary(depth, i0, count, n_threshold, single_read_threshold, deep, comm)
        keep = get_L_keep(depth, i0, summ)
        g = _ShardGather(comm, keep, i0) if sharded(comm) else None
        tabs, parts = stat_tables(summ)
        cols = [int(np.argwhere(pops == IDs[i0 + j, 1])[0][0]) for j in range(count)]
        wobs, wl, var = keep.stats(tabs, [afset.col_dev(k) for k in cols])
        _finish_batch(comm, g, keep, i0, summ, parts, wobs, wl, var, say, z_out, ind_start, details)
        keep.close()
    return z_out if not sharded(comm) or comm.rank == 0 else None


def reference_z_scores(beagle, depth, IDs, group_of, maf_iter=200, maf_tole=1e-4, n_threshold=0, single_read_threshold=False,
                       ind_start=0, ind_end=None, batch=64, say=print, details=None, deep=True, comm=None):
    """--get_reference_z_score (WGSassign.py:311-393): per individual the leave-one-out EM fit of its population on ITS kept sites
    (wgs_em_fit_masked: the existing sweeps, the convergence chain over the kept sites), the clamp, then as above.  `beagle` must
    hold one slab per population (group_of as --get_reference_af builds it).
    comm with several ranks (collective): one EM batch per rank over its shard, the chain crossing the ranks
    (wgs_em_fit_masked_sharded); every rank reports the fits' iterations through `say`; otherwise as assignment_z_scores."""
    from .device import EMBatch
    ind_end = beagle.n if ind_end is None else ind_end
    sizes = np.bincount(group_of, minlength=int(np.max(group_of)) + 1)
    z_out = np.empty((ind_end - ind_start, 1), dtype=np.float32)
    for i0, count in _batches(ind_start, ind_end, batch):
        summ = AD_summary(depth, i0, count, n_threshold, single_read_threshold, deep, comm)
        keep = get_L_keep(depth, i0, summ)
        g = _ShardGather(comm, keep, i0) if sharded(comm) else None
        tabs, parts = stat_tables(summ)
        ids = np.arange(i0, i0 + count)
        if np.any(sizes[group_of[ids]] < 2):
            raise ValueError("a population with a single individual has nobody left for the leave-one-out fit")
        em = EMBatch(beagle, group_of[ids], ids)
        iters = np.zeros(count, dtype=np.int32)
        slots = np.arange(count, dtype=np.int32)
        if sharded(comm):
            kept_total = np.ascontiguousarray(g.total, dtype=np.int64)
            check(_lib.load().wgs_em_fit_masked_sharded(em.handle, keep.handle, i32p(slots), int(maf_iter), float(maf_tole),
                                                        kept_total.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), comm_handle(comm),
                                                        i32p(iters)))
        else:
            check(_lib.load().wgs_em_fit_masked(em.handle, keep.handle, i32p(slots), int(maf_iter), float(maf_tole), i32p(iters)))
        for j in range(count):
            if iters[j]:
                say("EM (MAF) converged at iteration: " + str(int(iters[j])))
            em.clamp(j, int(sizes[group_of[i0 + j]]) - 1)
        wobs, wl, var = keep.stats(tabs, [em.f_dev(j) for j in range(count)])
        _finish_batch(comm, g, keep, i0, summ, parts, wobs, wl, var, say, z_out, ind_start, details,
                      extra=lambda j, sites: dict(A=em.get_f(j)[sites], it=int(iters[j])))
        em.close()
        keep.close()
    return z_out if not sharded(comm) or comm.rank == 0 else None


# ---------------------------------------------------------------- --get_assignment_z_score in site windows
class ZSum(Handle):
    """What a batch of individuals carries from site window to site window on the device (wgs_zsum): the class sweep's running sums
    and, per (individual, array) of the three per-site arrays, np.sum's float32 order -- the running value over the closed
    8192-element chunks and the open chunk."""

    _destroy, _at_exit = "wgs_zsum_destroy", False        # (its context closes it)

    def __init__(self, count, ctx=None):
        self.ctx = ctx or get_context()
        self.count = int(count)
        self.downloaded = 0                          # bytes that crossed to the host through this object
        h = ctypes.c_void_p()
        check(_lib.load().wgs_zsum_create(self.ctx.handle, self.count, ctypes.byref(h)))
        self._own(h, self.ctx)

    def classes(self, depth, i0):
        """The class sweep over the next window (wgs_zscore_classes_carry): counts, first sites (LOCAL, -1: none) and `over` of this
        window, and the running sums after it."""
        count = self.count
        cnt = np.empty((count, N_CLASSES), dtype=np.int32)
        sums = np.empty((count, N_CLASSES, 3), dtype=np.float32)
        first = np.empty((count, N_CLASSES), dtype=np.int32)
        over = np.empty(count, dtype=np.int32)
        check(_lib.load().wgs_zscore_classes_carry(depth.handle, int(i0), count, self._h, i32p(cnt), f32p(sums), i32p(first), i32p(over)))
        self.downloaded += cnt.nbytes + sums.nbytes + first.nbytes + over.nbytes
        return cnt, sums, first, over

    def push(self, dev, total, kept):
        kept = np.ascontiguousarray(kept, dtype=np.int64)
        check(_lib.load().wgs_zsum_push(self._h, dev, int(total), kept.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))

    def push_host(self, arrays, kept):
        """Test hook (wgs_debug_zsum_push): arrays (3, all) float32 on the host."""
        arrays = np.ascontiguousarray(arrays, dtype=np.float32)
        kept = np.ascontiguousarray(kept, dtype=np.int64)
        assert arrays.ndim == 2 and arrays.shape[0] == 3
        check(_lib.load().wgs_debug_zsum_push(self._h, f32p(arrays), arrays.shape[1], kept.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))

    def totals(self):
        out = np.zeros(self.count, dtype=np.int64)
        check(_lib.load().wgs_zsum_totals(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def state(self):
        """(totals (count,), run (count, 3) float32, tails: [j][a] float32 arrays of totals[j] % 8192 elements) as the device holds them."""
        totals = self.totals()
        fill = totals % 8192
        run = np.zeros((self.count, 3), dtype=np.float32)
        packed = np.zeros(max(1, 3 * int(fill.sum())), dtype=np.float32)
        check(_lib.load().wgs_zsum_finish(self._h, f32p(run), f32p(packed)))
        self.downloaded += run.nbytes + 12 * int(fill.sum())
        tails, at = [], 0
        for j in range(self.count):
            tails.append([packed[at + a * fill[j]:at + (a + 1) * fill[j]] for a in range(3)])
            at += 3 * int(fill[j])
        return totals, run, tails

    def finish(self):
        """(totals, sums (count, 3) float32): np.sum of everything pushed.  The ragged last chunk is closed here as NumPy closes it,
        run + np.sum(tail): exact, because a running value that started at +0.0 is never -0.0; nothing is added for an empty tail."""
        totals, run, tails = self.state()
        sums = np.empty((self.count, 3), dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(self.count):
                for a in range(3):
                    sums[j, a] = run[j, a] + np.sum(tails[j][a]) if tails[j][a].size else run[j, a]
        return totals, sums


class _ShapeTable(Handle):
    """A depth table of its own shape (wgs_depth_create_shape): the landing place of a depth file's chunks."""

    _destroy, _at_exit = "wgs_depth_destroy", False       # (the DepthWindows that made it closes it, else its context)

    def __init__(self, ctx, rows, n):
        h = ctypes.c_void_p()
        check(_lib.load().wgs_depth_create_shape(ctx.handle, int(rows), int(n), ctypes.byref(h)))
        self._own(h, ctx)
        self.ctx, self.rows = ctx, int(rows)


DEPTH_WINDOW_CHUNK = 8 << 20         # text bytes per chunk of a windowed depth pass


class DepthWindows:
    """ONE pass over a depth file whose rows go to consecutive window tables: one reader and one ingest stay open, the file is read
    once, and its chunks land in a small table of their own (at row 0) from which the rows are copied on the device to the window
    that owns them (wgs_depth_copy_rows) -- whichever edge a chunk straddles.  Line numbers in messages are the file's, and the
    number of data lines is compared with m at the end of the pass (finish).  counts=True: ANGSD counts with the (m, 2) selectors
    `majmin`, of which every chunk is handed the rows [lines so far, ...).  A .npy file (pairs) is read through np.load(mmap_mode="r")
    rows.  .stats after finish: wgs_depth_ingest_stats of the pass (text files)."""

    def __init__(self, path, m, n, ctx, counts=False, majmin=None, chunk_bytes=None, threads=None):
        from .reader_cy import host_threads
        self.path, self.m, self.n, self.ctx, self.counts = str(path), int(m), int(n), ctx, bool(counts)
        self.lines, self.lo, self.pending = 0, 0, 0      # data lines read; rows [lo, lo + pending) of the staging table wait for a window
        self.stats, self._r, self._g, self._stage, self._npy = None, ctypes.c_void_p(), ctypes.c_void_p(), None, None
        if self.path.endswith(".npy") and not counts:
            AD = np.load(self.path, mmap_mode="r")
            if AD.ndim != 2 or AD.shape[0] != self.m or AD.shape[1] < 2 * self.n:
                raise ValueError("allele depths have shape %s, the Beagle file has %d sites and %d individuals" % (AD.shape, self.m, self.n))
            self._npy = AD
            return
        lib = _lib.load()
        tpi = 4 if counts else 2
        chunk = int(chunk_bytes or DEPTH_WINDOW_CHUNK)
        # a data line holds at least tpi * n tokens of one character and a separator each: a bound on the lines of one chunk, with
        # room for the carried partial line and a BGZF member beyond the chunk's size.  (A chunk that still held more lines would be
        # refused below, not truncated.)
        self.stage_rows = max(1024, 2 * (max(chunk, 65536) + (1 << 17)) // (2 * tpi * self.n) + 1024)
        if counts:
            self.majmin = np.ascontiguousarray(majmin, dtype=np.uint8)
            if self.majmin.shape != (self.m, 2):
                raise ValueError("the allele selectors have shape %s, the table %d sites" % (self.majmin.shape, self.m))
        try:
            check(lib.wgs_reader_open_table(os.fsencode(self.path), int(threads or host_threads()), 1 if counts else 0, ctypes.byref(self._r)))
            self._stage = _ShapeTable(ctx, self.stage_rows, self.n)
            sel = self._selectors() if counts else None
            check(lib.wgs_depth_ingest_create(self._stage.handle, self._r, 1 if counts else 0, sel.ctypes.data if counts else None, -1, chunk,
                                              ctypes.byref(self._g)))
        except ValueError as e:
            self.close()
            raise self._named(e) from None
        except Exception:
            self.close()
            raise

    def _named(self, e):
        return e if self.path in str(e) else ValueError("%s: %s" % (self.path, e))

    def _selectors(self):
        """The selectors of the staging table's rows for the next chunk: the file's rows [lines, lines + stage_rows)."""
        sel = np.zeros((self.stage_rows, 2), dtype=np.uint8)
        rows = self.majmin[self.lines:self.lines + self.stage_rows]
        sel[:len(rows)] = rows
        return sel

    def _next_chunk(self):
        lib = _lib.load()
        got, wrote = ctypes.c_int64(), ctypes.c_int64()
        try:
            if self.counts and self.lines:
                sel = self._selectors()
                check(lib.wgs_depth_ingest_set_selectors(self._g, sel.ctypes.data, self.stage_rows))
            check(lib.wgs_depth_ingest_next(self._g, 0, ctypes.byref(got), ctypes.byref(wrote)))
        except ValueError as e:
            raise self._named(e) from None
        if got.value and wrote.value != got.value:
            raise RuntimeError("%s: a chunk of %d data lines does not fit the %d rows it is staged in" % (self.path, got.value, self.stage_rows))
        self.lines += got.value
        self.lo, self.pending = 0, got.value
        return got.value

    def fill(self, table, rows):
        """The file's next `rows` data rows into rows [0, rows) of the DepthTable `table`."""
        rows, at = int(rows), 0
        if self._npy is not None:
            step = max(1, (64 << 20) // (8 * self.n))
            for r in range(0, rows, step):
                table.upload_rows(np.asarray(self._npy[self.lines + r:self.lines + min(rows, r + step)]), r)
            self.lines += rows
            return
        while at < rows:
            if not self.pending and not self._next_chunk():
                raise ValueError("%s has %d data lines, %d sites were expected" % (self.path, self.lines, self.m))
            take = min(self.pending, rows - at)
            check(_lib.load().wgs_depth_copy_rows(table.handle, at, self._stage.handle, self.lo, take))
            at, self.lo, self.pending = at + take, self.lo + take, self.pending - take

    def finish(self):
        """The end of the pass: whatever the file still holds is read and counted, and the total must be m."""
        if self._npy is None:
            while self._next_chunk():
                pass
            if self.lines != self.m:
                raise ValueError("%s has %d data lines, %d sites were expected" % (self.path, self.lines, self.m))
            stats = np.zeros(8, dtype=np.float64)
            check(_lib.load().wgs_depth_ingest_stats(self._g, stats.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
            self.stats = dict(zip(("host_peak_bytes", "device_ms", "host_lines", "text_bytes", "lines", "chunks", "members_on_device",
                                   "tokenise_ms"), stats.tolist()))
        self.close()
        return self.stats

    def close(self):
        lib = _lib.load()
        if self._g:
            lib.wgs_depth_ingest_destroy(self._g)
            self._g = ctypes.c_void_p()
        if self._r:
            lib.wgs_reader_close(self._r)
            self._r = ctypes.c_void_p()
        if self._stage is not None:
            self._stage.close()
            self._stage = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge_windows(cnt_tot, first_glob, over_tot, site0, cnt, first, over):
    """One more window into the class sweep's host totals: counts and `over` add (int64), a first site is the smallest GLOBAL number
    site0 + local among the windows that have the class (-1: none yet).  Windows come in site order, so the first one to have a class
    sets it."""
    cnt_tot += cnt
    over_tot += over
    new = (first_glob < 0) & (first >= 0)
    first_glob[new] = int(site0) + first[new].astype(np.int64)


def window_pass(path, depth_path, m, n, W, ctx, info, body, counts=False, majmin=None, depth_chunk_bytes=None, group_of=None, n_groups=1):
    """ONE pass over a Beagle file and its depth file in windows of W sites: body(b, depth) for every window, the window's depth rows
    in place (DepthWindows); what was made from the window is closed before the next one is asked for.  group_of / n_groups: the
    windows carry one slab per population.  Returns the depth ingest's statistics."""
    from . import reader_cy
    dw = DepthWindows(depth_path, m, n, ctx, counts, majmin, depth_chunk_bytes)
    gen = reader_cy.stream_windows(path, W, ctx=ctx, info=info, group_of=group_of, n_groups=n_groups)
    try:
        for b in gen:
            depth = DepthTable(b)
            try:
                dw.fill(depth, b.m)
                body(b, depth)
            finally:
                depth.close()
        return dw.finish()
    finally:
        gen.close()
        dw.close()


def class_pass(zs, i0, count, deep, one_pass):
    """Pass A of the windowed z-scores: the class sweep with its running sums carried from window to window (ZSum.classes), counts,
    `over` and first sites put together as global numbers, the deep sites of every window listed.  one_pass(body) runs a pass.
    Returns (cnt_tot, first_glob, sums after the last window, over_tot, listed -- as `dictionaries` takes them -- and the depth
    ingest's statistics)."""
    cnt_tot = np.zeros((count, N_CLASSES), dtype=np.int64)
    first_glob = np.full((count, N_CLASSES), -1, dtype=np.int64)
    over_tot = np.zeros(count, dtype=np.int64)
    last = {}
    parts = [[] for _ in range(count)]

    def pass_a(b, depth):
        cnt, sums, first, over = zs.classes(depth, i0)
        merge_windows(cnt_tot, first_glob, over_tot, b.site0, cnt, first, over)
        last["sums"] = sums
        if deep and over.any():
            for j, (site, ad, g) in enumerate(list_deep_sites(depth, i0, count, over)):
                if len(site):
                    parts[j].append((site.astype(np.int64) + b.site0, ad, g))
                    zs.downloaded += site.nbytes + ad.nbytes + g.nbytes

    depth_stats = one_pass(pass_a)
    empty = (np.empty(0, dtype=np.int64), np.empty((0, 2), dtype=np.int32), np.empty((0, 2), dtype=np.float32))
    listed = [concat_deep(p) if p else empty for p in parts] if deep and over_tot.any() else None
    return cnt_tot, first_glob, last["sums"], over_tot, listed, depth_stats


def assignment_z_scores_windowed(path, depth_path, A, IDs, pops, n_threshold=0, single_read_threshold=False, ind_start=0, ind_end=None,
                                 window_sites=None, say=print, details=None, deep=True, counts=False, majmin=None, batch=None, ctx=None,
                                 depth_chunk_bytes=None):
    """assignment_z_scores for a Beagle FILE and a depth FILE whose matrix and depth table need not fit the device: two passes over
    both files in consecutive windows of `window_sites` sites (a multiple of 8192, rounded down; None: WGSASSIGN_Z_WINDOW_SITES, else
    what windows.plan_z derives -- one window when everything fits), all individuals of [ind_start, ind_end) together (or in rounds
    of `batch` individuals, each with its two passes, when windows.plan_z says their state does not fit beside a window).
      Pass A: the class sweep with its running sums carried from window to window (ZSum.classes); counts, `over` and first sites are
              put together here as global numbers; windows with sites deeper than 21 reads list them (wgs_zscore_deep_sites).
      Then the dictionaries, the key filter and the tables, once, as the resident path forms them.
      Pass B: per window the mask, the statistic sweep into device arrays and the push into np.sum's order (ZSum.push); the
              frequency columns are rows [site0, site0 + m_w) of A (an array or an np.load(..., mmap_mode="r") view).
    z, every printed line and the assertions of the key filter are those of the resident run, bit for bit.  details (a list) receives
    per individual the dictionary, the tables, kept (sites kept) and the sums -- no per-site array.  Host memory does not grow with m.
    .stats: windows, window_sites, rounds, seconds_a / seconds_b and depth_a / depth_b (the depth ingest's statistics) per round,
    downloaded_bytes; .info: n, m, sample_names, site_names (first and last four)."""
    import time

    from . import reader_cy, windows
    from .device import AFSet, get_context
    ctx = ctx or get_context()
    index, _, m = reader_cy.ensure_index(path)
    if m <= 0:
        raise ValueError("%s holds no sites" % path)
    if A.ndim != 2 or A.shape[0] != m:
        raise ValueError("the allele frequency file has %d sites, the Beagle file %d" % (A.shape[0], m))
    with reader_cy.BeagleStream(path, threads=1) as st:
        n = st.n
    ind_end = n if ind_end is None else ind_end
    total = ind_end - ind_start
    if window_sites is None:
        planned = windows.plan_z(m, n, A.shape[1], total, ctx.mem_info()[0])
        W, batch = planned if planned is not None else (windows.whole_file_window(m), batch)
    else:
        W = windows.explicit_window(window_sites)
    batch = windows.z_batch(W, n, A.shape[1], total, ctx.mem_info()[0]) if not batch else min(int(batch), total)
    rounds = list(_batches(ind_start, ind_end, batch))
    if len(rounds) > 1:
        say("wgsassign_amd: the z-scores of %d individuals run in %d rounds of at most %d" % (total, len(rounds), batch))
    z_out = np.empty((total, 1), dtype=np.float32)
    info = {}
    stats = dict(windows=0, window_sites=W, rounds=len(rounds), seconds_a=[], seconds_b=[], depth_a=[], depth_b=[], downloaded_bytes=0)

    def one_pass(body):
        return window_pass(path, depth_path, m, n, W, ctx, info, body, counts, majmin, depth_chunk_bytes)

    for i0, count in rounds:
        zs = ZSum(count, ctx)
        try:
            t0 = time.perf_counter()
            cnt_tot, first_glob, class_sums, over_tot, listed, depth_a = class_pass(zs, i0, count, deep, one_pass)
            stats["depth_a"].append(depth_a)
            stats["seconds_a"].append(time.perf_counter() - t0)
            summ = dictionaries(i0, cnt_tot, first_glob, class_sums, over_tot, listed, n_threshold, single_read_threshold, deep)
            key_mean, key_comp = mask_tables(summ)
            dmap, drows = deep_tables(summ)
            tabs, tparts = stat_tables(summ)
            cols = [int(np.argwhere(pops == IDs[i0 + j, 1])[0][0]) for j in range(count)]
            kept_tot = np.zeros(count, dtype=np.int64)

            def pass_b(b, depth):
                keep = KeepSet(depth, i0, key_mean, key_comp, dmap, drows)
                afs = AFSet.from_host(np.ascontiguousarray(A[b.site0:b.site0 + b.m], dtype=np.float32), ctx=ctx)
                try:
                    dev, all_kept = keep.stats_dev(tabs, [afs.col_dev(k) for k in cols])
                    zs.push(dev, all_kept, keep.kept)
                    kept_tot[:] += keep.kept
                finally:
                    afs.close()
                    keep.close()

            t0 = time.perf_counter()
            stats["depth_b"].append(one_pass(pass_b))
            stats["seconds_b"].append(time.perf_counter() - t0)
            totals, sums3 = zs.finish()
            assert np.array_equal(totals, kept_tot)
            for j in range(count):
                r = _finish_sums(i0 + j, kept_tot[j], sums3[j, 0], sums3[j, 1], sums3[j, 2], say)
                z_out[i0 + j - ind_start, 0] = r["z"]
                if details is not None:
                    details.append(dict(summ[j], fac=tparts[j][0], like=tparts[j][1], index=tparts[j][2], kept=int(kept_tot[j]), **r))
            stats["downloaded_bytes"] += zs.downloaded
        finally:
            zs.close()
    stats["windows"] = info.get("windows", 0)
    assignment_z_scores_windowed.stats = stats
    assignment_z_scores_windowed.info = dict({k: info.get(k) for k in ("m", "sample_names", "site_names")}, n=n)
    return z_out


# ---------------------------------------------------------------- --get_reference_z_score in site windows
ZREF_FIRST_HORIZON = 32         # iterations the first fit round runs every masked fit for (not measured: DESIGN.md section 5.1)
ENV_ZREF_HORIZON = "WGSASSIGN_ZREF_HORIZON"
RESIDENT_BLOCK = 64             # individuals per batch of the resident run, whose printed lines come block by block


def zref_first_horizon(first_horizon=None, environ=None):
    """The first horizon of the masked fits: the keyword, else WGSASSIGN_ZREF_HORIZON, else ZREF_FIRST_HORIZON; at least 1."""
    if first_horizon is None:
        value = (os.environ if environ is None else environ).get(ENV_ZREF_HORIZON)
        if value is not None and str(value).strip():
            try:
                first_horizon = int(str(value).strip())
            except ValueError:
                raise ValueError("%s must be a number of iterations (an integer >= 1), got %r" % (ENV_ZREF_HORIZON, value))
        else:
            first_horizon = ZREF_FIRST_HORIZON
    if int(first_horizon) < 1:
        raise ValueError("the first horizon of the masked fits is at least 1 iteration, not %d" % int(first_horizon))
    return int(first_horizon)


def resident_order(ind_start, ind_end, converged, six, block=RESIDENT_BLOCK):
    """The lines of the resident reference run in its order: per block of 64 individuals from ind_start first the lines
    `EM (MAF) converged at iteration: t` of the block's fits (converged[i]: the line or None), then each individual's six lines
    (six[i]).  Both are indexed by i - ind_start."""
    out = []
    for i0, count in _batches(ind_start, ind_end, block):
        out.extend(converged[i - ind_start] for i in range(i0, i0 + count) if converged[i - ind_start] is not None)
        for i in range(i0, i0 + count):
            out.extend(six[i - ind_start])
    return out


class _MaskedRounds:
    """windowed_fit.fit_masked's backend for one round of individuals [i0, i0 + count): a round is one pass over both files; every
    window gets its KeepSet and goes through the EMBatch of its matrix (count fits, made once per matrix and pass and kept while the
    matrix moves: the KeepSet and the DepthTable are closed before it does) into one device.EMStream.  The final round leaves every
    fit clamped in its batch, sweeps the statistic against it and pushes the arrays into the ZSum."""

    def __init__(self, one_pass, stream, zs, i0, count, ind_start, group_of, sizes, tables, stats):
        self.one_pass, self.stream, self.zs, self.i0, self.count, self.ind_start = one_pass, stream, zs, int(i0), int(count), int(ind_start)
        self.ids = np.arange(self.i0, self.i0 + self.count, dtype=np.int32)
        self.groups = np.ascontiguousarray(group_of[self.ids], dtype=np.int32)
        lo = 1 / (2 * (np.asarray(sizes, dtype=np.float64)[self.groups] - 1 + 1))      # EMBatch.clamp(j, size - 1)
        self.lo, self.hi = lo.astype(np.float32), (1 - lo).astype(np.float32)
        self.key_mean, self.key_comp, self.dmap, self.drows, self.tabs = tables
        self.slots = np.arange(self.count, dtype=np.int32)
        self.stats = stats
        self.kept_total = None
        self.carry_bytes = 0

    def run_round(self, plan):
        import time

        from .device import EMBatch
        kept = np.zeros(self.count, dtype=np.int64)
        batches = {}

        def body(b, depth):
            em = batches.get(id(b))
            if em is None:
                em = batches[id(b)] = EMBatch(b, self.groups, self.ids)
                b.window_em = em
            keep = KeepSet(depth, self.i0, self.key_mean, self.key_comp, self.dmap, self.drows)
            try:
                self.stream.push_masked(em, keep, self.slots, plan.run_iters, np.ones(self.count, dtype=np.int32) if plan.final else None,
                                        self.lo, self.hi, plan.chains)
                kept[:] += keep.kept
                if plan.final:
                    dev, all_kept = keep.stats_dev(self.tabs, [em.f_dev(j) for j in range(self.count)])
                    self.zs.push(dev, all_kept, keep.kept)
            finally:
                keep.close()

        t0 = time.perf_counter()
        try:
            depth_stats = self.one_pass(body)
        finally:
            for em in batches.values():
                em.close()
        C = self.stream.read_carries()
        self.carry_bytes += C.nbytes
        self.stats["seconds_final" if plan.final else "seconds_fit"][-1].append(time.perf_counter() - t0)
        self.stats["depth_final" if plan.final else "depth_fit"][-1].append(depth_stats)
        if self.kept_total is None:
            for j in range(self.count):             # (what wgs_em_fit_masked says of the resident run's fit of this individual)
                if kept[j] == 0:
                    raise ValueError("fit %d: no site was kept" % ((self.i0 + j - self.ind_start) % RESIDENT_BLOCK))
            self.kept_total = kept
        elif not np.array_equal(kept, self.kept_total):
            raise RuntimeError("the files changed between two passes: the kept sites differ")
        return C, self.kept_total


def reference_z_scores_windowed(path, depth_path, IDs, group_of, maf_iter=200, maf_tole=1e-4, n_threshold=0, single_read_threshold=False,
                                ind_start=0, ind_end=None, window_sites=None, say=print, details=None, deep=True, counts=False,
                                majmin=None, batch=None, ctx=None, depth_chunk_bytes=None, first_horizon=None):
    """reference_z_scores for a Beagle FILE and a depth FILE whose matrix and depth table need not fit the device, on one rank: passes
    over both files in consecutive windows of `window_sites` sites (a multiple of 8192, rounded down; None:
    WGSASSIGN_ZREF_WINDOW_SITES, else what windows.plan_zref derives -- one window when everything fits), one slab per population
    (group_of as --get_reference_af builds it), all individuals of [ind_start, ind_end) together (or in rounds of `batch`
    individuals, each with its own passes, when windows.plan_zref says their state does not fit beside a window).
      Pass A       exactly that of assignment_z_scores_windowed (class_pass); then the dictionaries, the key filter and the tables, once.
      Fit rounds   per window the KeepSet and one EMStream.push_masked: every undecided fit runs from 0.25 to its horizon and the
                   exact float32 chain of EVERY iteration not yet decided goes on over the individual's kept sites of the window, its
                   carry staying on the device; after the last window one read of the carries decides with the resident rule
                   (windowed_fit.ChainScheme: device.chain_diff against the kept sites of all windows).  A fit undecided at its
                   horizon gets another round with the horizon doubled.  first_horizon: the first one (None: WGSASSIGN_ZREF_HORIZON,
                   else ZREF_FIRST_HORIZON); correctness does not depend on it, the number of passes does.
      Final round  per window every fit run to its stop and clamped with n_pop - 1 in its batch, the statistic sweep against it into
                   device arrays and the push into np.sum's order (ZSum.push).
    z, every printed line -- in the resident run's order: blocks of 64 individuals from ind_start, whatever the rounds here were --
    the iteration counts and the assertions of the key filter are those of the resident run, bit for bit.  A population with a
    single individual raises the resident path's ValueError before the first pass; an individual that kept no site in any window
    raises wgs_em_fit_masked's message after the first fit round.  details (a list) receives per individual the dictionary, the
    tables, kept (sites kept), it (the iteration count) and the sums -- no per-site array.  Host memory does not grow with m.
    .stats: windows, window_sites, rounds, fit_rounds and horizons per round of individuals, first_horizon, passes, seconds_a /
    seconds_fit / seconds_final and depth_a / depth_fit / depth_final (the depth ingest's statistics) per pass, downloaded_bytes;
    .info: n, m, sample_names, site_names (first and last four)."""
    import time

    from . import reader_cy, windowed_fit, windows
    from .device import EMStream, get_context
    ctx = ctx or get_context()
    index, _, m = reader_cy.ensure_index(path)
    if m <= 0:
        raise ValueError("%s holds no sites" % path)
    with reader_cy.BeagleStream(path, threads=1) as st:
        n = st.n
    group_of = np.ascontiguousarray(group_of, dtype=np.int32)
    if group_of.shape != (n,):
        raise ValueError("group_of must have one entry for each of the %d individuals of %s" % (n, path))
    n_groups = int(np.max(group_of)) + 1
    sizes = np.bincount(group_of, minlength=n_groups)
    ind_end = n if ind_end is None else ind_end
    total = ind_end - ind_start
    if np.any(sizes[group_of[ind_start:ind_end]] < 2):
        raise ValueError("a population with a single individual has nobody left for the leave-one-out fit")
    horizon = zref_first_horizon(first_horizon)
    free = ctx.mem_info()[0]
    if window_sites is None:
        planned = windows.plan_zref(m, n, n_groups, total, free, maf_iter, counts=sizes)
        W, batch = planned if planned is not None else (windows.whole_file_window(m), batch)
    else:
        W = windows.explicit_window(window_sites)
    batch = windows.zref_batch(W, n, n_groups, total, free, maf_iter, sizes) if not batch else min(int(batch), total)
    rounds = list(_batches(ind_start, ind_end, batch))
    if len(rounds) > 1:
        say("wgsassign_amd: the z-scores of %d individuals run in %d rounds of at most %d" % (total, len(rounds), batch))
    z_out = np.empty((total, 1), dtype=np.float32)
    info = {}
    stats = dict(windows=0, window_sites=W, rounds=len(rounds), fit_rounds=[], horizons=[], first_horizon=horizon, passes=0, seconds_a=[],
                 seconds_fit=[], seconds_final=[], depth_a=[], depth_fit=[], depth_final=[], downloaded_bytes=0)
    converged, six = [None] * total, [None] * total

    def one_pass(body):
        stats["passes"] += 1
        return window_pass(path, depth_path, m, n, W, ctx, info, body, counts, majmin, depth_chunk_bytes, group_of, n_groups)

    for i0, count in rounds:
        zs = ZSum(count, ctx)
        stream = None
        try:
            t0 = time.perf_counter()
            cnt_tot, first_glob, class_sums, over_tot, listed, depth_a = class_pass(zs, i0, count, deep, one_pass)
            stats["depth_a"].append(depth_a)
            stats["seconds_a"].append(time.perf_counter() - t0)
            summ = dictionaries(i0, cnt_tot, first_glob, class_sums, over_tot, listed, n_threshold, single_read_threshold, deep)
            key_mean, key_comp = mask_tables(summ)
            dmap, drows = deep_tables(summ)
            tabs, tparts = stat_tables(summ)
            for key in ("seconds_fit", "seconds_final", "depth_fit", "depth_final"):
                stats[key].append([])
            stream = EMStream(count, maf_iter, m, ctx)
            backend = _MaskedRounds(one_pass, stream, zs, i0, count, ind_start, group_of, sizes, (key_mean, key_comp, dmap, drows, tabs), stats)
            iters, scheme = windowed_fit.fit_masked(backend, count, maf_iter, maf_tole, horizon)
            stats["fit_rounds"].append(scheme.fit_rounds)
            stats["horizons"].append(list(scheme.horizons))
            totals, sums3 = zs.finish()
            assert np.array_equal(totals, backend.kept_total)
            for j in range(count):
                lines = []
                r = _finish_sums(i0 + j, totals[j], sums3[j, 0], sums3[j, 1], sums3[j, 2], lines.append)
                six[i0 + j - ind_start] = lines
                if iters[j]:
                    converged[i0 + j - ind_start] = "EM (MAF) converged at iteration: " + str(int(iters[j]))
                z_out[i0 + j - ind_start, 0] = r["z"]
                if details is not None:
                    details.append(dict(summ[j], fac=tparts[j][0], like=tparts[j][1], index=tparts[j][2], kept=int(totals[j]),
                                        it=int(iters[j]), **r))
            stats["downloaded_bytes"] += zs.downloaded + backend.carry_bytes
        finally:
            if stream is not None:
                stream.close()
            zs.close()
    for line in resident_order(ind_start, ind_end, converged, six):
        say(line)
    stats["windows"] = info.get("windows", 0)
    reference_z_scores_windowed.stats = stats
    reference_z_scores_windowed.info = dict({k: info.get(k) for k in ("m", "sample_names", "site_names")}, n=n)
    return z_out
