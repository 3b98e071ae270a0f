"""Windowed scoring: how many sites one window holds.  Pure arithmetic, no GPU.

A file whose m x 2n float32 matrix does not fit the device is scored in consecutive windows of W sites; W is a multiple of
8192 (comm.SHARD_ALIGN: one addend of NumPy's running total), so the running total goes from window to window exactly as
it goes from SNP shard to SNP shard.

Device bytes per site of a matrix of n individuals scored against K populations (one group: the --get_pop_like layout):

    matrix       16 * ceil(n / 2)             one float4 per pair of individuals (csrc/common.h: Slab)
    frequencies  4 * K                        K float32 columns (wgs_afset)
    class codes  4 * ceil(n / 4) + 8 * 254    one byte per individual, padded to whole quads, and a dictionary of at most 254
                 + 1 + 8                      (g0, g1) rows (the bound: csrc/common.h: wgs_codes), the class count, and the
                                              encoder's per-wavefront records (csrc/codes.hip: wgs_beagle_codes, the build a
                                              scoring sweep asks for -- without the slabs' own numbering)

The class codes are counted whether or not the cost model will build them for a window: it decides per matrix, after the
window is there.  What may be used is FRACTION (0.8, the share wgs_loo gives its batches) of the free device memory less
RESERVE (4 GiB, at most a quarter of the free memory: the ingest's text and line arrays -- up to 3 GiB of text per chunk
when the device inflates -- the block sums of a sweep, the context's workspace).  A resident matrix needs m sites of it;
windowed scoring holds TWO windows (the one being scored and the one being filled), each with its frequencies and codes.

The other windowed routes, each with its options, variable, planner and driver, are in the table at the head of DESIGN.md
section 5.1; their arithmetic follows below.
"""
import os

ALIGN = 8192                    # = comm.SHARD_ALIGN = WGS_WINDOW_ALIGN of include/wgsassign_hip.h
FRACTION = 0.8
RESERVE = 4 << 30
ENV = "WGSASSIGN_WINDOW_SITES"
ENV_LOO = "WGSASSIGN_LOO_WINDOW_SITES"      # the leave-one-out run is sent to windows by a variable of its own (see plan_loo)
ENV_NE = "WGSASSIGN_NE_WINDOW_SITES"        # ... and so is --ne_obs (see plan_ne)
ENV_Z = "WGSASSIGN_Z_WINDOW_SITES"          # ... and --get_assignment_z_score (see plan_z)
ENV_ZREF = "WGSASSIGN_ZREF_WINDOW_SITES"    # ... and --get_reference_z_score (see plan_zref)
ENV_LOO_DS = "WGSASSIGN_LOO_DS_WINDOW_SITES"    # ... and --loo with --loo_downsampled_beagle (see plan_loo_ds)
SURELY_FITS = 64                # see surely_fits


def site_bytes(n, K):
    """Device bytes one site takes: matrix, frequency columns and the class codes a scoring sweep may build."""
    n, K = int(n), int(K)
    return 16 * ((n + 1) // 2) + 4 * K + 4 * ((n + 3) // 4) + 8 * 254 + 1 + 8


def budget(free_bytes):
    """Device bytes the matrices, frequencies and codes may take of `free_bytes` of free memory."""
    return int(FRACTION * int(free_bytes)) - min(RESERVE, int(free_bytes) // 4)


def env_window_sites(environ=None, name=ENV):
    """WGSASSIGN_WINDOW_SITES (or the variable named) rounded down to a multiple of 8192, or None when it is not set (or empty).
    A value below 8192, or not an integer, is an error that names the variable."""
    value = (os.environ if environ is None else environ).get(name)
    if value is None or not str(value).strip():
        return None
    try:
        sites = int(str(value).strip())
    except ValueError:
        raise ValueError("%s must be a number of sites (an integer >= %d), got %r" % (name, ALIGN, value))
    if sites < ALIGN:
        raise ValueError("%s=%d is below %d sites, the smallest window (windows are multiples of %d sites)" % (name, sites, ALIGN, ALIGN))
    return sites // ALIGN * ALIGN


def surely_fits(compressed_bytes, free_bytes):
    """The first, free look at a file: its matrix fits when SURELY_FITS (64) times its COMPRESSED size fits the budget, and then the
    command line looks no further (no reader opened, no index asked for: the resident run costs what it always did).  A likelihood is
    at least two characters of text and a third of them is dropped, so the matrix is at most 8 / 6 = 1.34 times the text; Beagle text
    deflates about 10 : 1, and 64 holds up to 48 : 1.  (The class codes are left out here: their allocation is asked for on its own
    and a sweep does without them when it fails.)"""
    return SURELY_FITS * int(compressed_bytes) <= budget(free_bytes)


def fits_resident(m, n, K, free_bytes):
    """Whether one matrix of m sites, its frequencies and its codes fit the budget."""
    return int(m) * site_bytes(n, K) <= budget(free_bytes)


def window_count(m, W):
    return (int(m) + int(W) - 1) // int(W)


def explicit_window(window_sites):
    """The window a driver was asked for outright: `window_sites` rounded down to a multiple of 8192; fewer is an error."""
    if int(window_sites) < ALIGN:
        raise ValueError("a window holds at least %d sites, not %d" % (ALIGN, int(window_sites)))
    return int(window_sites) // ALIGN * ALIGN


def whole_file_window(m):
    """The one window that holds all m sites: what a driver runs in when its planner says that everything fits."""
    return max(1, window_count(m, ALIGN)) * ALIGN


def _plan_two_windows(forced, fits, per_site, free_bytes, message, **named):
    """What plan, plan_fit, plan_loo, plan_loo_ds and plan_ne share: `forced` (the route's variable) when it is set, None when the
    resident run `fits`, else the largest multiple of 8192 sites of which two windows of `per_site` bytes a site fit the budget.
    None fits: MemoryError with the route's `message`, filled with sites, bytes (of the two smallest windows), usable, free and
    whatever is `named`."""
    if forced is not None:
        return forced
    if fits:
        return None
    W = budget(free_bytes) // (2 * per_site) // ALIGN * ALIGN
    if W < ALIGN:
        raise MemoryError(message % dict(named, sites=ALIGN, bytes=2 * ALIGN * per_site, usable=max(0, budget(free_bytes)), free=free_bytes))
    return W


def plan(m, n, K, free_bytes, environ=None):
    """The window for scoring m sites x n individuals against K populations with `free_bytes` of device memory free:
    None when the resident matrix fits and WGSASSIGN_WINDOW_SITES does not ask for windows, else W (a multiple of 8192;
    the last window may be shorter).  Too little memory for two windows of 8192 sites is an error."""
    return _plan_two_windows(env_window_sites(environ), fits_resident(m, n, K, free_bytes), site_bytes(n, K), free_bytes,
                             "windowed scoring needs two windows of %(sites)d sites x %(n)d individuals on the device (%(bytes)d bytes "
                             "with their frequencies and class codes); %(usable)d of the %(free)d free bytes can be used", n=n)


def _slab_pairs(n, K, counts=None):
    """float4 columns of the population slabs: per population one per pair of its individuals (fit_site_bytes)."""
    return sum((int(c) + 1) // 2 for c in counts) if counts is not None else (int(n) + int(K)) // 2


def _slab_quads(n, K, counts=None):
    """Code words of the population slabs: per population one per four of its individuals (fit_site_bytes)."""
    return sum((int(c) + 3) // 4 for c in counts) if counts is not None else (int(n) + 3 * int(K)) // 4


def fit_site_bytes(n, K, counts=None):
    """Device bytes one site takes in a windowed --get_reference_af of n individuals in K populations (counts: the individuals
    of every population when known, else the worst split is assumed), from what the library really allocates per site:

        matrix       16 * sum_g ceil(n_g / 2)       one slab per population (csrc/api.hip: wgs_beagle_create), at most
                                                    16 * ((n + K) // 2)
        frequencies  2 * 4 * K                      wgs_em_create's two float32 buffers per fit (csrc/em_api.hip; the third buffer
                                                    of fused sweeps is never asked for by a windowed fit)
        sums         8 * K / 64, rounded up         wgs_em_create's per-tile float64 partial sums: one per fit and 64 sites
        class codes  1 + 8 * 254 + 8                class counts, the dictionary of at most 254 (g0, g1) rows, the encoder's records
                     + sum_g (8 * ceil(n_g / 4)     per slab the codes AND the slab's own numbering of them (one byte per
                              + 1 + 8 * 254)        individual each, whole quads), the per-tile row counts and the slab's own
                                                    dictionary (csrc/codes.hip: wgs_beagle_codes, the build an EM sweep asks for)

    The stopping test's tables (wgs_em_stream: maf_iter x K float64 and float32) and the chains' workspace (60 bytes per fit and
    4096 sites) do not grow with the window worth mentioning and come out of RESERVE."""
    n, K = int(n), int(K)
    pairs, quads = _slab_pairs(n, K, counts), _slab_quads(n, K, counts)
    return 16 * pairs + 8 * K + (8 * K + 63) // 64 + (1 + 8 * 254 + 8) + 8 * quads + K * (1 + 8 * 254)


def fits_resident_fit(m, n, K, free_bytes, counts=None):
    """Whether one matrix of m sites with its EM batch and codes fits the budget."""
    return int(m) * fit_site_bytes(n, K, counts) <= budget(free_bytes)


def plan_fit(m, n, K, free_bytes, environ=None, counts=None):
    """plan() for --get_reference_af: None when the resident fit fits and WGSASSIGN_WINDOW_SITES does not ask for windows, else W (a
    multiple of 8192).  Two windows are held, each with its EM batch and codes."""
    return _plan_two_windows(env_window_sites(environ), fits_resident_fit(m, n, K, free_bytes, counts), fit_site_bytes(n, K, counts),
                             free_bytes,
                             "a windowed fit needs two windows of %(sites)d sites x %(n)d individuals on the device (%(bytes)d bytes "
                             "with their frequency buffers and class codes); %(usable)d of the %(free)d free bytes can be used", n=n)


def loo_site_bytes(n, K, counts=None, P=1):
    """Device bytes one site takes in a windowed --get_reference_af --loo of n individuals in K populations with P partition
    chains: fit_site_bytes with the frequency buffers and per-tile sums counted for the n re-fits of a window instead of K fits
    (all n are ONE EM batch: WGSASSIGN_LOO_BATCH does not apply in windows), plus what the leave-one-out scoring of the window
    allocates per site, read from the library as fit_site_bytes was:

        frequencies  2 * 4 * n                      wgs_em_create's two float32 buffers per re-fit
        sums         8 * n / 64, rounded up         its per-tile float64 partial sums
        columns      4 * K                          the window's rows of the full-population frequencies (wgs_afset)
        block sums   8 * n * K / 4096, rounded up   wgs_score_create: one float64 per (individual, population) and block of 4096
                                                    sites,
        chunk sums   8 * n * K / 8192, rounded up   and one per chunk of 8192 (score_sums_enqueue)
        chains       4 * n * K * P / 4096, r. up    wgs_score_chains_prepare: one block function per chain and block

    The column table (8 n K bytes), the chains' carries and results (12 n K P) and the stream's totals do not grow with the
    window and come out of RESERVE."""
    n, K, P = int(n), int(K), max(1, int(P))
    cells = n * K
    return (fit_site_bytes(n, K, counts) - 8 * K - (8 * K + 63) // 64 + 8 * n + (8 * n + 63) // 64 + 4 * K
            + (8 * cells + 4095) // 4096 + (8 * cells + 8191) // 8192 + (4 * cells * P + 4095) // 4096)


def plan_loo(m, n, K, free_bytes, environ=None, counts=None, P=1):
    """plan() for --get_reference_af --loo: None when the resident matrix fits (the resident run batches its re-fits by what is
    left and needs only the matrix: fits_resident_fit) and WGSASSIGN_LOO_WINDOW_SITES does not ask for windows, else W (a
    multiple of 8192) for two windows, each with its batch of n re-fits."""
    return _plan_two_windows(env_window_sites(environ, ENV_LOO), fits_resident_fit(m, n, K, free_bytes, counts),
                             loo_site_bytes(n, K, counts, P), free_bytes,
                             "a windowed leave-one-out run needs two windows of %(sites)d sites x %(n)d individuals on the device "
                             "(%(bytes)d bytes with their %(n)d re-fits, class codes and scoring tables); %(usable)d of the %(free)d "
                             "free bytes can be used", n=n)


def loo_ds_site_bytes(n, K, counts=None, P=1):
    """Device bytes one KEPT site takes in a windowed --get_reference_af --loo --loo_downsampled_beagle: loo_site_bytes for the
    window of the reference file, plus what the window of the downsampled file -- the matrix that is scored -- adds per site:

        matrix       16 * sum_g ceil(n_g / 2)       one more set of population slabs (csrc/api.hip: wgs_beagle_create), at most
                                                    16 * ((n + K) // 2)
        class codes  1 + 8 * 254 + 8                the codes a scoring sweep may build on the scored matrix (csrc/codes.hip:
                     + sum_g (4 * ceil(n_g / 4)     wgs_beagle_codes, for_scoring_only): class counts, the dictionary, the encoder's
                              + 1)                  records, and per slab the codes and the per-tile row counts -- without the slabs'
                                                    own numbering and dictionaries, which only an EM sweep asks for

    The re-fits never look at the scored matrix, so it carries no EM batch."""
    n, K = int(n), int(K)
    pairs, quads = _slab_pairs(n, K, counts), _slab_quads(n, K, counts)
    return loo_site_bytes(n, K, counts, P) + 16 * pairs + (1 + 8 * 254 + 8) + 4 * quads + K


def fits_resident_loo_ds(m, n, K, free_bytes, counts=None):
    """Whether the TWO resident matrices of m kept sites fit the budget: the reference file's with its EM batch and codes
    (fit_site_bytes) and the downsampled file's with the codes of a scoring sweep."""
    return int(m) * (fit_site_bytes(n, K, counts) + loo_ds_site_bytes(n, K, counts) - loo_site_bytes(n, K, counts)) <= budget(free_bytes)


def plan_loo_ds(m_kept, n, K, free_bytes, environ=None, counts=None, P=1):
    """plan() for --get_reference_af --loo --loo_downsampled_beagle over m_kept kept sites: None when two resident matrices fit
    (fits_resident_loo_ds) and WGSASSIGN_LOO_DS_WINDOW_SITES does not ask for windows, else W (a multiple of 8192 KEPT sites) for
    two windows of each file, the reference file's with their batches of n re-fits."""
    return _plan_two_windows(env_window_sites(environ, ENV_LOO_DS), fits_resident_loo_ds(m_kept, n, K, free_bytes, counts),
                             loo_ds_site_bytes(n, K, counts, P), free_bytes,
                             "a windowed leave-one-out run on downsampled likelihoods needs two windows of %(sites)d sites x %(n)d "
                             "individuals of both files on the device (%(bytes)d bytes with their %(n)d re-fits, class codes and scoring "
                             "tables); %(usable)d of the %(free)d free bytes can be used", n=n)


def kept_windows(keep, W):
    """Windows of W KEPT sites under a site mask, as file rows: for every window (kept_lo, kept_count, row_first, row_end) -- the
    window holds the kept sites [kept_lo, kept_lo + kept_count), which lie in the file rows [row_first, row_end); row_first and
    row_end - 1 are kept rows, so a window's slice of the mask neither begins nor ends in dropped rows, and the dropped rows
    between two windows belong to neither.  A pure function of the mask and W; a mask that keeps nothing has no windows."""
    import numpy as np
    W = int(W)
    if W < 1:
        raise ValueError("a window holds at least one site")
    kept_rows = np.flatnonzero(np.asarray(keep, dtype=bool))
    out = []
    for lo in range(0, len(kept_rows), W):
        hi = min(len(kept_rows), lo + W)
        out.append((lo, hi - lo, int(kept_rows[lo]), int(kept_rows[hi - 1]) + 1))
    return out


def ne_site_bytes(n, K, counts=None):
    """Device bytes one site takes in a windowed --get_reference_af --ne_obs pass of n individuals in K populations (counts: the
    individuals of every population when known, else the worst split), from what wgs_fisher_stream_push allocates per site:

        matrix       16 * sum_g ceil(n_g / 2)       one slab per population, at most 16 * ((n + K) // 2)
        frequencies  4 * K                          the window's rows of the fitted frequencies (wgs_afset)
        results      3 * 4 * K                      f_obs and ne_obs, population-major, and the site-major copy that crosses to the host
        leaf sums    4 * n / 128, rounded up        one float32 per individual and 128-site leaf of a full 8192-site chunk

    The row matrix of the file's last, shorter chunk (n x at most 8191 float32), its leaf sums, the plans and the stream's totals do
    not grow with the window and come out of RESERVE."""
    n, K = int(n), int(K)
    return 16 * _slab_pairs(n, K, counts) + 4 * K + 12 * K + (4 * n + 127) // 128


def plan_ne(m, n, K, free_bytes, environ=None, counts=None, loo=False, P=1):
    """plan() for --get_reference_af --ne_obs: None when the resident matrix fits (fits_resident_fit) and
    WGSASSIGN_NE_WINDOW_SITES does not ask for windows, else W (a multiple of 8192) for two windows: the fit's (plan_fit's
    arithmetic), or the Fisher pass's when that is smaller.  loo: --loo runs beside it in the same windows, so the window is the
    smaller of this and what plan_loo derives."""
    per_site = max(fit_site_bytes(n, K, counts), ne_site_bytes(n, K, counts))
    if loo:
        per_site = max(per_site, loo_site_bytes(n, K, counts, P))
    return _plan_two_windows(env_window_sites(environ, ENV_NE), fits_resident_fit(m, n, K, free_bytes, counts), per_site, free_bytes,
                             "a windowed --ne_obs run needs two windows of %(sites)d sites x %(n)d individuals on the device (%(bytes)d "
                             "bytes with their frequency buffers, class codes and Fisher results); %(usable)d of the %(free)d free bytes "
                             "can be used", n=n)


Z_RESIDENT_BATCH = 64           # individuals per launch of the resident z-score path (zscore.assignment_z_scores)


def z_state_bytes(count):
    """Device bytes that `count` individuals carry from window to window in a windowed --get_assignment_z_score (csrc/zscore.h:
    wgs_zsum), charged ONCE, not per site: per individual three open chunks of 8192 float32, three running values, the class sweep's
    256 x 3 running sums and three job records of 48 bytes."""
    return int(count) * (3 * ALIGN * 4 + 3 * 4 + 256 * 3 * 4 + 3 * 48)


def z_site_bytes(n, K, count):
    """Device bytes one site of ONE window takes in a windowed --get_assignment_z_score of n individuals against K populations, `count`
    of them in the batch, from what the library allocates per site:

        matrix       16 * ceil(n / 2)               one group, as --get_pop_like lays it out
        depths       2 * n                          one byte pair per (individual, site) (csrc/zscore.h: wgs_depth)
        frequencies  4 * K                          the window's rows of the frequency file (wgs_afset)
        mask words   12 * count / 64, rounded up    per (individual of the batch, tile of 64 sites) the kept-site word and its offset
                                                    (wgs_zkeep; the deep-site list of pass A takes the same and is gone by then)
        statistics   12 * count                     the three compacted float32 arrays, at most one element per (individual, site)

    The window that is being filled beside it is one more MATRIX (reader_cy.stream_windows holds two), nothing else: plan_z adds it."""
    n, K, count = int(n), int(K), int(count)
    return 16 * ((n + 1) // 2) + 2 * n + 4 * K + (12 * count + 63) // 64 + 12 * count


def fits_resident_z(m, n, K, count, free_bytes):
    """Whether the resident z-score run fits: matrix, depth table and frequencies of all m sites, and the masks and statistics of one
    batch of at most Z_RESIDENT_BATCH individuals."""
    return int(m) * z_site_bytes(n, K, min(int(count), Z_RESIDENT_BATCH)) <= budget(free_bytes)


def _round_batch(W, count, state_bytes, window_bytes, free_bytes):
    """What z_batch and zref_batch share: all `count` individuals when state_bytes(batch) and W sites of window_bytes(batch) each fit
    the budget, else the largest half, quarter, ... of them that does (at least one)."""
    batch = max(1, int(count))
    while batch > 1 and state_bytes(batch) + int(W) * window_bytes(batch) > budget(free_bytes):
        batch = (batch + 1) // 2
    return batch


def _plan_rounds(forced, fits, count, state_bytes, window_bytes, free_bytes, message, **named):
    """What plan_z and plan_zref share: None when the route's variable is not set (`forced` is None) and the resident run `fits`; with
    the variable set (forced, _round_batch(forced, ...)), whether or not that fits; else (W, batch) with batch = count halved until a
    window of 8192 sites of window_bytes(batch) each fits beside state_bytes(batch), and W the largest multiple of 8192 that does.
    Not even one individual: MemoryError with the route's `message`, filled with sites, bytes (of the smallest window), state (of one
    individual), usable, free and whatever is `named`."""
    if forced is not None:
        return forced, _round_batch(forced, count, state_bytes, window_bytes, free_bytes)
    if fits:
        return None
    batch = count
    while True:
        room = budget(free_bytes) - state_bytes(batch)
        W = room // window_bytes(batch) // ALIGN * ALIGN if room > 0 else 0
        if W >= ALIGN or batch == 1:
            break
        batch = (batch + 1) // 2
    if W < ALIGN:
        raise MemoryError(message % dict(named, sites=ALIGN, bytes=ALIGN * window_bytes(batch), state=state_bytes(1),
                                         usable=max(0, budget(free_bytes)), free=free_bytes))
    return W, batch


def _z_window_bytes(n, K, batch):
    """Per site of a window with the second matrix beside it."""
    return z_site_bytes(n, K, batch) + 16 * ((int(n) + 1) // 2)


def z_batch(W, n, K, count, free_bytes):
    """Individuals per round for windows of W sites: all `count` when their state and one window's objects fit beside the second
    matrix, else the largest half, quarter, ... of them that does (at least one)."""
    return _round_batch(W, count, z_state_bytes, lambda batch: _z_window_bytes(n, K, batch), free_bytes)


def plan_z(m, n, K, count, free_bytes, environ=None):
    """plan() for --get_assignment_z_score of `count` individuals: None when the resident objects fit (fits_resident_z) and
    WGSASSIGN_Z_WINDOW_SITES does not ask for windows, else (W, batch): windows of W sites (a multiple of 8192) and rounds of `batch`
    individuals.  batch = count -- one round, two passes over the files -- whenever the state of all of them (z_state_bytes) leaves
    room for a window of 8192 sites beside the second matrix; otherwise the largest half, quarter, ... of them that does."""
    m, n, K, count = int(m), int(n), int(K), int(count)
    return _plan_rounds(env_window_sites(environ, ENV_Z), fits_resident_z(m, n, K, count, free_bytes), count, z_state_bytes,
                        lambda batch: _z_window_bytes(n, K, batch), free_bytes,
                        "windowed z-scores need two windows of %(sites)d sites x %(n)d individuals on the device (%(bytes)d bytes with the "
                        "depths, frequencies, masks and statistics of one) and %(state)d bytes of state per individual; %(usable)d of the "
                        "%(free)d free bytes can be used", n=n)


def _zref_fits_bytes(count):
    """Per site what an EM batch of `count` fits holds: two float32 frequency buffers per fit and the per-tile float64 partial sums
    (loo_site_bytes counts the same for its n re-fits)."""
    return 8 * int(count) + (8 * int(count) + 63) // 64


def zref_state_bytes(count, maf_iter=200):
    """Device bytes that `count` individuals carry from window to window in a windowed --get_reference_z_score, charged ONCE:
    z_state_bytes and the fit stream's tables (wgs_em_stream: maf_iter x count float64 sums, unused here, and float32 carries)."""
    return z_state_bytes(count) + 12 * max(1, int(maf_iter)) * int(count)


def zref_site_bytes(n, K, count, counts=None):
    """Device bytes one site of ONE window takes in a windowed --get_reference_z_score of n individuals in K populations (counts: the
    individuals of every population when known, else the worst split), `count` of them in the batch: z_site_bytes without a frequency
    file, with the population slabs in place of the one slab, plus what the batch of masked leave-one-out fits adds per site:

        matrix       16 * sum_g ceil(n_g / 2)       one slab per population, at most 16 * ((n + K) // 2)
        depths       2 * n                          one byte pair per (individual, site)
        mask words   12 * count / 64, rounded up    the kept-site word and its offset per (individual of the batch, tile)
        statistics   12 * count                     the three compacted float32 arrays
        frequencies  2 * 4 * count                  wgs_em_create's two float32 buffers per fit
        sums         8 * count / 64, rounded up     its per-tile float64 partial sums
        compacted    2 * 4 * count                  (f_t, f_t-1) over the kept sites of every fit (wgs_em_stream_push_masked): at most
                                                    one pair per (fit, site)

    The class codes an EM sweep may build are left out, as surely_fits leaves them out: their allocation is asked for on its own and
    a sweep does without them when it fails.  The window that is being filled beside it is one more matrix with its batch of fits
    (the batch stays with its matrix): plan_zref adds both."""
    n, K, count = int(n), int(K), int(count)
    return 16 * _slab_pairs(n, K, counts) + 2 * n + (12 * count + 63) // 64 + 12 * count + _zref_fits_bytes(count) + 8 * count


def fits_resident_zref(m, n, K, count, free_bytes, counts=None):
    """Whether the resident --get_reference_z_score fits: matrix and depth table of all m sites and one batch of at most
    Z_RESIDENT_BATCH masked fits with their masks, statistics and compacted vectors."""
    return int(m) * zref_site_bytes(n, K, min(int(count), Z_RESIDENT_BATCH), counts) <= budget(free_bytes)


def _zref_window_bytes(n, K, batch, counts=None):
    """Per site of a window with the second matrix and its batch of fits beside it."""
    return zref_site_bytes(n, K, batch, counts) + 16 * _slab_pairs(n, K, counts) + _zref_fits_bytes(batch)


def zref_batch(W, n, K, count, free_bytes, maf_iter=200, counts=None):
    """Individuals per round for windows of W sites: all `count` when their state and the two windows' objects fit, else the largest
    half, quarter, ... of them that does (at least one)."""
    return _round_batch(W, count, lambda batch: zref_state_bytes(batch, maf_iter), lambda batch: _zref_window_bytes(n, K, batch, counts),
                        free_bytes)


def plan_zref(m, n, K, count, free_bytes, maf_iter=200, environ=None, counts=None):
    """plan() for --get_reference_z_score of `count` individuals: None when the resident objects fit (fits_resident_zref) and
    WGSASSIGN_ZREF_WINDOW_SITES does not ask for windows, else (W, batch): windows of W sites (a multiple of 8192) and rounds of `batch`
    individuals, halved as plan_z halves them until a window of 8192 sites fits beside their state."""
    m, n, K, count = int(m), int(n), int(K), int(count)
    return _plan_rounds(env_window_sites(environ, ENV_ZREF), fits_resident_zref(m, n, K, count, free_bytes, counts), count,
                        lambda batch: zref_state_bytes(batch, maf_iter), lambda batch: _zref_window_bytes(n, K, batch, counts), free_bytes,
                        "windowed reference z-scores need two windows of %(sites)d sites x %(n)d individuals on the device (%(bytes)d bytes "
                        "with the depths, masks, statistics and masked fits of one) and %(state)d bytes of state per individual; "
                        "%(usable)d of the %(free)d free bytes can be used", n=n)
