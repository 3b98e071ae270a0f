"""Enumerated inputs for the --ne_obs kernels (csrc/em_kernels.hip: fisher_term, fisher_pop_kernel, fisher_ind_sites_kernel,
pairwise_leaf_kernel / pairwise_combine_kernel, fisher_window_kernel and its two stream kernels), each built for a place the generated
matrices of tests/test_gpu_fisher.py and tests/test_gpu_windowed_ne_obs.py never reach: the term's arithmetic off the beaten path
(hard calls, likelihoods that sum to more than 1, frequencies of 0, 1 and subnormal ones, a denominator of 0, results that are
subnormal, infinite, NaN or a signed zero), population slabs that take fisher_window_kernel round its loop of four pairs more than once,
the per-site values that a mean would hide, and populations whose finite sum a frequency turns into a signed zero.  NumPy only; the
twin of tests/zscore_cases.py, tests/codes_cases.py and tests/token_cases.py.  Every builder is deterministic and returns the inputs next to the claims they are built to satisfy;
tests/test_fisher_cases_cpu.py holds them to those claims on the oracle, and tests/test_gpu_fisher_cases.py runs them through the
library."""
import numpy as np

import synth

F32 = np.float32

# ---- the term grid -------------------------------------------------------------------------------------------------------------
# Likelihood pairs (g0, g1).  The first thirteen are the grid the enumeration started from: the two hard calls and the empty pair, a
# missing genotype as ANGSD writes it, float32 sums above 1 (g2 < 0), near-hard calls, and pairs so small that u = g0 is tiny or
# subnormal when the frequency vanishes.
PAIRS_BASE = ((1, 0), (0, 1), (0, 0), (0.333333, 0.333333), (0.666667, 0.333334), (0.999999, 1e-6), (1e-6, 0.999999), (1e-6, 1e-6),
              (0.5, 0.5), (0.25, 0.5), (0.9, 0.2), (1e-30, 1e-30), (1e-42, 0))
# Added:
#   (0.6, 0.6)      a sum far above 1: g2 = -0.2, every product with g2 carries its sign (the base grid's g2 < 0 are all tiny);
#   (0.5, 0.25)     n1/u == (n2/u)^2 exactly at a frequency of 0: the term is -1.0 * (+0.0) = -0.0 -- a negative zero BEFORE the
#                   multiplication by the frequency, whatever that is; and negative terms at every frequency;
#   (0, 0.5)        g0 = 0 without a hard call: u vanishes only with the frequency;
#   (1e-38, 1e-38)  terms of -2e38, the largest finite magnitude float32 holds here (n1 / u just below overflow);
#   (1, 1e-8)       g2 = -1e-8: the smallest negative g2 a float32 pair next to 1 gives;
#   (0.2, 0.1), (0.05, 0.05), (0.1, 0.1)   negative terms of ordinary size at ordinary frequencies (g0 + g2 > 2 g1): negative ne that
#                   are neither tiny nor huge, so a sign or operand mix-up in the last product shows at ordinary sites.
PAIRS_ADDED = ((0.6, 0.6), (0.5, 0.25), (0, 0.5), (1e-38, 1e-38), (1, 1e-8), (0.2, 0.1), (0.05, 0.05), (0.1, 0.1))
PAIRS = PAIRS_BASE + PAIRS_ADDED
# the pairs whose term is infinite or NaN at some frequency strictly inside (0, 1): left out of the `finite` variant
NOT_FINITE_INSIDE = ((0, 1), (0, 0), (1e-42, 0), (0, 0.5))

# Frequencies.  The first twelve are the grid's: 0 and 1, the smallest subnormal, a subnormal, one whose square is subnormal, one
# below float32's epsilon, the clamp bounds of a population of 84, two exact binary fractions, the float32 below 1 and 0.999.
FREQS_BASE = (0.0, 1.0, 1e-45, 1e-38, 1e-20, 1e-7, 1 / 170, 0.25, 0.5, 1 - 1 / 170, float(np.nextafter(F32(1), F32(0))), 0.999)
# Added:
#   -0.0            a zero with a sign: 0.5 * f * (-0.0) * 1 turns the sign of every POSITIVE term's zero (hostile only);
#   2.0             the library takes any af: 1 - th is negative and so is every ne of a positive term (hostile only);
#   0.75, 1/3, 2/3, 0.4, 0.6, 0.1, 0.9, 0.02, 0.98, 0.05   ordinary frequencies on both sides of 1/2 with full mantissas: where a
#                   float32 product written in double, or a divide written as a reciprocal multiply, rounds differently;
#   2^-12, 1 - 2^-12  th * th and (1 - th) exact in float32, next to frequencies where they are not;
#   1e-3, 1e-5      between the clamp bound and epsilon;
#   1/34, 1 - 1/34, 1/8   the clamp bounds of populations of 16 and of 3.
# They also keep the frequencies with non-finite terms (0, -0.0, 1, 1e-45, 1e-38, 1e-20) below a quarter of all, and both variants'
# counts odd (grid_in_windows).
FREQS_ADDED = (-0.0, 2.0, 0.75, 1 / 3, 2 / 3, 0.4, 0.6, 0.1, 0.9, 0.02, 0.98, 0.05, 2.0 ** -12, 1 - 2.0 ** -12, 1e-3, 1e-5, 1 / 34,
               1 - 1 / 34, 1 / 8)
FREQS = FREQS_BASE + FREQS_ADDED
VARIANTS = ("finite", "hostile")
GRID_M = 197                      # three tiles and a partial one


def variant_lists(variant):
    """(pairs (np, 2) float32, freqs (nf,) float32) of a variant.  hostile: everything.  finite: the frequencies strictly inside
    (0, 1) and the pairs whose term the reference keeps finite at every one of them."""
    assert variant in VARIANTS
    if variant == "hostile":
        pairs, freqs = PAIRS, FREQS
    else:
        pairs = tuple(p for p in PAIRS if p not in NOT_FINITE_INSIDE)
        freqs = tuple(f for f in FREQS if 0.0 < float(F32(f)) < 1.0)
    return np.array(pairs, dtype=np.float64).astype(F32), np.array(freqs, dtype=np.float64).astype(F32)


def ids_for(labels):
    return np.array([["Ind%d" % i, "pop%02d" % k] for i, k in enumerate(labels)], dtype=str)


def group_of(IDs):
    pops = np.unique(IDs[:, 1])
    return np.searchsorted(pops, IDs[:, 1]).astype(np.int32), len(pops)


def term_grid(variant, m=GRID_M):
    """One frequency per site, one likelihood pair per individual.  There are as many populations as frequencies, nf, and every
    population holds every pair once:
        population k, site s      frequency freqs[(s + k) % nf]
        population k, column c    pair pairs[(c + k) % np]              (column c: the c-th of its individuals in file order)
        individual c * nf + k     is column c of population k           (the populations interleave in file order)
    so EVERY cell (pair, frequency) of the grid -- hence every class of result -- stands at the first site (in population k = its
    frequency's number), at the last site, at lanes 0 and 63 of a tile, and in both halves of a slab's float4 (columns of both
    parities: x/y and z/w).  Returns dict(L (m, 2n), af (m, nf), IDs, pairs, freqs, pair_of (n,), freq_of (m, nf), pop_of (n,),
    col_of (n,)): the last four say which pair, frequency, population and slab column a cell has."""
    pairs, freqs = variant_lists(variant)
    n_pairs, nf = len(pairs), len(freqs)
    n = n_pairs * nf
    i = np.arange(n)
    col_of, pop_of = i // nf, i % nf
    pair_of = (col_of + pop_of) % n_pairs
    freq_of = (np.arange(m)[:, None] + np.arange(nf)[None, :]) % nf
    L = np.empty((m, 2 * n), dtype=F32)
    L[:, 0::2] = pairs[pair_of, 0][None, :]
    L[:, 1::2] = pairs[pair_of, 1][None, :]
    af = np.ascontiguousarray(freqs[freq_of])
    assert m > 3 * 64 and m % 64 and nf <= 64 and n_pairs > 2
    return dict(variant=variant, L=L, af=af, IDs=ids_for(pop_of), pairs=pairs, freqs=freqs, pair_of=pair_of, freq_of=freq_of,
                pop_of=pop_of, col_of=col_of)


def cell_places(grid, p, f):
    """Where the cell (pair number p, frequency number f) of a term_grid stands: [(individual, its slab column, sites)]."""
    out = []
    for i in np.flatnonzero(grid["pair_of"] == p):
        sites = np.flatnonzero(grid["freq_of"][:, grid["pop_of"][i]] == f)
        out.append((int(i), int(grid["col_of"][i]), sites))
    return out


# ---- ordinary likelihoods in populations of every slab shape -----------------------------------------------------------------------
# 1 .. 17 pairs: every npairs % 4, one to five trips of fisher_window_kernel's loop, odd and even last columns.  11, 14 and 27 are
# there for a LAST trip of two and of three pairs after the first (6, 7 and 14 pairs) and for a walk of exactly four trips.
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 11, 14, 15, 16, 17, 27, 33)
M_RESIDENT, M_TAIL, M_TWO = 197, 8192 + 200, 16384    # three tiles and a partial one; a full chunk and a tail; two chunks


def interleave(sizes):
    """Population labels in file order, round-robin until every population has its size: a total filed under a slab column instead
    of an individual shows.  (The largest population ends the file with a run of its own.)"""
    return np.array([k for r in range(max(sizes)) for k, size in enumerate(sizes) if r < size], dtype=np.int64)


def clamp_bounds(sizes):
    """The float32 clamp bounds of WGSassign.py:236-240 for populations of these sizes."""
    lo = np.array([1 / (2 * (s + 1)) for s in sizes]).astype(F32)
    hi = np.array([1 - 1 / (2 * (s + 1)) for s in sizes]).astype(F32)
    return lo, hi


def clamped_frequencies(m, sizes, seed):
    """(m, K) float32 inside the clamp; per population every seventh site at its lower bound and every eleventh at its upper one."""
    lo, hi = clamp_bounds(sizes)
    rng = np.random.Generator(np.random.PCG64(seed))
    af = np.clip(rng.random((m, len(sizes))).astype(F32), lo, hi).astype(F32)
    for k in range(len(sizes)):
        af[k::7, k] = lo[k]
        af[k + 3::11, k] = hi[k]
    return af


def population_shapes(m, sizes=SIZES, seed=4100):
    """dict(L, af, IDs, labels, sizes): synth.make_beagle_for_labels for populations of `sizes`, interleaved in file order, with
    frequencies inside the clamp and at its bounds."""
    labels = interleave(sizes)
    L, IDs = synth.make_beagle_for_labels(m, labels, len(sizes), seed=seed + len(labels))
    return dict(L=L, af=clamped_frequencies(m, sizes, seed + m), IDs=IDs, labels=labels, sizes=tuple(sizes))


# ---- the grid in windows -------------------------------------------------------------------------------------------------------------
WINDOW = 8192
WINDOW_SIZES = (3, 9)             # one trip with an odd last column; two trips, the second of one column (the LDS turn-round again)
HOT_COLUMNS = ((2,), (1, 4, 8))   # hostile: the slab columns (per population) that take the pairs with non-finite terms
HOT_FIRST = ((0, 1), (0, 0), (1e-42, 0))


def grid_in_windows(variant, m=M_TAIL):
    """The grid's cells over `m` = 8192 + 200 sites for populations of 3 and 9: a full chunk for fisher_window_kernel and a tail for
    the row route.  With t = s - 8191 (site 8191 is the anchor) population k has frequency freqs[(t + k) % nf] at site s, and the
    pairs move on by one every nf sites, so every individual meets every cell and a cell meets every site number modulo 128 (nf and 128 share no
    factor): the first and last site of a 128-site leaf, both its tiles, and the tail.  The sites 8191 and 8192 have the
    frequencies number 0, 1 (population 0) and 1, 2 (population 1): 0, 1 and the smallest subnormal in `hostile`, the three
    smallest frequencies in `finite`.
    finite: column c holds pairs[(c + t // nf) % np].
    hostile: only the columns HOT_COLUMNS go through all pairs -- starting, at the anchor, with HOT_FIRST -- so that the other
    individuals' means stay finite and say something; those go through the pairs that are finite at EVERY frequency.
    Returns dict(L, af, IDs, labels, sizes, pair_at (m, n) pair number per cell, freq_at (m, K), pairs, freqs, hot (n,) bool)."""
    pairs, freqs = variant_lists(variant)
    nf = len(freqs)
    labels = interleave(WINDOW_SIZES)
    n = len(labels)
    col_of = np.array([int((labels[:i] == labels[i]).sum()) for i in range(n)])
    t = np.arange(m, dtype=np.int64) - (WINDOW - 1)
    block = t // nf                                          # floor division: negative before the anchor's block
    freq_at = (t[:, None] + np.arange(len(WINDOW_SIZES))[None, :]) % nf
    hot = np.zeros(n, dtype=bool)
    pair_at = np.empty((m, n), dtype=np.int64)
    if variant == "hostile":
        key = [tuple(float(x) for x in p) for p in pairs]
        first = [key.index(tuple(float(F32(x)) for x in p)) for p in HOT_FIRST]
        order_all = np.array(first + [j for j in range(len(pairs)) if j not in first])
        wild = [tuple(float(F32(x)) for x in p) for p in NOT_FINITE_INSIDE + ((1, 0), (0.5, 0.5))]
        tame = np.array([j for j in range(len(pairs)) if key[j] not in wild])
        for i in range(n):
            cols = HOT_COLUMNS[labels[i]]
            if col_of[i] in cols:
                hot[i] = True
                pair_at[:, i] = order_all[(cols.index(col_of[i]) + block) % len(order_all)]
            else:
                pair_at[:, i] = tame[(col_of[i] + block) % len(tame)]
    else:
        for i in range(n):
            pair_at[:, i] = (col_of[i] + block) % len(pairs)
    L = np.empty((m, 2 * n), dtype=F32)
    L[:, 0::2] = pairs[pair_at, 0]
    L[:, 1::2] = pairs[pair_at, 1]
    af = np.ascontiguousarray(freqs[freq_at])
    assert np.gcd(nf, 128) == 1 and m > WINDOW + 128
    return dict(variant=variant, L=L, af=af, IDs=ids_for(labels), labels=labels, sizes=WINDOW_SIZES, pair_at=pair_at, freq_at=freq_at,
                pairs=pairs, freqs=freqs, hot=hot, col_of=col_of)


# ---- populations whose SUM is a finite number that a frequency turns into -0.0 ------------------------------------------------------
# In term_grid every population holds every pair, so wherever a frequency makes a product -0.0 some hard call has already made the
# population's sum infinite or NaN: the per-site rows meet the signed zero there, fisher_pop_kernel's ne_obs never does.  Here each
# population holds only pairs with g0 != 0 and g2 != 0, whose terms are finite at every frequency, chosen so that the sum has the sign
# that its own frequency ZERO_FREQS[k] turns into a product of -0.0 (names, pairs, and that frequency):
ZERO_POPULATIONS = (
    ("negative at 0", ((0.2, 0.1), (0.05, 0.05), (0.1, 0.1)), 0.0),                  # u = g0, g0 + g2 > 2 g1: every term negative
    ("negative at 1", ((0.7, 0.1), (0.9, 0.05), (0.8, 0.1), (0.7, 0.1)), 1.0),        # the same with g0 and g2 exchanged: u = g2
    ("underflows", ((0.5, 0.24), (0.5, 0.24)), 1e-45),                               # a sum of -0.08: half of it times 1.4e-45 is no float32
    ("positive at -0.0", ((0.25, 0.5), (0.9, 0.2), (0.25, 0.5), (0.9, 0.2), (0.25, 0.5)), -0.0))
ZERO_FREQS = tuple(z for _, _, z in ZERO_POPULATIONS)
# the frequencies of the other sites: ordinary ones, and tiny ones at which the products are tiny but not zero
ZERO_ORDINARY = (0.25, 1e-38, 0.5, 1 / 170, 1e-20, 0.999, 1 / 3, 1 - 1 / 170, 0.9)
M_ZEROS = 198                     # three tiles and a partial one, whose last site takes the same frequency as the first


def zero_site(s):
    """The sites of signed_zeros that take a frequency of ZERO_FREQS: lanes 0 and 63 of every tile, the last site, one in five."""
    return (s % 64 == 0) | (s % 64 == 63) | (s % 5 == 2) | (s == M_ZEROS - 1)


def signed_zeros(m=M_ZEROS):
    """dict(L, af, IDs, labels, sizes, own (m, K) bool): the populations of ZERO_POPULATIONS (3, 4, 2 and 5 individuals: odd and even
    last columns, one to three pairs of columns), interleaved in file order.  At a site s of zero_site() population k has the frequency
    ZERO_FREQS[(s // 64 + s % 64 + k) % 4], so it meets each of the four at lane 0, and its OWN (`own`) at the first site, at the last
    one and at a lane 63; elsewhere ZERO_ORDINARY[(s + k) % 9]."""
    assert m == M_ZEROS and ((m - 1) // 64 + (m - 1) % 64) % 4 == 0 and m > 3 * 64 and m % 64
    sizes = tuple(len(p) for _, p, _ in ZERO_POPULATIONS)
    K = len(sizes)
    labels = interleave(sizes)
    n = len(labels)
    col_of = np.array([int((labels[:i] == labels[i]).sum()) for i in range(n)])
    pair = np.array([ZERO_POPULATIONS[k][1][c] for k, c in zip(labels, col_of)], dtype=np.float64).astype(F32)
    L = np.empty((m, 2 * n), dtype=F32)
    L[:, 0::2] = pair[:, 0][None, :]
    L[:, 1::2] = pair[:, 1][None, :]
    s, k = np.arange(m)[:, None], np.arange(K)[None, :]
    which = (s // 64 + s % 64 + k) % K
    zf, of = np.array(ZERO_FREQS, dtype=np.float64).astype(F32), np.array(ZERO_ORDINARY, dtype=np.float64).astype(F32)
    af = np.ascontiguousarray(np.where(zero_site(s), zf[which], of[(s + k) % len(of)]).astype(F32))
    return dict(L=L, af=af, IDs=ids_for(labels), labels=labels, sizes=sizes, col_of=col_of, own=zero_site(s) & (which == k))


def stored_product(f, af):
    """What a kernel that STORES n_tilde = (float)(0.5 * f * a * (1 - a)) (fisher_cy.pyx:37, :64) holds where the reference, which adds
    it to a zero, has ne: equal to ne everywhere but in the sign of a zero."""
    with np.errstate(all="ignore"):
        a = np.asarray(af, dtype=np.float64)
        return (((0.5 * np.asarray(f, dtype=np.float64)) * a) * (1.0 - a)).astype(F32)


# ---- what the tests share ----------------------------------------------------------------------------------------------------------------
# the inputs that tests/golden/fisher_cases.npz records the real reference on: name -> (builder, its arguments as the golden names them)
GOLDEN = {"finite": ("term_grid", dict(variant="finite", m=GRID_M)), "hostile": ("term_grid", dict(variant="hostile", m=GRID_M)),
          "zeros": ("signed_zeros", dict(m=M_ZEROS))}
_reference = {}


def reference(orc, builder, *args):
    """(case, dict(f_obs, ne_obs, ne_ind, f_rows, ne_rows)) of a builder on the oracle: computed once, shared, read-only."""
    key = (builder,) + args
    if key not in _reference:
        case = globals()[builder](*args)
        L, af, IDs = case["L"], case["af"], case["IDs"]
        f_obs, ne_obs = orc.fisher_obs(L, af.copy(), IDs, 2)
        f_rows, ne_rows = oracle_rows(orc, L, af, IDs)
        with np.errstate(all="ignore"):
            ne_ind = orc.fisher_obs_ind(L, af.copy(), IDs, 2)
        want = dict(f_obs=f_obs, ne_obs=ne_obs, ne_ind=ne_ind, f_rows=f_rows, ne_rows=ne_rows)
        for a in list(want.values()) + [L, af]:
            a.setflags(write=False)
        _reference[key] = (case, want)
    return _reference[key]


def digest(case):
    return synth.digest(np.concatenate((case["L"].ravel().view(np.uint32), case["af"].ravel().view(np.uint32))))


def oracle_rows(orc, L, af, IDs):
    """(f_ind, ne_ind), both (n, m) float32: per individual the rows fisher_cy.pyx:41-65 fills (from zeros) before fisher.py:59 takes
    np.mean of the second -- the oracle's orc_fisher_obs_ind, site by site."""
    pops = np.unique(IDs[:, 1])
    col = np.searchsorted(pops, IDs[:, 1])
    m, n = L.shape[0], L.shape[1] // 2
    f_rows = np.zeros((n, m), dtype=F32)
    ne_rows = np.zeros((n, m), dtype=F32)
    L, af = np.ascontiguousarray(L, dtype=F32), np.ascontiguousarray(af, dtype=F32)
    lib = orc.lib()
    for i in range(n):
        lib.orc_fisher_obs_ind(orc._p(L), m, n, orc._p(af), af.shape[1], i, int(col[i]), orc._p(f_rows[i]), orc._p(ne_rows[i]), 1)
    return f_rows, ne_rows


def same_nan(a, b):
    """Bit-identical where the reference is not NaN, NaN exactly where it is."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return a[ok].tobytes() == b[ok].tobytes()


def first_difference(got, want):
    """None, or the flat index of the first value that is not the reference's (NaN for NaN counts as equal)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F32, (got.shape, want.shape, got.dtype, want.dtype)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    where = np.flatnonzero(bad.ravel())
    return None if where.size == 0 else int(where[0])


def negative_zeros(a):
    a = np.asarray(a)
    return (a == 0) & np.signbit(a)


def subnormal(a):
    a = np.asarray(a)
    return (a != 0) & (np.abs(a) < np.finfo(F32).tiny)
