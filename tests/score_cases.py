"""Enumerated inputs for the scoring sweeps (csrc/assign_kernels.hip: score_sweep_kernel, score_coded_kernel, chain_cand_kernel /
chain_walk_kernel, parts_exact_kernel, assign_kernel, loglike_site_kernel), built for what the generated matrices, the AMRE files and
edge.npz never reach: a likelihood sum s = (like0 + like1) + like2 (glassy_cy.pyx:18-21, float32 in the reference's rounding sequence)
that is +inf, negative, a subnormal of either sign or finite above 1, each at a chosen lane, tile, slab column, pair and quad.  One
term of the operation is v = (float)log((double)s); it depends on a likelihood pair (g0, g1) and a frequency a, and the cell
(individual i, population k) is the set of terms v(pair[site, i], a[site, k]) over the sites.  NumPy only; the twin of
tests/em_cases.py and tests/fisher_cases.py.

THE LAYOUT.  Every individual rotates through one PAIR FAMILY and every population through one FREQUENCY FAMILY:
    individual i, term site t     PAIR_FAMILIES[family of i][(t + r) % its length]            one step per site
    population k, term site t     FREQ_FAMILIES[family of k][(t // STEP + r) % its length]    one step per STEP sites
with r the number of earlier individuals (populations) of the same family, so that no two of a family walk in step.
STEP is no shorter than the longest pair family and there are more runs of STEP sites than the longest frequency family has members, so
every pair of an individual's family meets every frequency of a population's family (family_products() counts it; rotating both by
a multiple of the site number silently drops products).  The individuals interleave over the population slabs SLABS in file order.

THE SHAPES.  `grid`: M_GRID = 197 sites, three tiles and a ragged fourth, every site a term site.  `block`: M_BLOCK = 4096 + 64 + 5
sites -- one block of 64 tiles, a full tile and a ragged one in the second block -- for the coded sweep's parts, block_prefix_kernel
and the chains' block functions; its term sites are the first and the last tile of the first block, both tiles of the second, and of
every other tile lane 0 and the last sixteen lanes (the last 16-, 8- and 4-SNP batch of a part, wherever the parts are cut); all
other sites hold the neutral term (1, 0) at a = 0, which is exactly 0.  `ragged`: the grid's 197 sites with terms in the five sites of
the ragged tile ONLY.  A cell's sum is poisoned by its first non-finite term, and in `grid` and `block` every cell that has one has
it in every tile: a sweep that lost the special values of one tile alone would still return the right sums.  Here the ragged tile is
the only one that has any.

WHY THE FAMILIES ARE CUT AS THEY ARE.  The float64 sum of a finite cell must be exact in any order (exact_sum_margin): a term of
2^-24 next to hundreds of ordinary ones is not.  A term is that small only where the likelihood is within 2^-23 of 1: (1, 0) and
(1 - 2^-24, 2^-24) at a frequency below 2^-12, (0, 0) at one above 1 - 2^-12.  So the hard calls stand in families of their own
(`edge0`, `edge1`, `edge2`) next to their near-edge twin only, and the near-edge frequencies in `near0`, `near1` and `over1`."""
import math

import numpy as np

import synth
from fisher_cases import F32, first_difference, ids_for, interleave, same_nan  # noqa: F401  (what the tests share)

INF, NAN = float("inf"), float("nan")
VARIANTS = ("finite", "hostile")
SHAPES = ("grid", "block")
RAGGED = "ragged"                 # a third shape, for one place only (see THE SHAPES)

PAIR_FAMILIES = {
    # valid likelihoods -------------------------------------------------------------------------------------------------------------
    "edge0": ((1, 0), (1 - 2.0 ** -24, 2.0 ** -24)),                      # the hard call towards g0 and its near-edge twin
    "edge1": ((0, 1), (2.0 ** -24, 1 - 2.0 ** -24)),
    "edge2": ((0, 0), (0.000999, 0.000999)),                                # (a twin nearer (0, 0) has s within 2^-23 of 1 at a = -1, next to ordinary terms)
    "near": ((0.999, 0.001), (0.001, 0.999), (0.000999, 0.000999), (0.941176, 0.058824), (0.799840, 0.199960)),       # near-hard, six digits
    "mid": ((0.333333, 0.333333), (0.5, 0.5), (0.25, 0.5), (0.000999, 0.666445), (0.123456, 0.654321), (0.666667, 0.333334), (0.57735, 0.31831)),
    # likelihoods with little weight on the heterozygote: positive at every negative frequency but (0.5, 0.5) at a = -1, where
    # like0 = 2, like1 = -2, like2 = 0 cancel to s = +0 exactly -- the family whose cells keep -inf as their only non-finite class there
    "half": ((0.5, 0.5), (0.25, 0.25), (0.5, 0.25), (0.75, 0.125)),
    # hostile -----------------------------------------------------------------------------------------------------------------------
    # subnormals of both signs, -0.0.  s is subnormal only for a subnormal g0 next to g1 = 0 at a frequency whose square underflows (six
    # of the eight of `near0h`); in this order any four neighbours (the family's four individuals at one site) hold a positive and a
    # negative one
    "tiny": ((1e-40, 0), (-1e-40, 0), (-0.0, 0.0), (1e-45, 0), (-1e-45, 0), (0, 1e-40), (0, -1e-40)),
    "over": ((0.75, 0.75), (1.5, 0), (0, 2), (0.6, 0.6), (1e-30, 1e-30), (0.0, -0.0)),       # sums above 1: g2 < 0 (NaN at a = 1, so the two guests never make a finite cell inexact)
    "neg": ((-0.25, 0.5), (0.5, -0.25), (-1, -1), (0.25, 0.5)),
    "big": ((1e20, 0), (3e38, 3e38), (0, 3e38), (-3e38, 0), (0.5, 0.5)),  # 3e38 doubled: like0 + like1 overflows as a float32 sum
    # 3e38 alone: the double-to-float conversion of like0 overflows where 1 - a > 1.07.  s is about g0 (1 - 2a): finite above 1 at a
    # frequency below 1/2, +inf at a negative one -- the family whose cells keep +inf as their only non-finite class
    "pinf": ((3e38, 0), (1e20, 0), (3.2e38, 0), (2e38, 0)),
    "infnan": ((INF, 0), (0, INF), (-INF, 0), (INF, -INF), (NAN, 0), (0, NAN), (0.5, 0.5)),
}
FREQ_FAMILIES = {
    # inside [0, 1] -----------------------------------------------------------------------------------------------------------------
    "mid": (0.5, 0.25, 0.1, 0.9, 0.333333, 0.05, 0.75),
    "low": (0.25, 0.1, 0.05, 0.333333, 1 / 86, 0.4),                       # all below 1/2: the cells of `pinf` are finite and positive
    "clamp": (1 / 4, 3 / 4, 1 / 86, 1 - 1 / 86, 1 / 4002, 1 - 1 / 4002),   # 1 / (2 (n + 1)) and its complement for n = 1, 42, 2000
    "near0": (0.0, 2.0 ** -24, 2.0 ** -12, 1e-30, 1e-40),
    "near1": (1.0, 1 - 2.0 ** -24, 1 - 2.0 ** -12),
    "ends": (0.0, 1.0, 0.5, 0.25),
    # hostile -----------------------------------------------------------------------------------------------------------------------
    "near0h": (0.0, 2.0 ** -24, 1e-30, 1e-40, 2.0 ** -12, -0.0, -1e-40, -1e-30),      # near0 and its negative twins (a negative subnormal among them)
    "negs": (-0.25, -1.0, 0.25, -0.5, 0.1),                                # (none at or above 1/2: the cells of `pinf` are +inf only; -1: those of `half` -inf only)
    "negh": (-0.25, -1.0, 0.25, -0.5, 0.5),                                # ... and with 1/2, where the sums of `pinf` cancel to +0: +inf and -inf in one chain, no NaN
    "huge": (1e20, -1e20, 1.5, 2.0, 0.5),                                  # tiny or zero pairs have like2 = +inf here and nothing else that is not finite
    "over1": (1 + 2.0 ** -23, 1.0, 1 - 2.0 ** -24),
    "infnan": (INF, -INF, NAN, 3e38, 0.5, 0.9),
}
# the family of individual i is IND_CYCLE[variant][i % its length]; of population k, POP_ORDER[variant][k]
IND_CYCLE = {
    "finite": ("mid", "edge0", "near", "edge2", "half", "edge1", "near"),
    "hostile": ("tiny", "pinf", "edge2", "near", "mid", "half", "edge0", "pinf", "half", "over", "near", "mid", "pinf", "neg", "half", "edge1",
                "big", "mid", "pinf", "infnan", "tiny", "edge0", "pinf", "half", "edge2", "near"),
}
K_ALL = 23
# (the hostile families stand at 0, 12 and 22 among others: the last population of K = 1, 13 and 23, which the padded slots of a
# register batch repeat)
POP_ORDER = {
    "hostile": ("negs", "low", "mid", "near0h", "low", "near1", "clamp", "low", "huge", "low", "ends", "near0h", "negh", "low", "clamp", "low",
                "huge", "negs", "over1", "low", "near0h", "clamp", "infnan"),
}
POP_ORDER["finite"] = tuple({"negs": "near0", "negh": "near0", "huge": "clamp", "over1": "near1", "infnan": "ends", "near0h": "near0"}.get(f, f) for f in POP_ORDER["hostile"])
assert len(POP_ORDER["hostile"]) == K_ALL

SLABS = (1, 2, 5, 8, 9, 11, 16)   # seven population slabs, odd and even: a pair of the wave and a quad straddle their ends
STEP = 7                          # sites per step of a population's rotation: the longest pair family
M_GRID = 3 * 64 + 5               # the smallest shape that has a full tile behind the first, a tile before the last, and a ragged one
M_BLOCK = 4096 + 64 + 5           # ... and the smallest that has a block edge, a full tile and a ragged one behind it
NEUTRAL_PAIR, NEUTRAL_FREQ = (1.0, 0.0), 0.0

S_CLASSES = ("positive normal <= 1", "finite > 1", "positive subnormal", "+0", "-0", "negative subnormal", "negative normal", "+inf", "-inf", "NaN")
CELL_KINDS = ("finite", "-inf only", "+inf only", "NaN only", "mixed")


def term_sites(shape):
    """(m, the term sites in order) of a shape."""
    assert shape in SHAPES + (RAGGED,)
    if shape == "grid":
        return M_GRID, np.arange(M_GRID)
    if shape == RAGGED:
        return M_GRID, np.arange(M_GRID - M_GRID % 64, M_GRID)
    s = np.arange(M_BLOCK)
    tile, lane = s // 64, s % 64
    return M_BLOCK, np.flatnonzero(np.isin(tile, (0, 63, 64, 65)) | (lane == 0) | (lane >= 48))


def extra_pairs(count):
    """`count` distinct ordinary six-digit pairs (an extra slab that raises the classes per SNP, see build)."""
    j = np.arange(count)
    return np.stack([np.round(0.11 + 0.0071 * j, 6), np.round(0.23 + 0.0053 * j, 6)], axis=1).astype(F32)


def build(variant, shape="grid", extra=0, extra_at=None):
    """dict(variant, shape, L (m, 2n), A (m, K_ALL), labels (n,), sizes, col_of (n,), pair_family (n,) names, freq_family (K_ALL,) names,
    pair_index (m, n), freq_index (m, K_ALL) (-1 at the neutral sites), t_of (m,) rank among the term sites or -1, IDs).
    extra: that many more individuals in a slab of their own behind the others, each with an ordinary pair of its own -- at every site,
    or at the sites `extra_at` only (elsewhere they share one pair): what pushes the classes per SNP over a table of the coded sweep,
    or over the encoder's tables at chosen SNPs, which it then leaves uncoded."""
    assert variant in VARIANTS
    m, sites = term_sites(shape)
    labels = interleave(SLABS)
    n0 = len(labels)
    if extra:
        labels = np.concatenate((labels, np.full(extra, len(SLABS), dtype=labels.dtype)))
    n = len(labels)
    sizes = SLABS + ((extra,) if extra else ())
    col_of = np.array([int((labels[:i] == labels[i]).sum()) for i in range(n)])
    t_of = np.full(m, -1, dtype=np.int64)
    t_of[sites] = np.arange(len(sites))
    live = t_of >= 0
    cycle, order = IND_CYCLE[variant], POP_ORDER[variant]
    pair_family = [cycle[i % len(cycle)] for i in range(n0)] + ["extra"] * extra
    L = np.empty((m, 2 * n), dtype=F32)
    L[:, 0::2], L[:, 1::2] = NEUTRAL_PAIR
    A = np.full((m, K_ALL), NEUTRAL_FREQ, dtype=F32)
    pair_index = np.full((m, n), -1, dtype=np.int64)
    freq_index = np.full((m, K_ALL), -1, dtype=np.int64)
    for i in range(n0):
        fam = np.array(PAIR_FAMILIES[pair_family[i]], dtype=np.float64).astype(F32)
        pair_index[live, i] = (t_of[live] + pair_family[:i].count(pair_family[i])) % len(fam)
        L[live, 2 * i], L[live, 2 * i + 1] = fam[pair_index[live, i], 0], fam[pair_index[live, i], 1]
    for k in range(K_ALL):
        fam = np.array(FREQ_FAMILIES[order[k]], dtype=np.float64).astype(F32)
        freq_index[live, k] = (t_of[live] // STEP + list(order[:k]).count(order[k])) % len(fam)
        A[live, k] = fam[freq_index[live, k]]
    if extra:
        own = extra_pairs(extra)
        at = np.ones(m, dtype=bool) if extra_at is None else np.isin(np.arange(m), extra_at)
        for j in range(extra):
            L[:, 2 * (n0 + j)], L[:, 2 * (n0 + j) + 1] = np.where(at, own[j, 0], own[0, 0]), np.where(at, own[j, 1], own[0, 1])
    return dict(variant=variant, shape=shape, L=L, A=A, labels=labels, sizes=sizes, col_of=col_of, pair_family=pair_family, freq_family=list(order),
                pair_index=pair_index, freq_index=freq_index, t_of=t_of, IDs=ids_for(labels), n_grid=n0)


def family_products(case):
    """{(pair family, frequency family): (products met, products there are)} over the (individual, population) cells of a case, each
    cell counted on its own: the least covered cell of the two families."""
    out = {}
    live = case["t_of"] >= 0
    for i in range(case["n_grid"]):
        np_ = len(PAIR_FAMILIES[case["pair_family"][i]])
        for k in range(K_ALL):
            nf = len(FREQ_FAMILIES[case["freq_family"][k]])
            met = len(set((case["pair_index"][live, i] * nf + case["freq_index"][live, k]).tolist()))
            key = (case["pair_family"][i], case["freq_family"][k])
            out[key] = (min(met, out.get(key, (met, 0))[0]), np_ * nf)
    return out


# ---- the terms -----------------------------------------------------------------------------------------------------------------------
def like_sum(g0, g1, a):
    """s = (like0 + like1) + like2 of glassy_cy.pyx:18-20 for float32 g0, g1, a (broadcast): the products in double, each likelihood
    rounded to float32, the two additions in float32."""
    with np.errstate(all="ignore"):
        g0d, g1d, ad = (np.asarray(x, dtype=F32).astype(np.float64) for x in (g0, g1, a))
        oma = 1.0 - ad
        like0 = ((g0d * oma) * oma).astype(F32)
        like1 = (((g1d * 2.0) * oma) * ad).astype(F32)
        like2 = ((((1.0 - g0d) - g1d) * ad) * ad).astype(F32)
        return ((like0 + like1).astype(F32) + like2).astype(F32)


def classify(s):
    """The number in S_CLASSES of every float32 sum."""
    s = np.asarray(s, dtype=F32)
    tiny = np.finfo(F32).tiny
    with np.errstate(all="ignore"):
        conds = [np.isfinite(s) & (s >= tiny) & (s <= 1), np.isfinite(s) & (s > 1), (s > 0) & (s < tiny), (s == 0) & ~np.signbit(s),
                 (s == 0) & np.signbit(s), (s < 0) & (s > -tiny), np.isfinite(s) & (s <= -tiny), np.isposinf(s), np.isneginf(s), np.isnan(s)]
    out = np.full(s.shape, -1, dtype=np.int8)
    for c, cond in enumerate(conds):
        out[cond] = c
    assert (out >= 0).all()
    return out


def sums_of(case, pops=None):
    """(m, n, K) float32: s of every (site, individual, population)."""
    A = case["A"] if pops is None else case["A"][:, pops]
    return like_sum(case["L"][:, 0::2, None], case["L"][:, 1::2, None], A[:, None, :])


def class_counts(case):
    """{class name: terms} over the term sites of a case's own individuals: the classes the operation REACHES on these inputs (computed,
    not claimed -- a class with a count of 0 is unreachable from them)."""
    cls = classify(sums_of(case))[case["t_of"] >= 0][:, :case["n_grid"]]
    return {name: int((cls == c).sum()) for c, name in enumerate(S_CLASSES)}


def reachable(variant):
    """The numbers of the classes of s that the `grid` case of a variant holds at all."""
    counts = class_counts(case_of(variant, "grid"))
    return [c for c, name in enumerate(S_CLASSES) if counts[name] > 0]


def places(case, site, i):
    """Where (site, individual) stands for the kernels: tile, lane, block, the slab and its column, the half of the wave's pair and the
    column of the coded sweep's quad, and whether the site ends a 16-, 8- or 4-SNP batch of a coded part (any split: the last batch
    of a tile; the ragged tile's last batch)."""
    m = case["L"].shape[0]
    tile, lane, col = site // 64, site % 64, int(case["col_of"][i])
    last_tile = tile == (m - 1) // 64
    end = (m - tile * 64) if last_tile else 64                     # live lanes of the tile
    batch = {b: lane >= ((end - 1) // b) * b for b in (16, 8, 4)}
    return dict(tile=tile, lane=lane, block=tile // 64, tile_in_block=tile % 64, slab=int(case["labels"][i]), col=col, half=col % 2, quad_col=col % 4,
                last_live_lane=bool(last_tile and lane == end - 1), last_batch=batch)


def describe(case, i, k, site, pops=None):
    """The term of (individual i, population k, site) for a failure message: pair, frequency, class of s, place.  pops: the columns of
    A the K populations of the comparison stand for (per individual: pops[i])."""
    col = k if pops is None else int(np.asarray(pops)[i][k] if np.ndim(pops) == 2 else pops[k])
    g0, g1, a = case["L"][site, 2 * i], case["L"][site, 2 * i + 1], case["A"][site, col]
    s = like_sum(g0, g1, a)
    p = places(case, site, i)
    return "individual %d (%s, slab %d of %d, column %d: half %d of its pair, column %d of its quad), population %d (column %d, %s), site %d (tile %d, lane %d%s): pair (%r, %r) at a = %r, s = %r [%s]" % (
        i, case["pair_family"][i], p["slab"], case["sizes"][p["slab"]], p["col"], p["half"], p["quad_col"], k, col, case["freq_family"][col], site, p["tile"],
        p["lane"], ", neutral" if case["t_of"][site] < 0 else "", float(g0), float(g1), float(a), float(s), S_CLASSES[int(classify(s))])


# ---- what the reference makes of them ------------------------------------------------------------------------------------------------
_cases, _reference = {}, {}


def case_of(variant, shape="grid"):
    key = (variant, shape)
    if key not in _cases:
        c = build(variant, shape)
        for a in (c["L"], c["A"]):
            a.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def per_site(orc, L, A, threads=4):
    """(n, K, m) float32: glassy_cy.loglike into zeros for every (individual, population) -- the per-site values v."""
    m, n, K = L.shape[0], L.shape[1] // 2, A.shape[1]
    L, A = np.ascontiguousarray(L, dtype=F32), np.ascontiguousarray(A, dtype=F32)
    V = np.zeros((n, K, m), dtype=F32)
    with np.errstate(all="ignore"):
        for i in range(n):
            for k in range(K):
                orc.loglike(L, A, V[i, k], threads, i, k)
    return V


def reference(orc, variant, shape="grid"):
    """(case, V (n, K_ALL, m) float32): the oracle's per-site values.  Computed once, shared, read-only."""
    key = (variant, shape)
    if key not in _reference:
        c = case_of(variant, shape)
        V = per_site(orc, c["L"], c["A"])
        V.setflags(write=False)
        _reference[key] = (c, V)
    return _reference[key]


def permutation(i, K=K_ALL):
    """The columns of A that individual i's K populations point at in the per-individual tests: a permutation of its own (K_ALL is
    prime: every stride walks through all columns)."""
    return (i + np.arange(K) * (1 + i % (K_ALL - 1))) % K_ALL


def cell_kinds(V):
    """(..., ) int8 over the leading axes of V (..., m): the number in CELL_KINDS of every cell -- finite; -inf, +inf or NaN the ONLY
    non-finite class among its terms; mixed."""
    ninf, pinf, nan = np.isneginf(V).any(axis=-1), np.isposinf(V).any(axis=-1), np.isnan(V).any(axis=-1)
    count = ninf.astype(int) + pinf + nan
    return np.where(count == 0, 0, np.where(count > 1, 4, np.where(ninf, 1, np.where(pinf, 2, 3)))).astype(np.int8)


def exact_sum_margin(v):
    """For the finite float32 terms v of one cell: (sum |v|, 2^53 u) with u the ulp of the smallest non-zero |v|.  sum |v| < 2^53 u is
    sufficient for the float64 sum to be exact in ANY order: every partial sum is a multiple of u below 2^53 u."""
    mag = np.abs(np.asarray(v, dtype=np.float64))
    nz = mag[mag != 0]
    if nz.size == 0:
        return 0.0, math.inf
    u = 2.0 ** (math.frexp(float(nz.min()))[1] - 24)
    return float(math.fsum(nz)), 2.0 ** 53 * u


def expected_sums(V):
    """(...) float64: what np.sum(vec, dtype=float) of glassy.py:38 gives for every cell of V (..., m) -- math.fsum of the float32 values
    where they are all finite (exact in any order, see exact_sum_margin), else -inf, +inf or NaN by the classes present."""
    kinds = cell_kinds(V)
    out = np.empty(kinds.shape, dtype=np.float64)
    for idx in np.ndindex(kinds.shape):
        kind = kinds[idx]
        out[idx] = math.fsum(V[idx].astype(np.float64)) if kind == 0 else (-math.inf if kind == 1 else math.inf if kind == 2 else math.nan)
    return out


def partition_sums(V, P, site0=0, carry=None):
    """(n * P, K) float32: utils.py:147-149 for every cell of V (n, K, m) -- labels (site0 + s) % P, serial float32 np.add.at from
    zeros or from `carry`."""
    n, K, m = V.shape
    labels = (site0 + np.arange(m)) % P
    out = np.zeros((n * P, K), dtype=F32) if carry is None else np.array(carry, dtype=F32)
    with np.errstate(all="ignore"):
        for i in range(n):
            for k in range(K):
                pr = out[i * P:(i + 1) * P, k].copy()
                np.add.at(pr, labels, V[i, k])
                out[i * P:(i + 1) * P, k] = pr
    return out


def classes_per_snp(L):
    """(m,) the distinct (g0, g1) bit patterns of every site: what the class encoder counts."""
    bits = np.ascontiguousarray(L, dtype=F32).view(np.uint64)
    return np.array([len(np.unique(row)) for row in bits])


def table_snps(L):
    """SNPs per table of the coded sweep for a matrix (codes.hip: wgs_beagle_codes_plan): 16 while 16 x the 99th percentile of the
    classes per SNP -- the smallest count with 99 % of the SNPs at or below it -- stays within 616 rows, else 8, else 4."""
    g99 = int(np.percentile(classes_per_snp(L), 99, method="inverted_cdf"))
    return 16 if g99 * 16 <= 616 else (8 if g99 * 8 <= 616 else 4)


def digest(case):
    return synth.digest(np.concatenate((case["L"].ravel().view(np.uint32), case["A"].ravel().view(np.uint32))))


def same_bits64(got, want):
    """float64 arrays: the same bits where the reference is not NaN, NaN exactly where it is."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return got[ok].tobytes() == want[ok].tobytes()


def first_difference_any(got, want):
    """first_difference for any float dtype: None, or the flat index of the first value that is not the reference's."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    u = np.uint32 if got.dtype == F32 else np.uint64
    bad = (got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want))
    where = np.flatnonzero(bad.ravel())
    return None if where.size == 0 else int(where[0])


# ---- the record of the real reference --------------------------------------------------------------------------------------------------
# tests/golden/score_cases.npz (make_golden_score_cases.py): the `grid` case of both variants on one individual of every pair family
# and one population of every frequency family (all of them would be 1.9 MB)
GOLDEN_INDIVIDUALS = {"finite": (0, 1, 2, 3, 4, 5, 6), "hostile": (0, 1, 2, 3, 4, 5, 6, 9, 13, 15, 16, 19)}
GOLDEN_POPULATIONS = (0, 1, 2, 3, 5, 6, 8, 10, 18, 22, 12)
GOLDEN_PARTS = (1, 3, 64)
GOLDEN_STARTS = (-1.5, -INF, 3e38, NAN, 0.0, INF, -3e38, 1e-3)     # loglike into a non-zero vector: vec[s] = STARTS[s % 8] (ordinary, -inf, huge, NaN ...)
GOLDEN_START_CELLS = ((0, 0), (1, 0), (2, 1), (4, 2), (6, 3), (3, 4), (5, 6), (1, 8), (2, 9), (6, 7))      # (number among the individuals, among the populations)
GOLDEN = {v: dict(variant=v, shape="grid", individuals=GOLDEN_INDIVIDUALS[v], populations=GOLDEN_POPULATIONS) for v in VARIANTS}


def golden_inputs(variant):
    """(case, L of the recorded individuals, A of the recorded populations, the start vector of the accumulating runs)."""
    c = case_of(variant, "grid")
    inds = np.array(GOLDEN_INDIVIDUALS[variant])
    L = np.empty((c["L"].shape[0], 2 * len(inds)), dtype=F32)
    L[:, 0::2], L[:, 1::2] = c["L"][:, 2 * inds], c["L"][:, 2 * inds + 1]
    A = np.ascontiguousarray(c["A"][:, list(GOLDEN_POPULATIONS)])
    start = np.array(GOLDEN_STARTS, dtype=np.float64).astype(F32)[np.arange(L.shape[0]) % len(GOLDEN_STARTS)]
    return c, L, A, start


def golden_record(loglike, partition_loglikes, variant):
    """What tests/golden/score_cases.npz holds of a variant besides glassy.assignLL, from `loglike` (glassy_cy.loglike of the reference,
    or the oracle's) and `partition_loglikes` (utils.partition_loglikes, or the oracle's): dict(loglike (n, K, m) float32 per-site
    values, started (cells, m) the same accumulated into the start vector, parts_P (n * P, K) float32)."""
    c, L, A, start = golden_inputs(variant)
    n, K, m = L.shape[1] // 2, A.shape[1], L.shape[0]
    V = np.zeros((n, K, m), dtype=F32)
    with np.errstate(all="ignore"):
        for i in range(n):
            for k in range(K):
                loglike(L, A, V[i, k], 1, i, k)
        started = np.stack([start.copy() for _ in GOLDEN_START_CELLS])
        for row, (i, k) in zip(started, GOLDEN_START_CELLS):
            loglike(L, A, row, 1, i, k)
        out = dict(loglike=V, started=started)
        for P in GOLDEN_PARTS:
            parts = np.zeros((n * P, K), dtype=F32)
            for i in range(n):
                for k in range(K):
                    parts[i * P:(i + 1) * P, k] = partition_loglikes(V[i, k], P)
            out["parts_%d" % P] = parts
    return out


# the sites whose extra individuals push them over the class encoder's tables (build(extra_at=...)): the first and the last site, lanes
# 63 and 0 of neighbouring tiles, the last 16-, 8- and 4-SNP batch of a tile, sites inside a tile, and in the block case both sides of
# the block edge
UNCODED_SITES = {"grid": (0, 5, 38, 63, 64, 100, 115, 120, 127, 150, 194, 196), "block": (0, 5, 38, 63, 64, 115, 127, 4095, 4096, 4100, 4164)}


def uncoded_sites(shape="grid"):
    return np.array(UNCODED_SITES[shape])
