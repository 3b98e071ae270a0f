"""Enumerated terms for the per-site z-score statistic (csrc/zscore_kernels.hip: zstat_kernel with zs_loops<6> out of the LDS table
and zs_loops<WGS_Z_DEEP_ROW> out of the deep rows, zs_logf's special branch, the deep branch of zmask_kernel), which restates
zscore_cy.pyx:10-57.  The generated cases and tests/zscore_cases.py give it frequencies strictly inside the clamp, six-digit
likelihoods next to their class mean and binomial tables; here every special value of the operation is placed on purpose.  NumPy
only; the twin of tests/fisher_cases.py, tests/em_cases.py and tests/score_cases.py, whose pair lists it draws from.

A TERM is (pair (g0, g1), frequency A, depth dl, the individual's table).  The device forms no sum across sites -- the host sums
the compacted arrays -- so every kept site is a term compared on its own: nothing is poisoned by a neighbour, nothing is left out.
The mask sweep is fed directly (a class whose mean is NaN keeps every one of its sites: !(|NaN - v| > 0.01)), so any likelihood pair
reaches the statistic.  Every builder is deterministic and returns its inputs next to the claims they are built for;
tests/test_zstat_cases_cpu.py holds them to those claims on the restatement (tests/zscore_cpu.py) and the restatement to the record of
the real reference (tests/golden/zstat_cases.npz), tests/test_gpu_zstat_cases.py runs them through the library."""
from fractions import Fraction

import numpy as np

import em_cases
import fisher_cases
import score_cases
import synth_deep
import synth_depth
import zscore_cases
import zscore_cpu

F32 = np.float32
F64 = np.float64
INF, NAN = float("inf"), float("nan")
N_CLASSES, MAX_DENSE, DEEP_MAX, DEEP_ROW = 253, 21, 510, 8
TINY = np.finfo(F32).tiny

# ---- the terms -----------------------------------------------------------------------------------------------------------------------
# Likelihood pairs, every one of them out of score_cases.PAIR_FAMILIES, fisher_cases.PAIRS or em_cases.PAIRS_ADDED (POOL): the hard
# calls and their near-edge twins, ordinary six-digit pairs (one summing above 1), subnormals of both signs and signed zeros, sums
# above 1, negative entries, 3e38 twice, infinite entries, NaN entries.  (-0.0, 1.0000001) is the only way to s_obs = -0.0 (at
# A = -0.0: g0 P0 = -0, g1 P1 = -0 and (1 - g0 - g1) P2 = -1.2e-7 * +0 = -0).
ORDINARY_PAIRS = ((0.333333, 0.333333), (0.666667, 0.333334), (0.941176, 0.058824))
PAIRS = ((1, 0), (0, 1), (0, 0), (1 - 2.0 ** -24, 2.0 ** -24), (2.0 ** -24, 1 - 2.0 ** -24)) + ORDINARY_PAIRS + (
    (1e-40, 0), (-1e-40, 0), (0, 1e-40), (-0.0, 0.0), (-0.0, 1.0000001), (0.75, 0.75), (1.5, 0), (-0.25, 0.5), (0.5, -0.25),
    (3e38, 3e38), (INF, 0), (-INF, 0), (NAN, 0), (0, NAN))
POOL = tuple(p for fam in score_cases.PAIR_FAMILIES.values() for p in fam) + tuple(fisher_cases.PAIRS) + tuple(em_cases.PAIRS_ADDED)


def clamp_bounds(n_pop):
    """(lo, 1 - lo) as zscore_cpu.clamp stores them into a float32 vector."""
    f = zscore_cpu.clamp(np.array([-1.0, 2.0], dtype=F32), n_pop)
    return float(f[0]), float(f[1])


# Frequencies: the ends and the smallest subnormal and normal, ordinary ones, the ties of 1 - A and (1 - A)^2 between float32 and
# float64 (2^-24, 2^-25, 3 2^-25, 1 - 2^-24, 1 - 2^-23), the clamp bounds of populations of 2, 16 and 84 with their complements, and
# what lies outside the domain: 2.0, -0.25, 1.5e19 (P1 alone overflows to -inf), 1e20 (P0 = +inf, P1 = -inf), +inf, NaN.
CLAMPS = tuple(v for n_pop in (2, 16, 84) for v in clamp_bounds(n_pop))
FREQS = (0.0, -0.0, 1.0, 2.0 ** -149, 2.0 ** -126, 0.5, 1 / 3, 0.999999, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1 - 2.0 ** -24,
         1 - 2.0 ** -23) + CLAMPS + (2.0, -0.25, 1.5e19, 1e20, INF, NAN)
FREQS_FOR_EVERY_PAIR = (0.0, 0.5, 1.0, CLAMPS[4])          # what every hostile table sees every pair at
DENSE_DEPTHS, DEEP_DEPTHS = (0, 1, 2, 8, 21), (22, 23, 40)
DEPTHS = DENSE_DEPTHS + DEEP_DEPTHS
# where the dropped sites live: a dense depth no class of which has a component, a dense and a deep class with a finite mean far from
# the site's value, a deep depth without rows (deep_map = -1)
DROP_DENSE_DEPTH, DROP_DENSE_CLASS, DROP_DEEP_CLASS, DROP_DEEP_DEPTH = 5, (7, 1), (21, 1), 30
DROP_MEAN, DROP_VALUES = 0.25, (1.0, 0.0, INF, -1e30)

# Hostile table rows.  AD_like: the three unit rows and the empty one (lg = -inf next to P = 0: -inf * 0 = NaN), the negative zeros
# (s_exp = -0), negative entries, one whose first two products cancel exactly at A = 0.5 (fused: the whole result), a subnormal
# of either sign (the negative one: the logarithm of a negative subnormal is NaN, which the hardware's own logarithm, taking a
# subnormal for a zero of its sign, does not say), 3e38 twice, +inf, NaN.  AD_factorial (the same value in all three columns): 0,
# -0.0, the smallest subnormal, a negative one, 3e38, +inf, NaN.
HOSTILE_LIKE = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0), (-0.0, -0.0, -0.0), (-0.25, 0.5, 0.75), (0.5, -0.25, 0.75), (1e-40, 0, 0),
                (-1e-40, 0, 0), (3e38, 3e38, 0), (INF, 0.5, 0.25), (0.5, NAN, 0.25))
HOSTILE_FAC = (0.0, -0.0, 1e-45, -0.5, 3e38, INF, NAN)
HOSTILE = tuple(("like", r) for r in HOSTILE_LIKE) + tuple(("fac", (v, v, v)) for v in HOSTILE_FAC)
N_VARIANTS = len(HOSTILE)                                  # hostile tables: variant v = 1 .. N_VARIANTS; variant 0 is wholly ordinary

M = 4096 + 64 + 5           # one full block of ZS_TILES_PER_BLOCK = 64 tiles, then a full and a ragged tile in the second block
ROW0 = {d: int(sum(e + 1 for e in DEPTHS if e < d)) for d in DEPTHS}       # first table row of depth d; row of (d, a) = ROW0[d] + a
N_ROWS = sum(d + 1 for d in DEPTHS)
N_DEEP_ROWS = sum(d + 1 for d in DEEP_DEPTHS)
N_SLABS = 5
STRIDE = 1237               # prime, not a factor of the product's size: neighbouring slots hold unrelated terms


def f32(values):
    with np.errstate(over="ignore"):
        return np.array(values, dtype=F64).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def pool_holds(pair):
    want = bits(f32(pair)).tolist()
    return any(bits(f32(p)).tolist() == want for p in POOL)


def term_sites():
    """The first and the last tile of the first block, both tiles of the second block, lanes 0 and 63 of every other tile."""
    s = list(range(64)) + [64 * t + lane for t in range(1, 63) for lane in (0, 63)] + list(range(63 * 64, M))
    return np.array(sorted(s), dtype=np.int64)


def placements(v):
    """Hostile table v (1 ..): [(depth, step a, index into HOSTILE)], one per depth.  Over the variants every hostile row stands at
    a = 0 (depths 2 and 22), at a middle step (8 and 23) and at a = dl (21 and 40): once through the LDS table, once through the deep
    rows; depth 0 has its one step, depth 1 its two in turn."""
    h = lambda k: (v - 1 + k) % N_VARIANTS
    return [(22, 0, h(0)), (23, 11, h(1)), (40, 40, h(2)), (2, 0, h(3)), (8, 4, h(4)), (21, 21, h(5)), (0, 0, h(6)), (1, v % 2, h(7))]


def ordinary_table():
    """(fac, like, index): zscore_cpu.tables of the class means of synth_deep.class_triple for every class of DEPTHS, the index
    written as the reference READS it: index[a, dl - a] is the row of class (Ar = dl - a, Aa = a)."""
    arr = np.array([(d - a, a, d, 1) for d in DEPTHS for a in range(d + 1)], dtype=np.int32)
    g0, g1 = (x.astype(F32) for x in synth_deep.class_triple(arr[:, 0], arr[:, 1]))
    means = np.stack((g0, g1, (F32(1) - g0) - g1), axis=1)
    fac, like, index = zscore_cpu.tables(arr, arr[:, :2], means)
    index = np.ascontiguousarray(index.T)
    assert index.shape == (41, 41) and all(index[a, d - a] == ROW0[d] + a for d in DEPTHS for a in range(d + 1))
    return fac, like, index


def tables_of(variant):
    fac, like, index = ordinary_table()
    if variant:
        for d, a, h in placements(variant):
            kind, row = HOSTILE[h]
            (like if kind == "like" else fac)[ROW0[d] + a] = f32(row)
    return fac, like, index


def product_terms():
    return [(p, f, d) for d in range(len(DEPTHS)) for f in range(len(FREQS)) for p in range(len(PAIRS))]


def hostile_terms(v):
    """The slots of a hostile table: every (frequency, depth) with the ordinary pairs in turn, then every pair at
    FREQS_FOR_EVERY_PAIR, depths in turn."""
    ordinary = [PAIRS.index(p) for p in ORDINARY_PAIRS]
    four = [FREQS.index(f) for f in FREQS_FOR_EVERY_PAIR]
    out = [(ordinary[(f + d) % 3], f, d) for f in range(len(FREQS)) for d in range(len(DEPTHS))]
    k = 0
    n_slots = len(term_sites())
    while len(out) < n_slots:
        p, j = (k // 4) % len(PAIRS), k % 4
        out.append((p, four[j], (p + 3 * j + v + 4 * (k // (4 * len(PAIRS)))) % len(DEPTHS)))
        k += 1
    return out


def class_index(Ar, Aa):
    return (Ar + Aa) * (Ar + Aa + 1) // 2 + Aa


def grid():
    """The whole grid: dict of
    L (M, 2n), AD (M, 2n) int32, A (M, n) -- every individual has a frequency column of its own --, group_of (n,): N_SLABS population
    slabs of 7, 7, 7, 6 and 6 individuals, interleaved (both halves of a float4, a last odd column);
    variant (n,): the table of each individual (0: ordinary); fac, like (n, N_ROWS, 3), index (41, 41): what the reference reads;
    key_mean, key_comp (n, 253), deep_map (n, 511) (rows counted per individual), deep_rows (n, N_DEEP_ROWS, 8), tabs (n, 253, 6):
    what the device reads; sites (321,): the term sites, the same for everybody; t_pair, t_freq, t_depth (n, 321): indices into
    PAIRS, FREQS, DEPTHS of the term at each of them.  Every other site is dropped by the mask."""
    pairs, freqs = f32(PAIRS), f32(FREQS)
    sites = term_sites()
    ns = len(sites)
    product = product_terms()
    n_ord = -(-len(product) // ns)
    variant = []
    for k in range(max(N_VARIANTS, n_ord)):
        variant += ([k + 1] if k < N_VARIANTS else []) + ([0] if k < n_ord else [])
    variant = np.array(variant, dtype=np.int32)
    n = len(variant)
    L = np.zeros((M, 2 * n), dtype=F32)
    AD = np.zeros((M, 2 * n), dtype=np.int32)
    A = np.zeros((M, n), dtype=F32)
    t_pair, t_freq, t_depth = (np.zeros((n, ns), dtype=np.int64) for _ in range(3))
    fac, like = np.zeros((n, N_ROWS, 3), dtype=F32), np.zeros((n, N_ROWS, 3), dtype=F32)
    key_mean = np.zeros((n, N_CLASSES), dtype=F32)
    key_comp = np.full((n, N_CLASSES), -1, dtype=np.int32)
    deep_map = np.full((n, DEEP_MAX + 1), -1, dtype=np.int32)
    deep_rows = np.zeros((n, N_DEEP_ROWS, DEEP_ROW), dtype=F32)
    tabs = np.zeros((n, N_CLASSES, 6), dtype=F32)
    is_term = np.zeros(M, dtype=bool)
    is_term[sites] = True
    other = np.flatnonzero(~is_term)
    q = 0
    for i in range(n):
        fac[i], like[i], index = tables_of(int(variant[i]))
        # ---- what the device reads
        for d in DENSE_DEPTHS:
            for a in range(d + 1):
                k = class_index(d - a, a)
                key_mean[i, k], key_comp[i, k] = NAN, (d + a + i) % 3
                tabs[i, k] = np.concatenate((like[i, index[a, d - a]], fac[i, index[a, d - a]]))
        key_mean[i, class_index(*DROP_DENSE_CLASS)], key_comp[i, class_index(*DROP_DENSE_CLASS)] = DROP_MEAN, 0
        at = 0
        for d in DEEP_DEPTHS:
            deep_map[i, d] = at
            for a in range(d + 1):
                r = index[a, d - a]
                deep_rows[i, at + a] = np.concatenate(([(d + a + i) % 3, NAN], like[i, r], fac[i, r]))
            at += d + 1
        deep_rows[i, deep_map[i, sum(DROP_DEEP_CLASS)] + DROP_DEEP_CLASS[1], :2] = (0, DROP_MEAN)
        # ---- the terms
        if variant[i] == 0:
            terms = [product[((q * ns + k) * STRIDE) % len(product)] for k in range(ns)]
            q += 1
        else:
            terms = hostile_terms(int(variant[i]))
        for k, (p, f, d) in enumerate(terms):
            slot = (k + 37 * i) % ns
            t_pair[i, slot], t_freq[i, slot], t_depth[i, slot] = p, f, d
        dl = np.array(DEPTHS)[t_depth[i]]
        aa = (np.arange(ns) * 7 + i) % (dl + 1)
        aa = np.where(np.isin(dl, (sum(DROP_DENSE_CLASS), sum(DROP_DEEP_CLASS))) & (aa == 1), 2, aa)
        L[sites, 2 * i], L[sites, 2 * i + 1] = pairs[t_pair[i], 0], pairs[t_pair[i], 1]
        A[sites, i] = freqs[t_freq[i]]
        AD[sites, 2 * i], AD[sites, 2 * i + 1] = dl - aa, aa
        # ---- the dropped sites: hostile terms among them
        kind = (other + i) % 4
        g = pairs[(other * 5 + i) % len(pairs)]
        g0 = np.where(kind >= 2, f32(DROP_VALUES)[other % 4], g[:, 0])
        L[other, 2 * i], L[other, 2 * i + 1] = g0, g[:, 1]
        A[other, i] = freqs[(other * 3 + i) % len(freqs)]
        Aa = np.select([kind == 0, kind == 1, kind == 2], [other % (DROP_DENSE_DEPTH + 1), other % (DROP_DEEP_DEPTH + 1), DROP_DEEP_CLASS[1]],
                       DROP_DENSE_CLASS[1])
        Dl = np.select([kind == 0, kind == 1, kind == 2], [DROP_DENSE_DEPTH, DROP_DEEP_DEPTH, sum(DROP_DEEP_CLASS)], sum(DROP_DENSE_CLASS))
        AD[other, 2 * i], AD[other, 2 * i + 1] = Dl - Aa, Aa
    return dict(L=L, AD=AD, A=A, group_of=(np.arange(n) % N_SLABS).astype(np.int32), variant=variant, fac=fac, like=like, index=index,
                key_mean=key_mean, key_comp=key_comp, deep_map=deep_map, deep_rows=deep_rows, tabs=tabs, sites=sites, t_pair=t_pair,
                t_freq=t_freq, t_depth=t_depth)


_grid = []


def shared_grid():
    """grid(), built once and read-only."""
    if not _grid:
        g = grid()
        for v in g.values():
            v.setflags(write=False)
        _grid.append(g)
    return _grid[0]


def digest(g):
    return synth_depth.digest(g["L"], g["AD"], g["A"], g["fac"], g["like"], g["index"])


def batch_tables(g, i0, count, deep=True):
    """(key_mean, key_comp, deep_map, deep_rows) of the individuals [i0, i0 + count) as wgs_zkeep_create_deep takes them: the rows of
    the batch one after the other, the map counting from the batch's first row.  deep=False: the dense pair alone."""
    rows = slice(i0, i0 + count)
    if not deep:
        return g["key_mean"][rows], g["key_comp"][rows]
    dmap = np.where(g["deep_map"][rows] >= 0, g["deep_map"][rows] + np.arange(count, dtype=np.int32)[:, None] * N_DEEP_ROWS, -1)
    return g["key_mean"][rows], g["key_comp"][rows], dmap, np.ascontiguousarray(g["deep_rows"][rows].reshape(-1, DEEP_ROW))


def describe(g, i, slot):
    """A term in words, for a failure's report."""
    return "individual %d site %d pair %r frequency %r depth %d table variant %d" % (
        i, g["sites"][slot], PAIRS[g["t_pair"][i, slot]], FREQS[g["t_freq"][i, slot]], DEPTHS[g["t_depth"][i, slot]], g["variant"][i])


def restatement(g, slots=None):
    """zscore_cpu.per_site per individual on its term sites (slots: per individual the positions in g["sites"]; None: all):
    three float32 arrays, individual after individual."""
    out = []
    with np.errstate(all="ignore"):
        for i in range(len(g["variant"])):
            keep = g["sites"] if slots is None else g["sites"][slots[i]]
            out.append(zscore_cpu.per_site(g["L"], g["AD"], i, keep, np.ascontiguousarray(g["A"][keep, i]), g["fac"][i], g["like"][i], g["index"]))
    return tuple(np.concatenate([o[c] for o in out]) for c in range(3))


# ---- the statistic once more, term by term, with its intermediate values and its deliberately wrong variants ------------------------
MUTANTS = ("one_minus_a_f32", "g2_f32", "fused", "flush", "untransposed", "running_wl", "log_nan_at_zero", "log_flushes_its_argument")


def flush(x):
    return np.where(np.abs(x) < TINY, np.copysign(F32(0), x), x).astype(F32)


def value_class(x):
    """0 positive normal, 1 positive subnormal, 2 +0, 3 -0, 4 negative normal, 5 +inf, 6 -inf, 7 NaN, 8 negative subnormal."""
    x = np.asarray(x, dtype=F32)
    neg = np.signbit(x)
    return np.select([np.isnan(x), np.isposinf(x), np.isneginf(x), (x == 0) & ~neg, (x == 0) & neg, x <= -TINY, x < 0, x < TINY],
                     [7, 5, 6, 2, 3, 4, 8, 1], 0)


CLASS_NAMES = ("positive normal", "positive subnormal", "+0", "-0", "negative normal", "+inf", "-inf", "NaN", "negative subnormal")


def statistic(g, slots=None, mutant=None, trace=None):
    """W_l_obs, W_l, var_W_l (float32, individual after individual as restatement() returns them) of the grid's terms as tests/zscore_cpu.per_site states them -- the test holds the
    two to each other -- or, with `mutant`, one of the subtly wrong variants of MUTANTS.  trace (a dict) receives s_obs, and per loop
    step the mask of the terms that take it, s_exp, lg, the three products of the first loop and d of the second."""
    assert mutant is None or mutant in MUTANTS
    n, ns = g["t_pair"].shape
    slots = [np.arange(ns)] * n if slots is None else slots
    ind = np.concatenate([np.full(len(x), i, dtype=np.int64) for i, x in enumerate(slots)])
    s = g["sites"][np.concatenate(slots)]
    g0, g1, A = g["L"][s, 2 * ind], g["L"][s, 2 * ind + 1], g["A"][s, ind]
    Dl = (g["AD"][s, 2 * ind] + g["AD"][s, 2 * ind + 1]).astype(np.int64)
    z = flush if mutant == "flush" else (lambda x: x)

    def logf(x):
        lg = zscore_cpu._logf(flush(x) if mutant == "log_flushes_its_argument" else x)       # (a negative subnormal: -inf for NaN)
        return np.where(x == 0, F32(NAN), lg) if mutant == "log_nan_at_zero" else lg
    with np.errstate(all="ignore"):
        Ad = A.astype(F64)
        if mutant == "one_minus_a_f32":
            om = F32(1) - A
            P0, P1 = om * om, (F32(2) * om) * A
        else:
            P0, P1 = ((1.0 - Ad) * (1.0 - Ad)).astype(F32), ((2.0 * (1.0 - Ad)) * Ad).astype(F32)
        P0, P1, P2 = z(P0), z(P1), z(A * A)
        g2 = ((F32(1) - g0) - g1).astype(F64) if mutant == "g2_f32" else (1.0 - g0.astype(F64)) - g1.astype(F64)
        f0, f1, f2 = z(g0 * P0), z(g1 * P1), z((g2 * P2.astype(F64)).astype(F32))
        s_obs = z(z(f0 + f1) + f2)
        wobs = logf(s_obs)
        wl = np.zeros(len(s), dtype=F32)
        var = np.zeros(len(s), dtype=F32)
        steps, running = [], []
        for a in range(int(Dl.max()) + 1):
            on = Dl >= a
            ar = np.where(on, Dl - a, 0)
            r = g["index"][ar, np.where(on, a, 0)] if mutant == "untransposed" else g["index"][np.where(on, a, 0), ar]
            like, fac = g["like"][ind, r], g["fac"][ind, r]
            if mutant == "fused":                       # (the exact product is a double; the sum rounds once more than an fma would)
                first = (like[:, 0].astype(F64) * P0.astype(F64) + (like[:, 1] * P1).astype(F64)).astype(F32)
            else:
                first = z(z(like[:, 0] * P0) + z(like[:, 1] * P1))
            s_exp = z(first + z(like[:, 2] * P2))
            lg = logf(s_exp)
            prods = []
            for c, P in enumerate((P0, P1, P2)):
                prods.append(z(z(lg * P) * fac[:, c]))
                wl = np.where(on, z(wl + prods[-1]), wl)
            steps.append((on, fac, lg, s_exp, prods))
            running.append(wl)
        ds = []
        for a, (on, fac, lg, s_exp, prods) in enumerate(steps):
            d = z((running[a] if mutant == "running_wl" else wl) - lg)
            ds.append(d)
            for c, P in enumerate((P0, P1, P2)):
                var = np.where(on, z(var + z(z(z(d * d) * P) * fac[:, c])), var)
    if trace is not None:
        trace.update(s_obs=s_obs, Dl=Dl, P=(P0, P1, P2), on=[st[0] for st in steps], fac=[st[1] for st in steps], lg=[st[2] for st in steps],
                     s_exp=[st[3] for st in steps], prods=[st[4] for st in steps], d=ds, ind=ind, A=A, g0=g0, g1=g1)
    return wobs, wl, var


def reached(g, slots=None):
    """The claims about value classes, subnormal sums and overflow, counted on the restatement: dict of counts of terms."""
    t = {}
    wobs, wl, var = statistic(g, slots, trace=t)
    Dl = t["Dl"]
    out = {"s_obs " + CLASS_NAMES[c]: int((value_class(t["s_obs"]) == c).sum()) for c in range(len(CLASS_NAMES))}
    where = {"first": lambda a: (Dl >= a) & (a == 0), "middle": lambda a: (Dl > a) & (a > 0), "last": lambda a: (Dl == a) & (a > 0)}
    for name, at in where.items():
        for c in range(len(CLASS_NAMES)):
            out["s_exp %s at a %s step" % (CLASS_NAMES[c], name)] = int(sum(((value_class(s) == c) & at(a)).sum() for a, s in enumerate(t["s_exp"])))
    for name, x in (("W_l", wl), ("var_W_l", var)):
        out[name + " finite"], out[name + " NaN"] = int(np.isfinite(x).sum()), int(np.isnan(x).sum())
        out[name + " +inf"], out[name + " -inf"] = int(np.isposinf(x).sum()), int(np.isneginf(x).sum())
    with np.errstate(all="ignore"):
        inf_zero = np.zeros(len(Dl), dtype=bool)
        for on, lg in zip(t["on"], t["lg"]):
            inf_zero |= on & np.isneginf(lg) & ((t["P"][0] == 0) | (t["P"][1] == 0) | (t["P"][2] == 0))
        out["a product -inf * 0"] = int(inf_zero.sum())
        # sums that are subnormal from the first product to the last: flushing any of them changes the bits
        small_wl, small_var, over = np.ones(len(Dl), dtype=bool), np.ones(len(Dl), dtype=bool), np.zeros(len(Dl), dtype=bool)
        for on, fac, prods, d in zip(t["on"], t["fac"], t["prods"], t["d"]):
            for c, p in enumerate(prods):
                small_wl &= ~on | (np.abs(p) < TINY)
                small_var &= ~on | (np.abs(((d * d) * t["P"][c]) * fac[:, c]) < TINY)
            over |= on & np.isfinite(d) & np.isinf(d * d) & np.isfinite(d.astype(F64) * d.astype(F64))
        out["W_l a non-zero subnormal sum of subnormal products"] = int((small_wl & (wl != 0) & (np.abs(wl) < TINY)).sum())
        out["var_W_l a non-zero subnormal sum of subnormal products"] = int((small_var & (var != 0) & (np.abs(var) < TINY)).sum())
        out["d * d overflows float32, not float64"] = int(over.sum())
    return out


# ---- exact arithmetic: where float64 versus float32, and a fused multiply-add, change bits -------------------------------------------
def rnd(x, p=24, emin=-149):
    """The Fraction x rounded to nearest-even at p bits of precision with the smallest exponent emin (float32; p = 53,
    emin = -1074: float64).  Overflow is not handled: the callers hand in what stays in range."""
    if x == 0:
        return Fraction(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = max(e - (p - 1), emin)
    scaled = a / Fraction(2) ** q
    n, rem = divmod(scaled.numerator, scaled.denominator)
    if 2 * rem > scaled.denominator or (2 * rem == scaled.denominator and n % 2):
        n += 1
    return (n if x > 0 else -n) * Fraction(2) ** q


def rnd64(x):
    return rnd(x, 53, -1074)


def exact_counts(g, slots=None):
    """Terms for which (a) forming 1 - A or 2 (1 - A) A in float32 changes the bits of P0 or P1, (b) forming (1 - g0) - g1 in float32
    changes f2, (c) a fused multiply-add in like0 P0 + like1 P1 changes the sum's bits at some loop step.  Every rounding is made
    here, on fractions; operands that are not finite, and frequencies beyond 2 in size, are not counted.  (A result of zero has no sign
    here: a sign that alone differs is not counted.)  The float64 path is asserted to be what NumPy computed."""
    t = {}
    statistic(g, slots, trace=t)
    A, g0, g1, (P0, P1, P2), ind = t["A"], t["g0"], t["g1"], t["P"], t["ind"]
    fr = lambda v: Fraction(float(v))
    usable = np.isfinite(A) & (np.abs(A) <= 2)
    p_of = {}
    for a in np.unique(A[usable]):
        x = fr(a)
        om64, om32 = rnd64(1 - x), rnd(1 - x)
        ref = (rnd(rnd64(om64 * om64)), rnd(rnd64(2 * om64 * x)))
        alt = (rnd(om32 * om32), rnd(2 * om32 * x))
        at = np.flatnonzero(A == a)[0]
        assert ref == (fr(P0[at]), fr(P1[at])), ("the restatement's P0, P1 at", a)
        p_of[float(a)] = ref != alt
    changed_p = int(sum(p_of[float(a)] for a in A[usable]))
    ok = usable & np.isfinite(g0) & np.isfinite(g1)
    f2_of, changed_f2 = {}, 0
    for j in np.flatnonzero(ok):
        key = (float(g0[j]), float(g1[j]), float(P2[j]))
        if key not in f2_of:
            x0, x1, p2 = (Fraction(v) for v in key)
            ref = rnd(rnd64(rnd64(rnd64(1 - x0) - x1) * p2))
            alt = rnd(rnd64(rnd(rnd(1 - x0) - x1) * p2))
            f2_of[key] = ref != alt
        changed_f2 += f2_of[key]
    fma_of, changed_fma = {}, np.zeros(len(A), dtype=bool)
    finite_p = np.isfinite(P0) & np.isfinite(P1) & usable
    for a, on in enumerate(t["on"]):
        Dl = t["Dl"]
        r = g["index"][np.where(on, a, 0), np.where(on, Dl - a, 0)]
        like = g["like"][ind, r]
        for j in np.flatnonzero(on & finite_p & np.isfinite(like[:, 0]) & np.isfinite(like[:, 1])):
            key = (float(like[j, 0]), float(P0[j]), float(like[j, 1]), float(P1[j]))
            if key not in fma_of:
                l0, p0, l1, p1 = (Fraction(v) for v in key)
                second = rnd(l1 * p1)
                fma_of[key] = rnd(rnd(l0 * p0) + second) != rnd(l0 * p0 + second)
            changed_fma[j] |= fma_of[key]
    return {"1 - A or 2 (1 - A) A in float32 changes P0 or P1": changed_p, "(1 - g0) - g1 in float32 changes f2": changed_f2,
            "a fused multiply-add changes like0 P0 + like1 P1": int(changed_fma.sum())}


# ---- what is recorded from the real reference ----------------------------------------------------------------------------------------
GOLDEN_GEN = dict(ordinary_every=1, hostile_every=1)


def recorded_slots(g, ordinary_every=1, hostile_every=1):
    """Per individual the term sites (positions in g["sites"]) whose terms the reference was run on: every `hostile_every`-th of a
    hostile table, every `ordinary_every`-th of an ordinary one, the first taken in turn.  (n, slots) is ragged: a list of arrays."""
    ns = len(g["sites"])
    return [np.arange(i % (hostile_every if v else ordinary_every), ns, hostile_every if v else ordinary_every)
            for i, v in enumerate(g["variant"])]


# ---- the pipeline case ---------------------------------------------------------------------------------------------------------------
PIPELINE_GEN = dict(m=1600, per_class=3, seed=3)


def boundary_frequencies(**gen):
    """(L, AD, IDs, A): zscore_cases.every_class with a frequency file that holds exactly 0 at every 7th site and exactly 1 at every
    11th -- the assignment flavour takes its frequencies from the file and does not clamp them.  A hard call against such a frequency
    is log(0) = -inf in W_l_obs, and a class mean with a zero next to P = 0 is NaN in W_l."""
    L, AD, IDs, A, _ = zscore_cases.every_class(**(gen or PIPELINE_GEN))
    A = A.copy()
    A[0::7] = 0
    A[0::11] = 1
    return L, AD, IDs, A


def same_nan(got, want):
    """Bit-identical where the reference is not NaN, NaN exactly where it is."""
    return fisher_cases.same_nan(np.asarray(want), np.asarray(got))


def differences(got, want):
    """Flat indices at which `got` is not the reference's value (NaN for NaN counts as equal)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F32, (got.shape, want.shape, got.dtype, want.dtype)
    return np.flatnonzero(((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).ravel())


# ---- the mask sweep: what NumPy keeps, the deep branch at the 0.01 edge, special values --------------------------------------------
def expected_keep(L, AD, i, key_mean, key_comp, deep_map=None, deep_rows=None):
    """get_L_keep as the mask sweep is fed: bool (m,).  A dense class keeps a site if it has a component (>= 0) and NumPy's
    ~(abs(mean - v) > float32(0.01)) holds there; a deep site (deep_map given) if its depth has rows, by the component and the mean
    in row deep_map[depth] + Aa; without a deep table no deep site is kept.  key_mean, key_comp (253,), deep_map (511,)."""
    g0, g1 = L[:, 2 * i], L[:, 2 * i + 1]
    with np.errstate(all="ignore"):
        T = np.stack((g0, g1, (F32(1) - g0) - g1), axis=1)
        Ar, Aa = AD[:, 2 * i].astype(np.int64), AD[:, 2 * i + 1].astype(np.int64)
        dense = Ar + Aa <= MAX_DENSE
        k = np.where(dense, class_index(Ar, Aa), 0)
        comp, mean = key_comp[k], key_mean[k]
        if deep_map is not None:
            r = deep_map[np.where(dense, 0, Ar + Aa)]
            row = deep_rows[np.where(dense | (r < 0), 0, r + Aa)]
            comp = np.where(dense, comp, np.where(r >= 0, row[:, 0].astype(np.int64), -1))
            mean = np.where(dense, mean, row[:, 1])
        else:
            comp = np.where(dense, comp, -1)
        v = T[np.arange(len(g0)), np.clip(comp, 0, 2)]
        return (comp >= 0) & ~(np.abs(mean.astype(F32) - v) > F32(0.01))


THRESHOLD_DEEP_DEPTH, THRESHOLD_DROPPED_DEPTH = 25, 31
THRESHOLD_DEEP_AA = (0, 25, 1, 13, 24, 7, 12, 2, 19, 23, 5, 14, 9)          # the Aa of the 13 classes with a component


def deep_threshold_sites():
    """zscore_cases.threshold_sites -- the groups of seven float32 neighbours around mean -/+ float32(0.01) at each of the three
    components, and the class whose mean is NaN -- under classes of the deep depth 25: their means and components sit in the deep rows
    (row[0], row[1]).  The sites of the class without a component lie at depth 31, whose deep_map entry is -1: all dropped.
    dict(L, AD, key_mean, key_comp (nothing dense has a component), deep_map (2, 511), deep_rows (52, 8), expect bool (m, 2))."""
    t = zscore_cases.threshold_sites()
    L, AD = t["L"], np.zeros_like(t["AD"])
    d = THRESHOLD_DEEP_DEPTH
    deep_map = np.full((2, DEEP_MAX + 1), -1, dtype=np.int32)
    deep_rows = np.zeros((2 * (d + 1), DEEP_ROW), dtype=F32)
    deep_rows[:, 1] = 0.5
    for i in range(2):
        classes = zscore_cases.THRESHOLD_CLASSES if i == 0 else zscore_cases.THRESHOLD_CLASSES[::-1]
        deep_map[i, d] = i * (d + 1)
        slot = np.array([classes.index(int(k)) for k in zscore_cases.class_index(t["AD"][:, 2 * i], t["AD"][:, 2 * i + 1])])
        for s, k in enumerate(classes):
            if t["key_comp"][i, k] >= 0:
                a = THRESHOLD_DEEP_AA[s if i == 0 else len(THRESHOLD_DEEP_AA) - 1 - s]
                deep_rows[i * (d + 1) + a, :2] = (t["key_comp"][i, k], t["key_mean"][i, k])
                AD[slot == s, 2 * i], AD[slot == s, 2 * i + 1] = d - a, a
            else:
                at = np.flatnonzero(slot == s)
                AD[at, 2 * i], AD[at, 2 * i + 1] = THRESHOLD_DROPPED_DEPTH - at % 32, at % 32
    return dict(L=L, AD=AD, key_mean=np.zeros((2, N_CLASSES), dtype=F32), key_comp=np.full((2, N_CLASSES), -1, dtype=np.int32),
                deep_map=deep_map, deep_rows=deep_rows, expect=t["expect"], dropped_sites=t["dropped_sites"], nan_sites=t["nan_sites"])


SPECIAL_MEANS = (0.5, INF, 0.0)
SPECIAL_VALUES = {0.5: (NAN, INF, -INF, 0.5, 0.52), INF: (INF, 1e30, NAN, -INF, 3e38), 0.0: (-0.0, 1e-40, -1e-40, 0.0, 0.02)}
SPECIAL_DEEP_DEPTH = 26


def special_mask_values():
    """One individual; per component 0, 1, 2 and per mean of SPECIAL_MEANS a dense class and a class of the deep depth 26, whose sites
    hold SPECIAL_VALUES at the component: NaN (kept), +/-inf under a finite mean (dropped), +inf under a mean of +inf (kept: inf - inf
    is NaN), -0.0 and subnormals under a mean of 0 (kept).  (At the third component -0.0 cannot be formed: it holds +0.0 there.)
    dict(L, AD, key_mean, key_comp (1, 253), deep_map (1, 511), deep_rows (27, 8), cells [(site, component, mean, value, deep)])."""
    d = SPECIAL_DEEP_DEPTH
    key_mean = np.zeros((1, N_CLASSES), dtype=F32)
    key_comp = np.full((1, N_CLASSES), -1, dtype=np.int32)
    deep_map = np.full((1, DEEP_MAX + 1), -1, dtype=np.int32)
    deep_map[0, d] = 0
    deep_rows = np.zeros((d + 1, DEEP_ROW), dtype=F32)
    deep_rows[:, 1] = 0.5
    rows, cells = [], []
    for c in range(3):
        for j, mean in enumerate(SPECIAL_MEANS):
            dense_pair, a = zscore_cases.pair_of((3, 66, 129, 200, 252, 40, 100, 150, 231)[3 * c + j]), (0, 26, 13, 1, 25, 7, 20, 3, 11)[3 * c + j]
            key_mean[0, class_index(*dense_pair)], key_comp[0, class_index(*dense_pair)] = mean, c
            deep_rows[a, :2] = (c, mean)
            for v in SPECIAL_VALUES[mean]:
                pair = (v, 0.0) if c == 0 else (0.0, v) if c == 1 else (1.0, -v) if 0 < abs(v) < 1e-30 else (1.0 - v, 0.0)
                for deep, ad in ((False, dense_pair), (True, (d - a, a))):
                    cells.append((len(rows), c, mean, v, deep))
                    rows.append(pair + ad)
    rows = np.array(rows, dtype=F64)
    order = np.argsort((np.arange(len(rows)) * 37) % len(rows), kind="stable")      # dense and deep, means and components mixed
    inverse = np.argsort(order)
    cells = [(int(inverse[s]), c, mean, v, deep) for s, c, mean, v, deep in cells]
    with np.errstate(all="ignore"):
        L = np.ascontiguousarray(rows[order, :2].astype(F32))
    AD = np.ascontiguousarray(rows[order, 2:].astype(np.int32))
    return dict(L=L, AD=AD, key_mean=key_mean, key_comp=key_comp, deep_map=deep_map, deep_rows=deep_rows, cells=cells)
