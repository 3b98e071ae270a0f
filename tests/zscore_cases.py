"""Enumerated inputs for the z-score kernels (csrc/zscore_kernels.hip), each built for one place the generated cases never reach:
the depth classes 64 .. 252 (depths 11 .. 21) that three of the four wavefronts of the class sweep own, the 0.01 site filter
exactly at its edge, the partitions the prefix scan makes of its 256 threads, and the sweep's own copy of the table logarithm.
NumPy only; the twin of tests/codes_cases.py and tests/token_cases.py.  Every builder is seeded and returns the inputs next to the
claims they are built to satisfy; tests/test_zscore_cases_cpu.py holds them to those claims on tests/zscore_cpu.py, and
tests/test_gpu_zscore_classes.py runs them through the library."""
import numpy as np

import synth_deep
import synth_depth

F32 = np.float32
N_CLASSES, MAX_DENSE = 253, 21
D_OF = np.repeat(np.arange(MAX_DENSE + 1), np.arange(MAX_DENSE + 1) + 1)             # class -> depth
A_OF = np.arange(N_CLASSES) - D_OF * (D_OF + 1) // 2                                 # class -> Aa
WAVE_CLASSES = (5, 70, 130, 252)          # one class of each wavefront of zclass_kernel (class >> 6 = 0, 1, 2, 3)
FULL = (1, 2)                             # the individuals that get every class: one in each population (batches of 2 part them)
CLASSES_JITTER = 0.006


def class_index(Ar, Aa):
    d = np.asarray(Ar) + np.asarray(Aa)
    return d * (d + 1) // 2 + np.asarray(Aa)


def pair_of(k):
    """(Ar, Aa) of class k."""
    return int(D_OF[k] - A_OF[k]), int(A_OF[k])


def overwrite(L, AD, i, sites, Ar, Aa, rng, jitter):
    """Cells (sites, individual i) get the depth pairs and the fixed-error likelihoods of their class plus N(0, jitter), clipped and
    rounded to 6 decimals exactly as synth_deep.make_deep does."""
    Ar, Aa = np.asarray(Ar, dtype=np.int64), np.asarray(Aa, dtype=np.int64)
    g0, g1 = synth_deep.class_triple(Ar, Aa)
    g0 = np.clip(g0 + rng.normal(0.0, jitter, g0.shape), 0.0, 1.0)
    g1 = np.clip(g1 + rng.normal(0.0, jitter, g1.shape), 0.0, 1.0 - g0)
    g0 = np.round(g0, 6)
    g1 = np.minimum(np.round(g1, 6), np.round(1.0 - g0, 6))
    L[sites, 2 * i], L[sites, 2 * i + 1] = g0, g1
    AD[sites, 2 * i], AD[sites, 2 * i + 1] = Ar, Aa


def fixed_places(m, q):
    """The fixed placements of full individual number q (0, 1): {site: class}.
    Every class of WAVE_CLASSES sits at lanes 0 and 63 of one of the first four tiles (two classes cannot share a site, so each takes
    a tile of its own; which class takes tile 0 differs between the two individuals); the sites 4095 and 4096 hold classes >= 64;
    the first and the last site of the last tile hold classes of depth 21."""
    at = {}
    for w, k in enumerate(WAVE_CLASSES):
        t = (w + 2 * q) % 4
        at[64 * t], at[64 * t + 63] = k, k
    if m > 4097:
        at[4095], at[4096] = 100 + q, 200 + q
    last = (m - 1) // 64 * 64
    at[last], at[m - 1] = 231 + q, 252 - 2 * q
    assert len(at) == (12 if m > 4097 else 10) and max(at) < m and m > 320
    return at


def every_class(m=4163, per_class=6, seed=3):
    """(L, AD, IDs, A, placed): synth_depth.make_depth(m, 4, 2, depth=1.5, jitter=0.01, sizes=(2, 2)) -- at the default 66 tiles, the
    last one partial, across site 4096 -- in which the individuals FULL have every one of the 253 pairs of the depths 0 .. 21 at
    `per_class` chosen sites each; the individuals 0 and 3 stay shallow and share batches with them.
    placed[i] = {site: class} of fixed_places; all other sites of the classes are seeded random ones."""
    gen = dict(m=m, n=4, K=2, depth=1.5, jitter=0.01, sizes=(2, 2))
    L, AD, IDs, A = synth_depth.make_depth(**gen)
    L, AD = L.copy(), AD.copy()
    assert int((AD[:, 0::2] + AD[:, 1::2]).max()) <= MAX_DENSE
    rng = np.random.Generator(np.random.PCG64(seed + 104729))
    placed = {}
    for q, i in enumerate(FULL):
        at = fixed_places(m, q)
        need = np.full(N_CLASSES, per_class)
        for k in at.values():
            need[k] -= 1
        assert need.min() >= 0
        rest = np.repeat(np.arange(N_CLASSES), need)
        rest = rest[rng.permutation(len(rest))]
        free = np.setdiff1d(np.arange(m), list(at))
        sites = np.concatenate((np.array(list(at), dtype=np.int64), rng.choice(free, size=len(rest), replace=False)))
        k = np.concatenate((np.array(list(at.values()), dtype=np.int64), rest))
        overwrite(L, AD, i, sites, D_OF[k] - A_OF[k], A_OF[k], rng, CLASSES_JITTER)
        placed[i] = at
    return L, AD, IDs, A, placed


def incomplete_21(**kw):
    """every_class with every site of class (10, 11) of individual 1 counted as (11, 10): depth 21 then has 21 classes and is dropped
    whole -- its sites reach the mask sweep with no component -- and depth 20 stays."""
    L, AD, IDs, A, placed = every_class(**kw)
    at = (AD[:, 2] == 10) & (AD[:, 3] == 11)
    assert at.sum() > 0
    AD[at, 2], AD[at, 3] = 11, 10
    return L, AD, IDs, A, placed


EDGE_IND = 2
EDGE_DENSE = ((21, 0), (0, 21), (10, 11))                  # classes 231, 252, 242: the last the dense tier holds
EDGE_OVER = ((22, 0), (0, 22), (11, 11)) + synth_deep.SINGLES


def edge_of_dense(m=331, seed=5, rounds=7):
    """(L, AD, IDs, A, claims): four shallow individuals (depths of Poisson 1.5, at most 12); individual EDGE_IND has, `rounds`
    times, the pairs of EDGE_DENSE and EDGE_OVER at consecutive sites, alternating.  claims: the number of its sites beyond the
    dense tier (`over`) and the counts of the classes 231, 252 and 242, which nothing else touches."""
    L, AD, IDs, A = synth_depth.make_depth(m, 4, 2, seed=seed, depth=1.5, jitter=0.01, sizes=(2, 2))
    L, AD = L.copy(), AD.copy()
    rng = np.random.Generator(np.random.PCG64(seed + 1299709))
    pairs = []
    for r in range(rounds):
        for j in range(len(EDGE_OVER)):
            pairs += [EDGE_DENSE[(j + r) % 3], EDGE_OVER[j]]
    starts = [0, 60, 126] + [int(s) for s in rng.choice(np.arange((m - 152) // 12), size=rounds - 3, replace=False) * 12 + 140]
    sites = np.concatenate([np.arange(s, s + 12) for s in starts])           # 0 .. 11, 60 .. 71 (across a tile), 126 .. 137, ...
    assert len(np.unique(sites)) == len(pairs) and sites.max() < m
    Ar, Aa = np.array(pairs, dtype=np.int64).T
    overwrite(L, AD, EDGE_IND, sites, Ar, Aa, rng, CLASSES_JITTER)
    claims = dict(over=rounds * len(EDGE_OVER), counts={int(class_index(a, b)): 2 * rounds for a, b in EDGE_DENSE})
    return L, AD, IDs, A, claims


THRESHOLD_MEANS = (F32(0.5), F32(0.02), F32(0.99), F32(1) / F32(3))
THRESHOLD_CLASSES = (1, 64, 5, 70, 127, 40, 128, 130, 191, 63, 192, 231, 242, 252)     # 12 (mean, component) pairs, NaN, no component


def step(v, k):
    """The float32 k steps above (below) the positive float32 v."""
    return (np.asarray(v, dtype=F32).view(np.int32) + np.int32(k)).view(F32)


def third_from(v):
    """(g0, g1) with (float32(1) - g0) - g1 == v exactly: g0 = 1 - 2^-j with the smallest power of two that is >= v (0 for v >= 1,
    where g1 comes out as a small negative number: the sweep does not ask for a valid likelihood)."""
    v = F32(v)
    a = F32(1)
    while a * F32(0.5) >= v:
        a = a * F32(0.5)
    g0 = F32(1) - a
    g1 = F32(np.float64(a) - np.float64(v))
    assert np.float64(g1) == np.float64(a) - np.float64(v) and (F32(1) - g0) - g1 == v, v
    return g0, g1


def threshold_sites(seed=9):
    """The 0.01 filter at its edge.  For every mean of THRESHOLD_MEANS and every component 0, 1, 2 one class (of one individual; the
    second individual has the same sites under the classes in reverse order); its sites hold, at that component, float32(mean -
    float32(0.01)), float32(mean + float32(0.01)) and the three float32 neighbours on each side of both: two groups of seven.  One more
    class has a mean of NaN and one no component (-1).  Site order is a seeded shuffle.
    Returns dict(L, AD, key_mean, key_comp float32/int32 (2, 253), expect bool (m, 2), groups [(individual-0 class, sites of the group)],
    nan_sites, dropped_sites)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, groups = [], []                                  # rows: (class slot, component, value)
    slot = 0
    for mean in THRESHOLD_MEANS:
        for c in range(3):
            for sign in (-1, 1):
                centre = F32(mean - F32(0.01)) if sign < 0 else F32(mean + F32(0.01))
                groups.append((slot, len(rows)))
                rows += [(slot, c, step(centre, k)) for k in range(-3, 4)]
            slot += 1
    nan_slot, drop_slot = slot, slot + 1
    rows += [(nan_slot, 0, F32(v)) for v in (0.0, 0.25, 0.5, 0.75, 0.98, 0.99, 1.0)]
    rows += [(drop_slot, 0, F32(v)) for v in (0.0, 0.25, 0.5, 0.75, 0.98, 0.99, 1.0)]
    m = len(rows)
    where = rng.permutation(m)                             # row r sits at site where[r]
    L = np.zeros((m, 4), dtype=F32)
    AD = np.zeros((m, 4), dtype=np.int32)
    key_mean = np.zeros((2, N_CLASSES), dtype=F32)
    key_comp = np.full((2, N_CLASSES), -1, dtype=np.int32)
    expect = np.zeros((m, 2), dtype=bool)
    means = [m_ for m_ in THRESHOLD_MEANS for _ in range(3)] + [F32(np.nan), F32(0.5)]
    comps = [c for _ in THRESHOLD_MEANS for c in range(3)] + [0, -1]
    for i in range(2):
        classes = THRESHOLD_CLASSES if i == 0 else THRESHOLD_CLASSES[::-1]
        for s, k in enumerate(classes):
            key_mean[i, k], key_comp[i, k] = means[s], comps[s]
        for r, (s, c, v) in enumerate(rows):
            if c == 0:
                g0, g1 = v, F32(0)
            elif c == 1:
                g0, g1 = F32(0), v
            else:
                g0, g1 = third_from(v)
            site = where[r]
            L[site, 2 * i], L[site, 2 * i + 1] = g0, g1
            AD[site, 2 * i:2 * i + 2] = pair_of(classes[s])
            with np.errstate(invalid="ignore"):
                expect[site, i] = comps[s] >= 0 and bool(~(np.abs(means[s] - v) > F32(0.01)))
    return dict(L=L, AD=AD, key_mean=key_mean, key_comp=key_comp, expect=expect,
                groups=[(THRESHOLD_CLASSES[s], means[s], comps[s], where[r0:r0 + 7]) for s, r0 in groups],
                nan_sites=where[[r for r, row in enumerate(rows) if row[0] == nan_slot]],
                dropped_sites=where[[r for r, row in enumerate(rows) if row[0] == drop_slot]])


SCAN_SITES = (37, 101, 255 * 64 - 27, 256 * 64 - 27, 256 * 64 + 1, 257 * 64 - 27, 511 * 64 - 27, 512 * 64, 513 * 64)
SCAN_PATTERNS = ("all", "none", "last", "lane0", "half")


def scan_pattern(name, m, rng):
    keep = np.zeros(m, dtype=bool)
    if name == "all":
        keep[:] = True
    elif name == "last":
        keep[m - 1] = True
    elif name == "lane0":
        keep[0::64] = True
    elif name == "half":
        keep[rng.permutation(m)[:m // 2]] = True
    else:
        assert name == "none"
    return keep


def scan_shapes(seed=13):
    """[(m, names, keep bool (m, 3))]: site counts of 1, 2, 255, 256, 257 (once with a last tile of a single site), 511, 512 and 513
    tiles -- zscan_kernel's 256 threads take 1, 2 or 3 tiles each, with and without idle threads -- and per launch three
    individuals with three different keep patterns of SCAN_PATTERNS, rotating from shape to shape."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for s, m in enumerate(SCAN_SITES):
        names = tuple(SCAN_PATTERNS[(s + j) % 5] for j in range(3))
        out.append((m, names, np.stack([scan_pattern(nm, m, rng) for nm in names], axis=1)))
    return out


def scan_inputs(m, keep):
    """(L, AD, key_mean, key_comp) that make the mask sweep keep exactly `keep` and the statistic sweep return a distinct W_l_obs =
    log(g0) per kept (site, individual) (depth (0, 0), g1 = 0, frequency 0: log_inputs): class 0 has component 0 and mean 0.5; a kept
    site holds g0 = 0.5 + (individual * m + site) * 2^-24 (at most 0.006 above the mean), a dropped one 0.25 + the same * 2^-25."""
    n = keep.shape[1]
    assert n * m < 0.009 * 2 ** 24
    number = np.arange(n, dtype=np.float64)[None, :] * m + np.arange(m, dtype=np.float64)[:, None]
    g0 = np.where(keep, 0.5 + number * 2.0 ** -24, 0.25 + number * 2.0 ** -25)
    L = np.zeros((m, 2 * n), dtype=F32)
    L[:, 0::2] = g0
    assert np.array_equal(L[:, 0::2].astype(np.float64), g0)                             # exact in float32
    key_mean = np.zeros((n, N_CLASSES), dtype=F32)
    key_comp = np.full((n, N_CLASSES), -1, dtype=np.int32)
    key_mean[:, 0], key_comp[:, 0] = 0.5, 0
    return L, np.zeros((m, 2 * n), dtype=np.int32), key_mean, key_comp


def log_tables(n):
    """Statistic tables (n, 253, 6) whose row of class 0 is AD_like = (1, 0, 0), AD_factorial = (1, 1, 1): with frequency 0 the loops
    of a site of depth 0 give W_l = log(1) = 0 and var_W_l = 0, and W_l_obs = log(g0 * 1 + g1 * 0 + ((1 - g0) - g1) * 0)."""
    tabs = np.zeros((n, N_CLASSES, 6), dtype=F32)
    tabs[:, 0] = (1, 0, 0, 1, 1, 1)
    return tabs


def log_inputs(x):
    """One individual whose site s has depth (0, 0), g0 = x[s], g1 = 0, kept by component 1 with mean 0: (L, AD, key_mean, key_comp)."""
    x = np.ascontiguousarray(x, dtype=F32)
    L = np.zeros((len(x), 2), dtype=F32)
    L[:, 0] = x
    key_mean = np.zeros((1, N_CLASSES), dtype=F32)
    key_comp = np.full((1, N_CLASSES), -1, dtype=np.int32)
    key_comp[0, 0] = 1
    return L, np.zeros((len(x), 2), dtype=np.int32), key_mean, key_comp


LOG_OFF, LOG_N = 0x3FE60000, 128                           # = WGS_LOG_OFF, WGS_LOG_N of csrc/log_table.h


def log_interval(bits):
    """The table interval the device logarithm takes for the float32 with these bits: ((bits(double(x)) >> 32) - LOG_OFF) >> 13."""
    hi = (np.asarray(bits, dtype=np.uint32).view(F32).astype(np.float64).view(np.uint64) >> np.uint64(32)).astype(np.int64)
    return (hi - LOG_OFF) >> 13


def log_arguments():
    """Float32 bit patterns (uint32), all finite and non-negative, as parts:
    quarter, half, one   every mantissa of [0.25, 0.5), [0.5, 1), [1, 2) -- the binade [0.5, 1) straddles the table's split at 0.6875
                         and the cancellation next to 1;
    stride               every 8193rd pattern of the whole positive range;
    edges                the 128 patterns of [0.6875, 1.375) at which the table interval changes, each with its two neighbours;
    specials             +0, the smallest and the largest subnormal, the smallest normal, FLT_MAX."""
    b = lambda v: int(F32(v).view(np.uint32))
    parts = {name: np.arange(b(lo), b(lo) + (1 << 23), dtype=np.uint32) for name, lo in (("quarter", 0.25), ("half", 0.5), ("one", 1.0))}
    parts["stride"] = np.arange(1, 0x7F800000, 8193, dtype=np.uint32)
    span = np.arange(b(0.6875) - 1, b(1.375), dtype=np.uint32)
    change = span[1:][np.diff(log_interval(span)) != 0]
    parts["edges"] = np.sort(np.concatenate((change - 1, change, change + 1)).astype(np.uint32))
    parts["specials"] = np.array([0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF], dtype=np.uint32)
    return parts


CLASSES_CUT = 2111          # the one cut of the sharded case `classes`: inside tile 32


def sides_of_cut(AD, i, cut, lo=64):
    """For individual i the classes >= lo whose sites lie all before `cut`, all from `cut` on, and on both sides."""
    k = class_index(AD[:, 2 * i].astype(np.int64), AD[:, 2 * i + 1].astype(np.int64))
    before, after = np.unique(k[:cut]), np.unique(k[cut:])
    before, after = before[before >= lo], after[after >= lo]
    return np.setdiff1d(before, after), np.setdiff1d(after, before), np.intersect1d(before, after)
