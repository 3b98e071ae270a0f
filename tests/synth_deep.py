"""Seeded inputs with DEEP sites (Ar + Aa > 21) for the z-score tests and tests/golden/zscore_deep.npz.

Starts from synth_depth.make_depth and overwrites chosen (site, individual) cells.  A deep site's likelihoods are a function of its
class -- the fixed-error model of synth_depth, which is nearly one-hot at these depths -- plus a small jitter: with likelihoods
drawn independently of the depth the reference's 0.01 filter around the class mean keeps almost no deep site, and a kept deep
depth would go untested.  Values are rounded to 6 decimals like the text of a Beagle file.  Test infrastructure (NumPy).

Roles of the individuals (`roles`, one per individual):
  "none"     no deep site;
  "dropped"  sites of depths 22..60 whose alternative count is never 0, so no deep depth has all its classes: all are dropped;
  "kept"     every class of the depths 22 and 23, `per_class` sites each -- except the class (10, 12), which gets `short_class`
             sites, so that a threshold between the two numbers removes it and with it depth 22;
  "single"   one site each of (255, 255), (200, 0) and (0, 37).
The first deep sites of every individual go to `corners`: lane 0 and lane 63 of the first tile (two in one tile), both sides of
site 4096 where there are that many sites, and the first and the last site of the last, partial tile."""
import numpy as np

import synth_depth

E = synth_depth.E
SHORT_CLASS = (10, 12)
SINGLES = ((255, 255), (200, 0), (0, 37))


def corners(m):
    last = (m - 1) // 64 * 64
    c = [0, 63] + ([4095, 4096] if m > 4097 else []) + [last, m - 1]
    return [s for s in dict.fromkeys(c) if 0 <= s < m]


def class_triple(Ar, Aa):
    """(g0, g1) of the fixed-error model in float64; computed in logs: E ** 255 underflows."""
    Ar, Aa = np.asarray(Ar, dtype=np.float64), np.asarray(Aa, dtype=np.float64)
    l0 = Ar * np.log(1.0 - E) + Aa * np.log(E)
    l1 = (Ar + Aa) * np.log(0.5)
    l2 = Aa * np.log(1.0 - E) + Ar * np.log(E)
    top = np.maximum(np.maximum(l0, l1), l2)
    e0, e1, e2 = np.exp(l0 - top), np.exp(l1 - top), np.exp(l2 - top)
    s = e0 + e1 + e2
    return e0 / s, e1 / s


def deep_pairs(role, rng, per_class, short_class):
    if role == "none":
        return []
    if role == "single":
        return list(SINGLES)
    if role == "dropped":
        d = rng.integers(22, 61, size=40)
        return [(int(x - a), int(a)) for x, a in zip(d, rng.integers(1, d + 1))]          # Aa >= 1: class (d, 0) never appears
    assert role == "kept", role
    pairs = []
    for d in (22, 23):
        for a in range(d + 1):
            pairs += [(d - a, a)] * (short_class if (d - a, a) == SHORT_CLASS else per_class)
    return [pairs[j] for j in rng.permutation(len(pairs))]


def make_deep(m, n, K, seed, roles, sizes=None, depth=1.5, jitter=0.01, deep_jitter=0.008, per_class=4, short_class=2):
    """Return (L, AD, IDs, A) as synth_depth.make_depth does, and deep: per individual the sorted sites that were overwritten."""
    assert len(roles) == n
    L, AD, IDs, A = synth_depth.make_depth(m, n, K, seed=seed, depth=depth, jitter=jitter, sizes=sizes)
    L, AD = L.copy(), AD.copy()
    assert int((AD[:, 0::2] + AD[:, 1::2]).max()) <= 21, "the base table is meant to be shallow"
    rng = np.random.Generator(np.random.PCG64(seed + 7919))
    deep = []
    for i, role in enumerate(roles):
        pairs = deep_pairs(role, rng, per_class, short_class)
        fixed = corners(m)[:len(pairs)]
        free = np.setdiff1d(np.arange(m), fixed)
        sites = np.array(fixed + list(rng.choice(free, size=len(pairs) - len(fixed), replace=False)), dtype=np.int64)
        if len(pairs):
            Ar, Aa = np.array(pairs, dtype=np.int64).T
            g0, g1 = class_triple(Ar, Aa)
            g0 = np.clip(g0 + rng.normal(0.0, deep_jitter, g0.shape), 0.0, 1.0)
            g1 = np.clip(g1 + rng.normal(0.0, deep_jitter, g1.shape), 0.0, 1.0 - g0)
            g0 = np.round(g0, 6)
            g1 = np.minimum(np.round(g1, 6), np.round(1.0 - g0, 6))
            L[sites, 2 * i], L[sites, 2 * i + 1] = g0, g1
            AD[sites, 2 * i], AD[sites, 2 * i + 1] = Ar, Aa
        deep.append(np.sort(sites))
    return L, AD, IDs, A, deep
