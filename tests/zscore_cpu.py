"""CPU restatement of the reference's z-score (zscore.py, zscore_cy.pyx, WGSassign.py:311-446), vectorised NumPy.

Test infrastructure: the yardstick the GPU path is held to on shapes the goldens do not cover.  tests/test_zscore_cpu.py pins
it, array by array and bit for bit, to tests/golden/zscore.npz, which was recorded from the real reference.  Written from the
description of the computation, operation by operation:

  1. depth classes   per individual the sites grouped by (Ar, Aa), in order of first appearance; per class the count and the mean
                     of (g0, g1, 1 - g0 - g1): float32 sums in site order, divided by the count;
  2. key filter      depth 1 only (single_read_threshold) or count > threshold and depth != 0; then only the depths d that have
                     more than d surviving classes;
  3. site filter     the site's class survived and, at the component where the class mean is largest, the site's own value is
                     within float32(0.01) of it;
  4. tables          binomial coefficient x error model in float64, stored float32; the class means; the index table;
  5. per kept site   the arithmetic of zscore_cy.pyx as its C translation performs it: 1 - A and 2 (1 - A) A in float64 (the
                     literals are doubles), A A in float32, products with the likelihoods in float32 except the third
                     ((1 - g0) - g1 in float64), the logarithms in float64 of a float32 sum, every accumulation a float32 add;
                     the tables are read at AD_index[Aa, Ar], the transpose of how the index was written;
  6. sums            NumPy's float32 pairwise sums of the compacted arrays; z = (W_l_obs - sum W_l) / sqrt(sum var).
"""
import math

import numpy as np

F32 = np.float32
E = 0.01


def triple(L, i):
    g0, g1 = L[:, 2 * i], L[:, 2 * i + 1]
    return g0, g1, (F32(1) - g0) - g1


def depth_classes(L, AD, i):
    """Step 1: keys (nk, 2) int in order of first appearance, counts (nk,), means float32 (nk, 3), sums float32 (nk, 3)."""
    Ar, Aa = AD[:, 2 * i].astype(np.int64), AD[:, 2 * i + 1].astype(np.int64)
    code = (Ar << 32) | Aa
    uniq, first, inv = np.unique(code, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    T = np.stack(triple(L, i), axis=1)
    keys = np.empty((len(uniq), 2), dtype=np.int64)
    counts = np.empty(len(uniq), dtype=np.int64)
    sums = np.empty((len(uniq), 3), dtype=F32)
    for j, u in enumerate(order):
        idx = np.flatnonzero(inv.reshape(-1) == u)
        keys[j] = (uniq[u] >> 32, uniq[u] & 0xFFFFFFFF)
        counts[j] = len(idx)
        sums[j] = np.cumsum(T[idx], axis=0, dtype=F32)[-1]          # float32, one addition per site, site order
    means = (sums.astype(np.float64) / counts[:, None]).astype(F32)
    return keys, counts, means, sums


def key_filter(keys, counts, n_threshold, single_read_threshold):
    """Step 2: rows of (Ar, Aa, depth, count) that survive, in order of first appearance (the reference's AD_array)."""
    S = np.column_stack((keys[:, 0], keys[:, 1], keys[:, 0] + keys[:, 1], counts)).astype(np.int32)
    if single_read_threshold:
        Fl = S[S[:, 2] == 1]
    else:
        Fl = S[(S[:, 3] > n_threshold) & (S[:, 2] != 0)]
    assert Fl.shape[0] != 0, "No loci were kept! Too stringent filtering?"
    assert Fl.shape[0] != 1, "Not enough loci were kept! Too stringent filtering?"
    dl, dl_counts = np.unique(Fl[:, 2], return_counts=True)
    return Fl[np.isin(Fl[:, 2], dl[dl < dl_counts])]


def site_filter(L, AD, i, keys, means, AD_array):
    """Step 3: indices of the kept sites (int32), ascending."""
    Ar, Aa = AD[:, 2 * i], AD[:, 2 * i + 1]
    T = np.stack(triple(L, i), axis=1)
    keep = np.zeros(AD.shape[0], dtype=bool)
    where = {(int(a), int(b)): j for j, (a, b) in enumerate(keys)}
    for a, b in AD_array[:, :2]:
        mean = means[where[(int(a), int(b))]]
        c = int(np.argmax(mean))                        # first of the largest
        at = (Ar == a) & (Aa == b)
        keep |= at & ~(np.abs(mean[c] - T[:, c]) > F32(0.01))
    return np.flatnonzero(keep).astype(np.int32)


def tables(AD_array, keys, means, e=E):
    """Step 4: AD_factorial, AD_like (float32 (rows, 3)) and AD_index (int32, zeros where no class was kept)."""
    where = {(int(a), int(b)): j for j, (a, b) in enumerate(keys)}
    rows = AD_array.shape[0]
    fac = np.zeros((rows, 3), dtype=F32)
    like = np.zeros((rows, 3), dtype=F32)
    index = np.zeros((int(AD_array[:, 0].max()) + 1, int(AD_array[:, 1].max()) + 1), dtype=np.int32)
    for r in range(rows):
        Ar, Aa = int(AD_array[r, 0]), int(AD_array[r, 1])
        index[Ar, Aa] = r
        c = math.factorial(Ar + Aa) / (math.factorial(Aa) * math.factorial(Ar))
        fac[r] = [c * ((1.0 - e) ** Ar) * (e ** Aa), c * (0.5 ** (Ar + Aa)), c * ((1.0 - e) ** Aa) * (e ** Ar)]
        like[r] = means[where[(Ar, Aa)]]
    return fac, like, index


def _logf(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(x.astype(np.float64)).astype(F32)


def per_site(L, AD, i, keep, A, fac, like, index):
    """Step 5 on the kept sites: W_l_obs, W_l, var_W_l as float32 arrays (len(keep),).  A: frequencies OF THE KEPT SITES."""
    g0, g1 = L[keep, 2 * i], L[keep, 2 * i + 1]
    A = A.astype(F32)
    Ad = A.astype(np.float64)
    P0 = ((1.0 - Ad) * (1.0 - Ad)).astype(F32)
    P1 = ((2.0 * (1.0 - Ad)) * Ad).astype(F32)
    P2 = A * A
    f0, f1 = g0 * P0, g1 * P1
    f2 = (((1.0 - g0.astype(np.float64)) - g1.astype(np.float64)) * P2.astype(np.float64)).astype(F32)
    wobs = _logf((f0 + f1) + f2)
    Dl = AD[keep, 2 * i] + AD[keep, 2 * i + 1]
    wl = np.zeros(len(keep), dtype=F32)
    var = np.zeros(len(keep), dtype=F32)
    steps = []
    for a in range(int(Dl.max()) + 1 if len(keep) else 0):
        on = Dl >= a
        r = index[a, np.where(on, Dl - a, 0)]                                  # AD_index[Aa, Ar]
        lg = _logf((like[r, 0] * P0 + like[r, 1] * P1) + like[r, 2] * P2)
        steps.append((on, r, lg))
        for c, P in enumerate((P0, P1, P2)):
            wl = np.where(on, wl + (lg * P) * fac[r, c], wl)
    for on, r, lg in steps:
        d = wl - lg
        for c, P in enumerate((P0, P1, P2)):
            var = np.where(on, var + ((d * d) * P) * fac[r, c], var)
    return wobs, wl, var


def clamp(f, n_pop):
    lo = 1 / (2 * (n_pop + 1))
    f = f.copy()
    f[f < lo] = lo
    f[f > 1 - lo] = 1 - lo
    return f


def individual(L, AD, i, freq_of_kept, n_threshold=0, single_read_threshold=False):
    """Steps 1-6 for one individual.  freq_of_kept(keep) -> float32 frequencies of the kept sites (and, optionally, extras)."""
    keys, counts, means, sums = depth_classes(L, AD, i)
    AD_array = key_filter(keys, counts, n_threshold, single_read_threshold)
    keep = site_filter(L, AD, i, keys, means, AD_array)
    fac, like, index = tables(AD_array, keys, means)
    A = freq_of_kept(keep)
    extra = None
    if isinstance(A, tuple):
        A, extra = A
    wobs, wl, var = per_site(L, AD, i, keep, A, fac, like, index)
    W_l_obs = np.sum(wobs, dtype=F32)
    z_mu, z_var = np.sum(wl), np.sum(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (W_l_obs - z_mu) / np.sqrt(z_var)
    return dict(keys=keys, counts=counts, means=means, sums=sums, AD_array=AD_array, keep=keep, fac=fac, like=like, index=index,
                A=A, wobs=wobs, wl=wl, var=var, W_l_obs=W_l_obs, z_mu=z_mu, z_var=z_var, z=z, extra=extra)


def stdout_lines(i, r):
    return ["Finished individual " + str(i), "z_mu: " + str(r["z_mu"]), "z_var: " + str(r["z_var"]), "z_obs: " + str(r["W_l_obs"]),
            "Loci used: " + str(len(r["keep"])), "Z-score: " + str(r["z"])]


def ind_range(n, ind_start, ind_end):
    if ind_start is not None:
        assert (ind_start > 0 and ind_start <= n), "Start individual index needs to be within range of number of individuals!"
    if ind_end is not None:
        assert (ind_end > 0 and ind_end <= n), "End individual index needs to be within range of number of individuals!"
    return (0 if ind_start is None else ind_start), (n if ind_end is None else ind_end)


def file_text(z):
    return "".join("%.7f\n" % v for v in np.asarray(z, dtype=F32))


def assignment(L, AD, IDs, pops, A, n_threshold=0, single_read_threshold=False, ind_start=None, ind_end=None):
    """--get_assignment_z_score (WGSassign.py:395-446): list of per-individual results for [ind_start, ind_end)."""
    lo, hi = ind_range(L.shape[1] // 2, ind_start, ind_end)
    out = []
    for i in range(lo, hi):
        k = int(np.argwhere(pops == IDs[i, 1])[0][0])
        out.append(individual(L, AD, i, lambda keep: np.ascontiguousarray(A[keep, k]), n_threshold, single_read_threshold))
    return out


def reference(L, AD, IDs, em, maf_iter=200, maf_tole=1e-4, n_threshold=0, single_read_threshold=False, ind_start=None, ind_end=None):
    """--get_reference_z_score (WGSassign.py:311-393).  em(L_pop, iter, tole) -> (f float32 unclamped, iteration at convergence or
    0): the EM fit of emMAF.py:15-27 (the tests hand in the oracle's).  r["extra"] = that iteration."""
    lo, hi = ind_range(L.shape[1] // 2, ind_start, ind_end)
    out = []
    for i in range(lo, hi):
        others = np.flatnonzero(IDs[:, 1] == IDs[i, 1])
        others = others[others != i]
        cols = np.sort(np.concatenate((2 * others, 2 * others + 1)))

        def fit(keep):
            f, it = em(np.ascontiguousarray(L[keep][:, cols]), maf_iter, maf_tole)
            return clamp(f, len(others)), it
        out.append(individual(L, AD, i, fit, n_threshold, single_read_threshold))
    return out
