"""Drop-in for the reference's Cython module `zscore_cy` (zscore_cy.pyx), backed by HIP: same arguments and in-place semantics
(W_l_obs_array / W_l_array / var_W_l_array are ACCUMULATED into), for inputs the reference handles in seconds -- uploads, runs the
device path of wgsassign_amd/zscore.py for the one individual, downloads.  `t` is accepted and ignored."""
import numpy as np

from . import zscore
from .device import AFSet, DeviceBeagle


def _site_values(L, L_keep, A, AD, AD_array, AD_factorial, AD_like, AD_index, i):
    L = np.ascontiguousarray(L, dtype=np.float32)
    m, n = L.shape
    n //= 2
    b = DeviceBeagle.from_host(L)
    depth = zscore.DepthTable(b, np.ascontiguousarray(AD, dtype=np.int32))
    comp = np.full((1, zscore.N_CLASSES), -1, dtype=np.int32)
    tabs = np.zeros((1, zscore.N_CLASSES, 6), dtype=np.float32)
    for d in np.unique(AD_array[:, 0] + AD_array[:, 1]):
        for a in range(int(d) + 1):
            r = AD_index[a, int(d) - a]
            tabs[0, zscore.class_index(int(d) - a, a)] = np.concatenate((AD_like[r], AD_factorial[r]))
    # the caller chose the sites: every site's class is marked kept with a mean that equals its own value is not expressible per
    # site, so the mask is made wide open for the classes and narrowed to L_keep on the host
    for Ar, Aa in AD_array[:, :2]:
        comp[0, zscore.class_index(int(Ar), int(Aa))] = 0
    mean = np.full((1, zscore.N_CLASSES), np.nan, dtype=np.float32)       # |NaN - g| > 0.01 is false: every site of a listed class is kept
    keep = zscore.KeepSet(depth, int(i), mean, comp)
    sites = keep.sites(0)
    full = np.zeros(m, dtype=np.float32)
    full[np.asarray(L_keep)] = np.asarray(A, dtype=np.float32)
    afs = AFSet.from_host(full.reshape(-1, 1))
    wobs, wl, var = keep.stats(tabs, [afs.col_dev(0)])
    pos = np.searchsorted(sites, np.asarray(L_keep))
    if len(sites) == 0 or np.any(pos >= len(sites)) or np.any(sites[pos] != np.asarray(L_keep)):
        raise ValueError("L_keep holds sites whose depth pair is not in AD_array")
    out = wobs[0][pos], wl[0][pos], var[0][pos]
    for o in (afs, keep, depth, b):
        o.close()
    return out


def expected_W_l(L, L_keep, A, AD, AD_array, AD_factorial, AD_like, AD_index, t, i, W_l_obs_array, W_l_array):
    """zscore_cy.pyx:10-33."""
    wobs, wl, _ = _site_values(L, L_keep, A, AD, AD_array, AD_factorial, AD_like, AD_index, i)
    W_l_obs_array += wobs
    W_l_array += wl


def variance_W_l(L, L_keep, A, AD, AD_array, AD_factorial, AD_like, AD_index, t, i, var_W_l_array, W_l_array):
    """zscore_cy.pyx:36-57 (W_l_array: what expected_W_l left, recomputed here on the device)."""
    _, _, var = _site_values(L, L_keep, A, AD, AD_array, AD_factorial, AD_like, AD_index, i)
    var_W_l_array += var
