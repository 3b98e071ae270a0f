"""--ne_obs on the enumerated inputs of tests/fisher_cases.py: the term grids (hard calls, sums above 1, frequencies of 0, 1 and
subnormal ones, u = 0, results that are infinite, NaN, subnormal or a signed zero), populations whose finite sum a frequency turns into
a signed zero, ordinary likelihoods in populations of every slab
shape, and the grid laid over a window's chunk and tail.  Every comparison is of bits, NaN equal to NaN; there is no tolerance and no
exclusion.  The yardstick is the oracle (oracle/wgs_oracle.c), which tests/test_fisher_cases_cpu.py ties to the real reference on
the grids and the signed-zero populations (tests/golden/fisher_cases.npz) and which holds the builders to what they claim; the oracle's results are computed once
per input, shared and read-only.

What runs: fisher_ind_sites_kernel per site (wgs_fisher_ind_sites), fisher_pop_kernel (fisher.fisher_obs), pairwise_leaf_kernel /
pairwise_combine_kernel with and without a carry (fisher.fisher_obs_ind, wgs_fisher_ind_sums), and fisher_window_kernel with the two
stream kernels (device.FisherStream fed from host matrices)."""
import numpy as np
import pytest

import fisher_cases as fc

pytestmark = pytest.mark.gpu
F32 = np.float32

CASES = {"finite": ("term_grid", "finite"), "hostile": ("term_grid", "hostile"), "shapes": ("population_shapes", fc.M_RESIDENT),
         "shapes_tail": ("population_shapes", fc.M_TAIL), "shapes_two": ("population_shapes", fc.M_TWO),
         "windows_finite": ("grid_in_windows", "finite"), "windows_hostile": ("grid_in_windows", "hostile"), "zeros": ("signed_zeros",)}
RESIDENT = ("finite", "hostile", "shapes", "zeros")


def case_of(oracle, name):
    return fc.reference(oracle, *CASES[name])


def equal(got, want, what, sites_last=None):
    """AssertionError naming the input, the result and the first place that is not the reference's."""
    got = np.asarray(got)
    bad = fc.first_difference(got, want)
    if bad is not None:
        where = np.unravel_index(bad, want.shape)
        n_bad = int(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).sum())
        raise AssertionError("%s: %d of %d values differ, first at %s (%s): device %r (0x%08x), reference %r (0x%08x)" % (
            what, n_bad, want.size, tuple(int(x) for x in where), sites_last or "index", got.ravel()[bad], got.view(np.uint32).ravel()[bad],
            want.ravel()[bad], want.view(np.uint32).ravel()[bad]))
    assert fc.same_nan(want, got), what


def on_device(case, lo=0, hi=None):
    """(DeviceBeagle, AFSet) of the rows [lo, hi) of a case: population slabs, site0 = lo."""
    from wgsassign_amd import device
    g, K = fc.group_of(case["IDs"])
    b = device.DeviceBeagle.from_host(np.ascontiguousarray(case["L"][lo:hi]), g, K, site0=lo)
    return b, device.AFSet.from_host(np.ascontiguousarray(case["af"][lo:hi]), ctx=b.ctx)


def runs_of(g, most):
    """[(i0, count)]: consecutive individuals of one population, at most `most` per run."""
    out, i = [], 0
    while i < len(g):
        j = i + 1
        while j < len(g) and j - i < most and g[j] == g[i]:
            j += 1
        out.append((i, j - i))
        i = j
    return out


def device_rows(case, most=4):
    """(n, m) float32: wgs_fisher_ind_sites for every individual, in runs of up to `most` of one population."""
    from wgsassign_amd import _lib
    b, afs = on_device(case)
    rows = np.full((b.n, b.m), 7.0, dtype=F32)
    for i0, count in runs_of(b.group_of, most):
        part = np.empty((count, b.m), dtype=F32)
        _lib.check(_lib.load().wgs_fisher_ind_sites(b.handle, afs.handle, i0, count, _lib.f32p(part)))
        rows[i0:i0 + count] = part
    afs.close()
    b.close()
    return rows


@pytest.mark.parametrize("name", RESIDENT)
def test_per_site_terms(oracle, golden, name):
    """Every individual's row of per-site values, which fisher_obs_ind only shows as a mean: fisher_term at every cell, the double
    product and its conversion to float32 -- and no -0.0 anywhere, because the reference ADDS its product to a zero
    (fisher_cy.pyx:65) and a kernel that stores the product keeps the sign of a negative term times a frequency of 0 or 1, of a product
    that underflows, and of the term -1.0 * (+0.0) itself."""
    case, want = case_of(oracle, name)
    got = device_rows(case)
    signed = np.argwhere(fc.negative_zeros(got))
    assert signed.size == 0, "%s: %d values of the device are -0.0, the reference has none; first: individual %d, site %d (g0, g1 = %r, af = %r)" % (
        name, len(signed), signed[0][0], signed[0][1], tuple(case["L"][signed[0][1], 2 * signed[0][0]:2 * signed[0][0] + 2]),
        case["af"][signed[0][1], fc.group_of(case["IDs"])[0][signed[0][0]]])
    equal(got, want["ne_rows"], name + ": per-site ne_ind", "individual, site")
    if name in fc.GOLDEN:                                  # ... and the rows the reference itself filled
        equal(got, golden("fisher_cases.npz")[name + "_ne_rows"], name + ": per-site ne_ind against the golden", "individual, site")
    if name == "shapes":                                     # one individual per call, and the file's last run of one population in one
        assert max(count for _, count in runs_of(fc.group_of(case["IDs"])[0], 16)) > 4
        equal(device_rows(case, 1), want["ne_rows"], name + ": per-site ne_ind, one individual per call", "individual, site")
        equal(device_rows(case, 16), want["ne_rows"], name + ": per-site ne_ind, up to 16 per call", "individual, site")


@pytest.mark.parametrize("name", RESIDENT)
def test_population_sweep(oracle, golden, name):
    """fisher_pop_kernel.  Its own signed zero -- a population's finite sum times a frequency that makes the product -0.0 -- is in
    `zeros` alone: in the grids every population holds a hard call, and its sum is already infinite or NaN wherever a frequency could
    turn the sign of a zero."""
    from wgsassign_amd import fisher
    case, want = case_of(oracle, name)
    f_obs, ne_obs = fisher.fisher_obs(case["L"], case["af"].copy(), case["IDs"], 1)
    signed = np.argwhere(fc.negative_zeros(ne_obs))
    assert signed.size == 0, "%s: %d values of ne_obs are -0.0, the reference has none; first: site %d, population %d (f_obs = %r, af = %r)" % (
        name, len(signed), signed[0][0], signed[0][1], f_obs[tuple(signed[0])], case["af"][tuple(signed[0])])
    assert not fc.negative_zeros(f_obs).any(), name
    equal(f_obs, want["f_obs"], name + ": f_obs", "site, population")
    equal(ne_obs, want["ne_obs"], name + ": ne_obs", "site, population")
    if name in fc.GOLDEN:                                  # ... and what the reference itself returned
        g = golden("fisher_cases.npz")
        assert fc.digest(case) == str(g[name + "_digest"])
        equal(f_obs, g[name + "_f_obs"], name + ": f_obs against the golden", "site, population")
        equal(ne_obs, g[name + "_ne_obs"], name + ": ne_obs against the golden", "site, population")


@pytest.mark.parametrize("name", RESIDENT)
def test_means(oracle, name):
    """np.mean on the device, on the host from downloaded rows, and in batches of one and of two individuals."""
    from wgsassign_amd import fisher
    case, want = case_of(oracle, name)
    L, af, IDs = case["L"], case["af"], case["IDs"]
    m = L.shape[0]
    with np.errstate(all="ignore"):
        for what, kw in (("device mean", {}), ("host mean", dict(host_mean=True)), ("batches of one", dict(exact_budget_bytes=4 * m)),
                         ("batches of two", dict(exact_budget_bytes=8 * m))):
            equal(fisher.fisher_obs_ind(L, af.copy(), IDs, 1, **kw), want["ne_ind"], "%s: ne_ind, %s" % (name, what), "individual")
    if name == "finite":
        assert np.isfinite(want["ne_ind"]).all()
    if name == "shapes":
        g = fc.group_of(IDs)[0]
        assert max(c for _, c in runs_of(g, 2)) == 2 and min(c for _, c in runs_of(g, 2)) == 1        # both batch sizes occur


def sums(b, afs, carry, most):
    from wgsassign_amd import _lib
    out = np.full(b.n, 7.0, dtype=F32)
    for i0, count in runs_of(b.group_of, most):
        part = np.empty(count, dtype=F32)
        c = None if carry is None else np.ascontiguousarray(carry[i0:i0 + count])
        _lib.check(_lib.load().wgs_fisher_ind_sums(b.handle, afs.handle, i0, count, _lib.f32p(c) if c is not None else None, _lib.f32p(part)))
        out[i0:i0 + count] = part
    return out


@pytest.mark.parametrize("name", ["shapes_two", "windows_finite", "windows_hostile"])
def test_continued_totals(oracle, name):
    """NumPy's running float32 total cut at site 8192: the second part continues from the first's totals (wgs_fisher_ind_sums with
    carry_in), and dividing in float64 as fisher.py does gives the whole matrix's means."""
    from wgsassign_amd import _lib
    case, want = case_of(oracle, name)
    m = case["L"].shape[0]
    b0, a0 = on_device(case, 0, fc.WINDOW)
    first = sums(b0, a0, None, 3)
    a0.close(), b0.close()
    b1, a1 = on_device(case, fc.WINDOW, m)
    total = sums(b1, a1, first, 3)
    a1.close(), b1.close()
    with np.errstate(all="ignore"):
        cut = (total.astype(np.float64) / m).astype(F32)
    b, a = on_device(case)
    whole = np.full(b.n, 7.0, dtype=F32)
    for i0, count in runs_of(b.group_of, 5):
        part = np.empty(count, dtype=F32)
        _lib.check(_lib.load().wgs_fisher_ind_means(b.handle, a.handle, i0, count, _lib.f32p(part)))
        whole[i0:i0 + count] = part
    a.close(), b.close()
    equal(whole, want["ne_ind"], name + ": wgs_fisher_ind_means of the whole matrix", "individual")
    equal(cut, want["ne_ind"], name + ": totals continued at site 8192", "individual")
    # the first part alone is np.add.reduce of the first 8192 values of every row
    equal(first, np.array([np.add.reduce(r[:fc.WINDOW]) for r in want["ne_rows"]], dtype=F32), name + ": totals of the first chunk", "individual")


WINDOWED = [("shapes_tail", 8192, 2), ("shapes_two", 16384, 1), ("shapes_two", 8192, 2), ("windows_finite", 8192, 2), ("windows_hostile", 8192, 2)]


@pytest.mark.parametrize("name, window, windows", WINDOWED)
def test_windowed_sweep(oracle, name, window, windows):
    """fisher_window_kernel on slabs of 1 .. 17 pairs -- every npairs % 4 on a trip after the first, odd and even last columns -- and on
    the grid's special values in a chunk's leaves and in the tail: the rows of f_obs and ne_obs, the per-individual means of finish(),
    and the column means continued from window to window."""
    from wgsassign_amd import device, fisher
    case, want = case_of(oracle, name)
    m = case["L"].shape[0]
    g, K = fc.group_of(case["IDs"])
    st = device.FisherStream(len(g), K, m)
    f_obs, ne_obs, running = np.full((m, K), 7.0, dtype=F32), np.full((m, K), 7.0, dtype=F32), None
    with np.errstate(all="ignore"):
        for lo in range(0, m, window):
            hi = min(m, lo + window)
            b, a = on_device(case, lo, hi)
            f_obs[lo:hi], ne_obs[lo:hi] = st.push(b, a)
            a.close(), b.close()
            running = fisher.continue_column_sum(running, ne_obs[lo:hi])
        ne_ind = st.finish()
        assert st.windows == windows
        st.close()
        mean, want_mean = fisher.column_mean(running, m), np.mean(want["ne_obs"], axis=0)
    what = "%s in windows of %d" % (name, window)
    assert not fc.negative_zeros(ne_obs).any(), what
    equal(f_obs, want["f_obs"], what + ": f_obs", "site, population")
    equal(ne_obs, want["ne_obs"], what + ": ne_obs", "site, population")
    equal(ne_ind, want["ne_ind"], what + ": ne_ind", "individual")
    equal(mean, want_mean, what + ": np.mean(ne_obs, axis=0)", "population")
