"""CPU-only: the enumerated EM inputs of tests/em_cases.py are what they claim to be, checked on the oracle -- so that a passing
comparison in tests/test_gpu_em_cases.py cannot hide a class of term or a place in a slab that the inputs never reach -- and the oracle
itself reproduces, bit for bit with NaN as NaN, what the real reference returned on them (tests/golden/em_cases.npz, made by
tests/golden/make_golden_em_cases.py)."""
import ast

import numpy as np
import pytest

import em_cases as ec

F32 = np.float32


def counts(grid, masks, big_only=True):
    big = np.array(grid["sizes"])[None, :] > 8
    return {name: int((mask & big).sum() if big_only else mask.sum()) for name, mask in masks.items()}


@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_every_class_of_term_is_there(oracle, variant):
    """Every class of s and of num is non-empty at a cell whose population has more than 8 columns (more than one buffer of the direct
    kernels), and every class of s stands at lanes 0 and 63, at the first site and at the last one."""
    grid, _ = ec.reference(oracle, variant)
    m, K = grid["cell"].shape
    assert (m, K, grid["sizes"]) == (461, 20, ec.SIZES) and len(grid["labels"]) == sum(ec.SIZES) == 342
    cls = ec.classify(ec.cell_terms(grid))
    have = counts(grid, cls)
    for name in (ec.CLASSES if variant == "hostile" else ec.FINITE_CLASSES):
        assert have[name] >= 1, (name, have)
    if variant == "finite":
        assert set(grid["reps"]) == {"s positive normal", "s positive subnormal", "s negative finite"}
        assert ((grid["f_old"] > 0) & (grid["f_old"] < 1)).all()
    else:
        assert set(grid["reps"]) == set(ec.S_CLASSES)
    big = np.array(grid["sizes"]) > 8
    for name in grid["reps"]:
        site, pop = np.nonzero(cls[name] & big[None, :])
        assert (site == 0).any() and (site == m - 1).any() and (site % 64 == 0).any() and (site % 64 == 63).any(), name
    # the frequencies the issue asks for
    if variant == "hostile":
        bits = set(grid["f_old"].view(np.uint32).ravel().tolist())
        lo, hi = ec.fc.clamp_bounds((84, 16))
        for f in [0.0, -0.0, 1.0, 1e-45, 2.0, -0.25, float("nan")] + list(lo) + list(hi):
            assert int(np.array(f, dtype=F32).view(np.uint32)) in bits, f
    # the tables say what the matrices hold
    for s, k in ((0, 0), (5, 7), (m - 1, K - 1), (64, 14)):
        i = grid["members"][k][grid["hot_col"][s, k]]
        assert grid["L"][s, 2 * i:2 * i + 2].tobytes() == grid["pairs_tab"][grid["cell"][s, k]].tobytes()
        assert grid["f_old"][k, s].tobytes() == grid["f_tab"][grid["cell"][s, k]].tobytes()
        others = np.delete(grid["members"][k], grid["hot_col"][s, k])
        ordinary = {tuple(p) for p in np.array(ec.ORDINARY, dtype=np.float64).astype(F32)}
        assert all(tuple(grid["L"][s, 2 * j:2 * j + 2]) in ordinary for j in others)
    assert list(grid["labels"][:K]) == list(range(K))          # interleaved in file order


@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_every_place_is_taken_by_a_term_that_needs_the_fixup(oracle, variant):
    """For both buffer geometries: a term whose sum is not a positive finite float32 stands in the first plain buffer at its first
    and at its last column, in a later plain buffer (the restore of the running sum), in the checked buffer with the odd tail, in the
    last column of an even population, in a population of exactly one buffer and of one buffer +- 1, and in populations of 1 and 2."""
    grid, _ = ec.reference(oracle, variant)
    bad = ec.redo(ec.cell_terms(grid))
    sizes = grid["sizes"]
    for B in ec.BUFFERS:
        seen, in_size, even_last, odd_tail = set(), set(), False, False
        for s, k in np.argwhere(bad):
            col = int(grid["hot_col"][s, k])
            place = ec.place_of(sizes[k], col, B)
            seen.add(place)
            in_size.add(sizes[k])
            even_last = even_last or (sizes[k] % 2 == 0 and col == sizes[k] - 1)
            odd_tail = odd_tail or (place == "checked buffer" and sizes[k] % 2 == 1 and sizes[k] > B)
        assert seen == set(ec.PLACES), (B, seen)
        assert {1, 2, B - 1, B, B + 1} <= in_size, (B, in_size)
        assert even_last and odd_tail, B
    # every population walks through every one of its columns, with a term that needs the fixup in each buffer it has
    for k, size in enumerate(sizes):
        assert set(grid["hot_col"][:, k]) == set(range(size))
        assert {c // 8 for c in grid["hot_col"][bad[:, k], k]} == set(range((size + 7) // 8)), size
    assert bad.sum() >= bad.size // ec.DENSE


@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_the_caps_and_the_predicted_nan_set(oracle, variant):
    """finite: no non-finite result after any update.  hostile: at most 5 % of a population's results are NaN.  And the oracle's NaN
    and infinite results of the first update are exactly those the classification of the terms predicts."""
    grid, f = ec.reference(oracle, variant)
    m, K = grid["cell"].shape
    if variant == "finite":
        assert np.isfinite(f).all()
    else:
        assert 0 < np.isnan(f[0]).sum(axis=1).max() <= m // 20
        assert np.isposinf(f[0]).any() and np.isneginf(f[0]).any() and ((f[0] == 0) & np.signbit(f[0])).any()
    assert (f[0] < 0).any() and (f[0] > 1).any() and ec.fc.subnormal(f[0]).any()
    assert len(np.unique(f[0].view(np.uint32))) > m * K // 2
    for k in range(K):
        nan, inf = ec.predicted(grid, k)
        assert np.array_equal(nan, np.isnan(f[0, k])), (k, np.flatnonzero(nan != np.isnan(f[0, k]))[:4])
        assert np.array_equal(inf, np.isinf(f[0, k])), (k, np.flatnonzero(inf != np.isinf(f[0, k]))[:4])


@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_no_cell_is_absorbed(oracle, variant):
    """Every cell stands in at least two populations, and unless all its results are non-finite they take at least two values.  Left
    out: a frequency of 0, -0.0 or 1 is a fixed point of the update for every pair with a positive sum -- every term is 0 or 1 -- and
    at the smallest subnormal the results are small multiples of it; there the comparison of the site itself has to do."""
    grid, f = ec.reference(oracle, variant)
    fixed = np.isin(np.abs(grid["f_tab"]).view(np.uint32), np.array([0.0, 1.0, 1e-45], dtype=F32).view(np.uint32))
    checked = 0
    for c in range(len(grid["f_tab"])):
        site, pop = np.nonzero(grid["cell"] == c)
        assert len(site) >= 2 and (c >= grid["n_grid"] or len(set(pop)) >= 2), c
        vals = f[0][pop, site]
        if fixed[c] or not np.isfinite(vals).any():
            continue
        checked += 1
        assert len(np.unique(vals[np.isfinite(vals)].view(np.uint32))) >= 2, (c, grid["pairs_tab"][c], grid["f_tab"][c], vals)
    assert checked >= len(grid["f_tab"]) * 3 // 4


@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_the_leave_one_out_lists(oracle, variant):
    """For every re-fit of a leave-one-out population there are sites whose term in need of the fixup is the very column it leaves out
    (the site is poisoned for the other fits only), a column of the same buffer, and a column of another buffer; one fit leaves out
    the last column.  Checked for both buffer sizes, with the classification and on the oracle's results."""
    assert ec.LOO_BATCHES == (1, 3, 4, 5) and all(s in ec.SIZES for s in ec.LOO_SIZES)
    for size in ec.LOO_SIZES:
        k = ec.SIZES.index(size)
        grid, cols, f = ec.reference_loo(oracle, variant, k)
        assert cols[1] == size - 1 and len(cols) == 5
        bad = ec.redo(ec.cell_terms(grid))[:, k]
        hot = grid["hot_col"][:, k]
        for j, c in enumerate(cols):
            assert (bad & (hot == c)).any(), (size, c)
            for B in ec.BUFFERS:
                mates, elsewhere = min(size, B * (c // B + 1)) - B * (c // B) > 1, size > B          # what the geometry has
                assert (bad & (hot != c) & (hot // B == c // B)).any() == mates and (bad & (hot // B != c // B)).any() == elsewhere, (size, c, B)
            nan, inf = ec.predicted(grid, k, c)
            assert np.array_equal(nan, np.isnan(f[0, j])) and np.array_equal(inf, np.isinf(f[0, j])), (size, c)
        if variant == "hostile":
            # a site that is finite for the fit that leaves the term out and NaN or infinite for its group mates
            own = [np.isfinite(f[0, j]) & ~np.isfinite(np.delete(f[0], j, axis=0)).any(axis=0) & (hot == c) for j, c in enumerate(cols)]
            assert all(o.sum() >= 3 for o in own), (size, [int(o.sum()) for o in own])
            assert np.isnan(f[0]).sum(axis=1).max() <= len(hot) // 20                       # the cap holds for every re-fit too
        else:
            assert np.isfinite(f).all()
        _, skips, some = ec.loo_fits(grid, k, 3)
        assert some == cols[:3] and list(grid["col_of"][skips]) == some and (grid["labels"][skips] == k).all()


def test_the_running_sum_of_negative_zero(oracle, golden):
    """negative_zero_sums: the terms are what the builder says -- half a quotient on the midpoint between -0.0 and the smallest
    subnormal, then numerators of -0.0 over positive sums -- the lead stands at every column, and the oracle, like the real reference,
    returns -0.0 at every site of every population."""
    case, f = ec.reference_zeros(oracle)
    lead = ec.terms(F32(ec.ZERO_LEAD[0]), F32(ec.ZERO_LEAD[1]), F32(ec.ZERO_F))
    rest = ec.terms(F32(ec.ZERO_REST[0]), F32(ec.ZERO_REST[1]), F32(ec.ZERO_F))
    assert lead["s"] == 1 and 0.5 * lead["q"] == -(2.0 ** -150) and F32(0.5 * lead["q"]) == 0 and np.signbit(F32(0.5 * lead["q"]))
    assert rest["s"] == F32(0.9) and rest["num"] == 0 and np.signbit(rest["num"]) and rest["q"] == 0 and np.signbit(rest["q"])
    assert not ec.redo(rest) and not ec.redo(lead)           # positive finite sums: the fixup-free loop keeps them
    m, K = case["lead_col"].shape
    assert (m, case["sizes"]) == (200, (1, 2, 8, 9, 16, 17, 24, 33))
    for k, size in enumerate(case["sizes"]):
        assert set(case["lead_col"][:, k]) == set(range(size))
        i = case["members"][k][case["lead_col"][5, k]]
        assert tuple(case["L"][5, 2 * i:2 * i + 2]) == (1.0, 0.5) and (case["L"][5, 0::2] == 1).sum() == K
    assert (f == 0).all() and np.signbit(f).all()
    g = golden("em_cases.npz")
    assert ec.digest(case) == str(g["zeros_digest"]) and g["zeros_updates"].tobytes() == f.tobytes()


@pytest.mark.parametrize("name", sorted(ec.GOLDEN))
def test_the_oracle_is_the_reference_on_the_recorded_inputs(oracle, golden, name):
    """Bit for bit, NaN as NaN: infinities, subnormals and the signs of zeros included -- one and two updates of every recorded
    population and of the five re-fits of the population of 17, and for `finite` the whole fit from 0.25 with its iteration."""
    g = golden("em_cases.npz")
    gen = ec.GOLDEN[name]
    assert ast.literal_eval(str(g[name + "_gen"])) == gen
    grid, f = ec.reference(oracle, gen["variant"], gen["sizes"])
    assert grid["L"].shape[0] == gen["m"] and ec.digest(grid) == str(g[name + "_digest"])
    k = gen["sizes"].index(ec.GOLDEN_LOO)
    _, cols, f_loo = ec.reference_loo(oracle, gen["variant"], k, gen["sizes"])
    assert list(g[name + "_loo_cols"]) == cols
    for what, mine, ref in (("update", f[:2], g[name + "_updates"]), ("leave-one-out update", f_loo[:2], g[name + "_loo_updates"])):
        bad = ec.first_difference(np.ascontiguousarray(mine), ref)
        assert bad is None, "%s %s: flat index %d: oracle %r, reference %r" % (name, what, bad, mine.ravel()[bad], ref.ravel()[bad])
        assert ec.same_nan(ref, np.ascontiguousarray(mine))
    if name == "finite":
        for kk in range(len(gen["sizes"])):
            fit, it = oracle.emMAF(ec.columns(grid["L"], grid["members"][kk]), 200, 1e-4, 1)
            assert it == int(g["finite_fit_iters"][kk]) and fit.tobytes() == g["finite_fit"][kk].tobytes(), kk
