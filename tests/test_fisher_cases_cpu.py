"""CPU-only: the enumerated --ne_obs inputs of tests/fisher_cases.py are what they claim to be, checked on the oracle -- so that a
passing comparison in tests/test_gpu_fisher_cases.py cannot hide a place the inputs never reach -- and the oracle itself reproduces,
bit for bit with NaN as NaN, what the real reference returned on the two term grids and the signed-zero populations (tests/golden/fisher_cases.npz, made by
tests/golden/make_golden_fisher_cases.py): its infinities, NaNs, subnormals and the sign of its zeros."""
import ast

import numpy as np
import pytest

import fisher_cases as fc

F32 = np.float32
reference = fc.reference


def classes(want):
    """Masks over the (n, m) per-site cells, by what the reference makes of them."""
    f, ne = want["f_rows"], want["ne_rows"]
    with np.errstate(invalid="ignore"):
        return {"+inf": np.isposinf(f), "-inf": np.isneginf(f), "nan": np.isnan(f), "negative": np.isfinite(f) & (f < 0),
                "subnormal": fc.subnormal(ne), "zero of a negative": np.isfinite(f) & (f < 0) & (ne == 0)}


CLASSES_OF = {"finite": ("negative", "subnormal", "zero of a negative"),
              "hostile": ("+inf", "-inf", "nan", "negative", "subnormal", "zero of a negative")}


def test_the_finite_grid_is_finite_and_still_has_its_hard_cells(oracle):
    grid, want = reference(oracle, "term_grid", "finite")
    assert ((grid["af"] > 0) & (grid["af"] < 1)).all()
    for name, a in want.items():
        assert np.isfinite(a).all(), name
    cls = classes(want)
    assert cls["subnormal"].sum() >= 1 and cls["negative"].sum() >= 1 and cls["zero of a negative"].sum() >= 1
    assert not fc.negative_zeros(want["ne_rows"]).any() and not fc.negative_zeros(want["ne_obs"]).any()
    assert len(grid["pairs"]) == len(fc.PAIRS) - len(fc.NOT_FINITE_INSIDE) and len(grid["freqs"]) == len(fc.FREQS) - 4


def test_the_hostile_grid_holds_every_class_and_stays_under_its_cap(oracle):
    grid, want = reference(oracle, "term_grid", "hostile")
    cls = classes(want)
    for name in CLASSES_OF["hostile"]:
        assert cls[name].sum() >= 1, name
    # the sign of a zero: negative terms times a frequency of 0 or 1, products that underflow, and the term -1.0 * (+0.0) itself
    with np.errstate(invalid="ignore"):
        assert fc.negative_zeros(want["f_rows"] * F32(0)).any()              # ... a kernel that stores the product has -0.0 to store
    assert not fc.negative_zeros(want["ne_rows"]).any() and not fc.negative_zeros(want["ne_obs"]).any()
    assert not fc.negative_zeros(want["f_rows"]).any() and not fc.negative_zeros(want["f_obs"]).any()
    # inf - inf inside one population's serial sum
    pop_of, K = grid["pop_of"], len(grid["freqs"])
    both = [(k, s) for k in range(K) for s in np.flatnonzero(cls["+inf"][pop_of == k].any(axis=0) & cls["-inf"][pop_of == k].any(axis=0))]
    assert both and all(np.isnan(want["f_obs"][s, k]) for k, s in both)
    # the cap: at most one site in four is not finite, for any population and either result
    m = grid["L"].shape[0]
    for name in ("f_obs", "ne_obs"):
        worst = (~np.isfinite(want[name])).sum(axis=0).max()
        assert 0 < worst <= m // 4, (name, worst, m)
    # the base grid alone, as counted when it was first tried: 9 infinite and 6 NaN terms in its 13 x 12 cells
    base = np.isin(grid["pair_of"], np.arange(len(fc.PAIRS_BASE)))
    site_of = [int(np.flatnonzero(grid["freq_of"][:, 0] == f)[0]) for f in range(len(fc.FREQS_BASE))]
    cells = want["f_rows"][base & (pop_of == 0)][:, site_of]
    assert cells.shape == (13, 12) and np.isinf(cells).sum() == 9 and np.isnan(cells).sum() == 6


@pytest.mark.parametrize("variant", fc.VARIANTS)
def test_every_cell_of_the_grid_stands_at_every_kind_of_place(oracle, variant):
    grid, want = reference(oracle, "term_grid", variant)
    m = grid["L"].shape[0]
    assert m == 197 and grid["af"].shape == (m, len(grid["freqs"])) and grid["L"].shape[1] == 2 * len(grid["pairs"]) * len(grid["freqs"])
    pops, counts = np.unique(grid["IDs"][:, 1], return_counts=True)
    assert len(pops) == len(grid["freqs"]) and (counts == len(grid["pairs"])).all() and len(grid["pairs"]) % 2 == 1
    assert len(set(grid["IDs"][:len(pops), 1])) == len(pops)                       # interleaved in file order
    for i in (0, 1, len(pops), len(grid["pair_of"]) - 1):                          # the tables say what the matrices hold
        assert tuple(grid["L"][5, 2 * i:2 * i + 2]) == tuple(grid["pairs"][grid["pair_of"][i]])
        assert grid["af"][5, grid["pop_of"][i]].tobytes() == grid["freqs"][grid["freq_of"][5, grid["pop_of"][i]]].tobytes()
    for p in range(len(grid["pairs"])):
        for f in range(len(grid["freqs"])):
            places = fc.cell_places(grid, p, f)
            sites = np.concatenate([s for _, _, s in places])
            assert 0 in sites and m - 1 in sites and (sites % 64 == 0).any() and (sites % 64 == 63).any(), (p, f)
            assert {c % 2 for _, c, _ in places} == {0, 1}, (p, f)
    # and so every class does: spelled out on the reference's own rows
    cls = classes(want)
    for name in CLASSES_OF[variant]:
        ind, site = np.nonzero(cls[name])
        assert (site == 0).any() and (site == m - 1).any() and (site % 64 == 0).any() and (site % 64 == 63).any(), name
        assert {int(c) % 2 for c in grid["col_of"][ind]} == {0, 1}, name


def test_population_shapes(oracle):
    case = fc.population_shapes(fc.M_RESIDENT)
    sizes = np.array(fc.SIZES)
    assert tuple(np.unique(case["IDs"][:, 1], return_counts=True)[1]) == fc.SIZES == (1, 2, 3, 4, 5, 7, 8, 9, 11, 14, 15, 16, 17, 27, 33)
    npairs = (sizes + 1) // 2
    assert set(npairs % 4) == {0, 1, 2, 3} and set((npairs + 3) // 4) == {1, 2, 3, 4, 5} and set(sizes % 2) == {0, 1}
    later = npairs > 4                                       # a last trip after the first, of 1, 2, 3 and 4 pairs
    assert set(npairs[later] % 4) == {0, 1, 2, 3} and set(sizes[later] % 2) == {0, 1}
    labels = case["labels"]
    assert list(labels[:15]) == list(range(15)) and (labels[-6:] == 14).all()           # interleaved; the largest ends with a run
    lo, hi = fc.clamp_bounds(fc.SIZES)
    af = case["af"]
    assert ((af >= lo) & (af <= hi)).all() and af.dtype == F32
    for k in range(len(sizes)):
        assert (af[k::7, k] == lo[k]).sum() >= len(af[k::7]) - 3 and (af[k + 3::11, k] == hi[k]).all()
    assert (fc.M_RESIDENT, fc.M_TAIL, fc.M_TWO) == (197, 8392, 16384)
    _, want = reference(oracle, "population_shapes", fc.M_RESIDENT)
    for name, a in want.items():
        assert np.isfinite(a).all(), name
    assert (want["ne_ind"] > 0).all()


@pytest.mark.parametrize("variant", fc.VARIANTS)
def test_the_grid_in_windows_falls_where_it_should(oracle, variant):
    case, want = reference(oracle, "grid_in_windows", variant)
    m, labels, col_of = case["L"].shape[0], case["labels"], case["col_of"]
    assert m == 8192 + 200 and tuple(np.bincount(labels)) == (3, 9) and list(labels[:6]) == [0, 1, 0, 1, 0, 1]
    cls = classes(want)
    second_trip = (labels == 1) & (col_of == 8)
    assert second_trip.sum() == 1
    for name in CLASSES_OF[variant]:
        ind, site = np.nonzero(cls[name])
        assert (site % 128 == 0).any() and (site % 128 == 127).any(), name                  # the first and last site of a leaf
        assert (site % 128 == 63).any() and (site % 128 == 64).any(), name                  # where its two tiles meet
        assert (site < 8192).any() and (site >= 8192).any(), name          # the chunk and the tail
        assert second_trip[ind].any() and (col_of[ind] % 2 == 0).any() and (col_of[ind] % 2 == 1).any(), name
        assert {int(k) for k in labels[ind]} == {0, 1}, name
    special = np.zeros_like(cls["nan"])
    for name in (("+inf", "-inf", "nan") if variant == "hostile" else ("subnormal", "zero of a negative", "negative")):
        special |= cls[name]
    for k in (0, 1):
        assert special[labels == k][:, 8191].any() and special[labels == k][:, 8192].any(), k
    if variant == "hostile":
        assert tuple(case["freqs"][case["freq_at"][8191]]) == (0.0, 1.0) and case["freqs"][case["freq_at"][8192, 0]] == 1.0
        assert tuple(np.flatnonzero(case["hot"])) == tuple(np.flatnonzero(((labels == 0) & (col_of == 2)) | ((labels == 1) & np.isin(col_of, (1, 4, 8)))))
        assert np.isfinite(want["ne_ind"][~case["hot"]]).all() and not np.isfinite(want["ne_ind"][case["hot"]]).any()
        assert np.isfinite(want["ne_rows"][~case["hot"]]).all()
        for name in ("f_obs", "ne_obs"):
            assert 0 < (~np.isfinite(want[name])).sum(axis=0).max() <= m // 4, name
        assert not np.isfinite(want["ne_rows"][:, :8192]).all() and not np.isfinite(want["ne_rows"][:, 8192:]).all()
    else:
        for name, a in want.items():
            assert np.isfinite(a).all(), name
    assert not fc.negative_zeros(want["ne_rows"]).any() and not fc.negative_zeros(want["ne_obs"]).any()
    with np.errstate(invalid="ignore"):
        assert fc.negative_zeros(want["f_rows"] * F32(0)).any()


def test_the_signed_zeros_come_from_finite_population_sums(oracle):
    """fisher_pop_kernel's own signed zero: ne_obs == +0 where the population's sum is a finite number of the sign that the frequency
    turns into a product of -0.0 -- negative at 0 and at 1, negative and so small that the product underflows, positive at -0.0."""
    case, want = reference(oracle, "signed_zeros")
    m, labels, own = case["L"].shape[0], case["labels"], case["own"]
    assert m == fc.M_ZEROS == 198 and tuple(np.bincount(labels)) == case["sizes"] == (3, 4, 2, 5) and list(labels[:8]) == [0, 1, 2, 3] * 2
    for name, a in want.items():                             # nothing hides: every sum, row and mean is finite
        assert np.isfinite(a).all(), name
    f_obs, ne_obs, af = want["f_obs"], want["ne_obs"], case["af"]
    stored = fc.stored_product(f_obs, af)                    # what a kernel without the reference's addition would store
    minus = fc.negative_zeros(stored)
    assert np.array_equal(np.where(minus, F32(0), stored).view(np.uint32), ne_obs.view(np.uint32))      # ... and differs in nothing else
    assert not fc.negative_zeros(ne_obs).any() and not fc.negative_zeros(want["ne_rows"]).any()
    sites = np.arange(m)
    for k, (what, _, z) in enumerate(fc.ZERO_POPULATIONS):
        s = sites[own[:, k]]
        assert (af[s, k].view(np.uint32) == np.array(z, dtype=F32).view(np.uint32)).all(), what
        assert minus[s, k].all() and (ne_obs[s, k] == 0).all(), what
        assert ((f_obs[s, k] > 0) if what.startswith("positive") else (f_obs[s, k] < 0)).all(), what
        assert 0 in s and m - 1 in s and (s % 64 == 0).any() and (s % 64 == 63).any() and len(s) >= 10, what
        at_lane_0 = set(af[sites % 64 == 0, k].view(np.uint32).tolist())                             # every zeroing frequency at lane 0
        assert at_lane_0 == set(np.array(fc.ZERO_FREQS, dtype=np.float64).astype(F32).view(np.uint32).tolist()), what
    assert abs(f_obs[own[:, 2], 2]).max() < 0.1               # the product that underflows: half of it times 1.4e-45 is below 0.7e-45
    # the rows: every individual of a population has its signed zeros too
    g = fc.group_of(case["IDs"])[0]
    rows = fc.negative_zeros(fc.stored_product(want["f_rows"], af[:, g].T))
    assert (rows.sum(axis=1) >= 10).all()
    assert {int(c) % 2 for c in case["col_of"]} == {0, 1} and set((np.array(case["sizes"]) + 1) // 2) == {1, 2, 3}


@pytest.mark.parametrize("name", sorted(fc.GOLDEN))
def test_the_oracle_is_the_reference_on_the_recorded_inputs(oracle, golden, name):
    """Bit for bit, NaN as NaN: infinities, subnormals and the signs of zeros included."""
    g = golden("fisher_cases.npz")
    builder, gen = fc.GOLDEN[name]
    assert ast.literal_eval(str(g[name + "_gen"])) == gen
    case, want = reference(oracle, builder, *[v for k, v in gen.items() if k != "m"])
    assert case["L"].shape[0] == gen["m"] and fc.digest(case) == str(g[name + "_digest"])
    for what, a in want.items():
        ref = g[name + "_" + what]
        bad = fc.first_difference(a, ref)
        assert bad is None, "%s %s: flat index %d: oracle %r, reference %r" % (name, what, bad, a.ravel()[bad], ref.ravel()[bad])
        assert fc.same_nan(ref, a)
        assert not fc.negative_zeros(ref).any(), what
