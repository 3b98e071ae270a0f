"""CPU-only: the enumerated scoring inputs of tests/score_cases.py are what they claim to be, checked on the oracle -- so that a passing
comparison in tests/test_gpu_score_cases.py cannot hide a class of likelihood sum, a place in a tile, a slab or a part, or a kind of
cell that the inputs never reach -- and the oracle itself reproduces, bit for bit with NaN as NaN, what the real reference returned
on them (tests/golden/score_cases.npz, made by tests/golden/make_golden_score_cases.py).  The counts are printed (pytest -s)."""
import ast
import math

import numpy as np
import pytest

import score_cases as sc

F32 = np.float32
# the kernel configurations of tests/test_gpu_score_cases.py: the first K populations with shared columns (sweep, coded sweep,
# assign_kernel, chains), and K populations through the per-individual permutation
SHARED_K = (1, 4, 5, 6, 7, 8, 9, 10, 13, 20, 23)
PER_IND_K = (4, 5, 10)


def bits(x):
    return int(np.array(x, dtype=np.float64).astype(F32).view(np.uint32))


@pytest.mark.parametrize("shape", sc.SHAPES)
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_the_layout(variant, shape):
    """The shapes, the slabs, the rotation: every pair of an individual's family meets every frequency of a population's family, in
    every cell; the values the families were asked to hold are there."""
    c = sc.case_of(variant, shape)
    m, n = c["L"].shape[0], c["L"].shape[1] // 2
    assert (m, n, c["A"].shape) == ({"grid": 197, "block": 4096 + 64 + 5}[shape], 52, (m, 23))
    assert c["sizes"] == (1, 2, 5, 8, 9, 11, 16) and list(c["labels"][:7]) == list(range(7))         # interleaved in file order
    assert len(c["sizes"]) >= 5 and {1, 2} <= set(c["sizes"]) and any(s % 2 for s in c["sizes"][2:]) and any(s % 2 == 0 for s in c["sizes"][2:])
    live = c["t_of"] >= 0
    assert live.sum() == {"grid": 197, "block": 1251}[shape]
    products = sc.family_products(c)
    short = {key: val for key, val in products.items() if val[0] != val[1]}
    print("%s/%s: %d (pair family, frequency family) products, every one complete in every cell: %d pairs x frequencies" % (
        variant, shape, len(products), sum(v[1] for v in products.values())))
    assert not short, short
    assert sc.STEP >= max(len(f) for f in sc.PAIR_FAMILIES.values()) and live.sum() // sc.STEP >= max(len(f) for f in sc.FREQ_FAMILIES.values())
    # the rotation the issue's prototype warns of would drop products: s * 3 % 5 against s * 5 % 10 meets 10 of 50
    assert len({(s * 3 % 5, s * 5 % 10) for s in range(m)}) < 50
    # offsets differ per individual and per population: no two individuals of a family (populations of a family) are in step
    for fam in set(c["pair_family"]):
        mine = [i for i in range(n) if c["pair_family"][i] == fam]
        assert len({int(c["pair_index"][live, i][0]) for i in mine}) == min(len(mine), len(sc.PAIR_FAMILIES[fam])), fam
    # neutral sites: (1, 0) at a = 0, whose term is exactly 0
    if shape == "block":
        assert (c["L"][~live, 0::2] == 1).all() and (c["L"][~live, 1::2] == 0).all() and (c["A"][~live] == 0).all() and not np.signbit(c["A"][~live]).any()
        tile, lane = np.arange(m) // 64, np.arange(m) % 64
        assert live[np.isin(tile, (0, 63, 64, 65))].all() and live[lane == 0].all() and live[lane >= 48].all()
    # what the pairs and frequencies have to hold
    have_p = {(bits(a), bits(b)) for i in range(n) for a, b in zip(c["L"][live, 2 * i], c["L"][live, 2 * i + 1])}
    have_f = set(c["A"][live].view(np.uint32).ravel().tolist())
    pairs = [(1, 0), (0, 1), (0, 0), (0.999, 0.001), (1 - 2.0 ** -24, 2.0 ** -24), (0.333333, 0.333333), (0.941176, 0.058824)]
    freqs = [0.0, 1.0, 0.5, 2.0 ** -24, 1 - 2.0 ** -24, 2.0 ** -12, 1e-30, 1e-40] + [x for nn in (1, 42, 2000) for x in (1 / (2 * (nn + 1)), 1 - 1 / (2 * (nn + 1)))]
    if variant == "hostile":
        inf, nan = math.inf, math.nan
        pairs += [(-0.0, 0.0), (0.0, -0.0), (1e-40, 0), (-1e-40, 0), (0, -1e-40), (1e-30, 1e-30), (0.75, 0.75), (-0.25, 0.5), (1e20, 0), (3e38, 0), (3e38, 3e38),
                  (inf, 0), (-inf, 0), (inf, -inf), (nan, 0), (0, nan)]
        freqs += [-0.0, -1e-40, -0.25, 1 + 2.0 ** -23, 1.5, 2.0, 1e20, -1e20, 3e38, inf, -inf, nan]
    for a, b in pairs:
        assert (bits(a), bits(b)) in have_p, (a, b)
    for f in freqs:
        assert bits(f) in have_f, f
    if variant == "finite":
        assert ((c["A"] >= 0) & (c["A"] <= 1)).all() and ((c["L"] >= 0) & (c["L"] <= 1)).all()


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_the_classes_of_s_that_are_reached(variant):
    """Computed, not claimed: which classes of s = (like0 + like1) + like2 the inputs reach.  -0 is reached by nothing here: like0 + like1
    is -0 only when both are, and then like2 = (1 - g0 - g1) a^2 is +0 or positive unless a is NaN -- so no input is invented for it."""
    for shape in sc.SHAPES:
        counts = sc.class_counts(sc.case_of(variant, shape))
        print("%s/%s terms per class of s: %r" % (variant, shape, counts))
        want = set(sc.S_CLASSES) - {"-0"} if variant == "hostile" else {"positive normal <= 1", "positive subnormal", "+0", "negative normal"}
        assert {name for name, cnt in counts.items() if cnt > 0} == want, counts
    # -0 over the whole product of all pairs and all frequencies, not only the products the layout pairs up
    pairs = np.array([p for fam in sc.PAIR_FAMILIES.values() for p in fam], dtype=np.float64).astype(F32)
    freqs = np.array([f for fam in sc.FREQ_FAMILIES.values() for f in fam], dtype=np.float64).astype(F32)
    s = sc.like_sum(pairs[:, None, 0], pairs[:, None, 1], freqs[None, :])
    assert not ((s == 0) & np.signbit(s)).any()


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_every_class_stands_at_every_place(variant):
    """Every reachable class of s: in both halves of a wave's pair and in all four columns of a quad, in the first and the last column
    of a slab, at lanes 0 and 63 of a tile, in the last live lane of the ragged tile, in the first and the last tile of a block and
    behind the block edge, and in the last 16-, 8- and 4-SNP batch of a tile (the end of a part of the coded sweep, wherever the
    parts are cut)."""
    reach = sc.reachable(variant)
    for shape in sc.SHAPES:
        c = sc.case_of(variant, shape)
        m, n = c["L"].shape[0], c["n_grid"]
        cls = sc.classify(sc.sums_of(c))[:, :n]                         # (m, n, K)
        site, col = np.arange(m), c["col_of"][:n]
        size = np.array(c["sizes"])[c["labels"][:n]]
        tile, lane = site // 64, site % 64
        end = np.where(tile == (m - 1) // 64, m - tile * 64, 64)
        where_site = {"lane 0": lane == 0, "lane 63": lane == 63, "last live lane of the ragged tile": site == m - 1, "first tile": tile == 0,
                      "last tile of a block": (tile % 64 == 63) | (tile == (m - 1) // 64), "ragged tile": tile == (m - 1) // 64}
        for b in (16, 8, 4):
            where_site["last %d-SNP batch of a tile" % b] = lane >= ((end - 1) // b) * b
        if shape == "block":
            where_site["first tile behind the block edge"] = tile == 64
        where_ind = {"pair half 0": col % 2 == 0, "pair half 1": col % 2 == 1, "first column of a slab": col == 0, "last column of a slab": col == size - 1,
                     "last column of an odd slab": (col == size - 1) & (size % 2 == 1)}
        for q in range(4):
            where_ind["quad column %d" % q] = col % 4 == q
        table = {}
        for cnum in reach:
            hit = (cls == cnum).any(axis=2)                             # (m, n): the class in any population
            for name, mask in where_site.items():
                table[(sc.S_CLASSES[cnum], name)] = int(hit[mask].sum())
            for name, mask in where_ind.items():
                table[(sc.S_CLASSES[cnum], name)] = int(hit[:, mask].sum())
        for cnum in reach:
            print("%s/%s %-22s %s" % (variant, shape, sc.S_CLASSES[cnum], ", ".join("%s %d" % (name, cnt) for (cl, name), cnt in table.items() if cl == sc.S_CLASSES[cnum])))
        missing = [key for key, cnt in table.items() if cnt == 0]
        assert not missing, missing


def configurations(case, V):
    """name -> (n, K) cell kinds of every kernel configuration of the GPU tests."""
    kinds = sc.cell_kinds(V)
    n = case["n_grid"]
    out = {"shared columns, K = %d" % K: kinds[:, :K] for K in SHARED_K}
    for K in PER_IND_K:
        out["per-individual columns, K = %d" % K] = np.stack([kinds[i, sc.permutation(i, K)] for i in range(n)])
    return out


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_the_kinds_of_cell(oracle, variant):
    """From the oracle's per-site values: at least half of all cells are finite; in `hostile` every kernel configuration sees at least 8
    cells whose only non-finite class is -inf, 8 with +inf and 8 with NaN; the individuals of the family with NaN pairs, which
    poison all their cells, are a minority (2 of 52).  `finite` has what Beagle-like data has: -inf from hard calls at a = 0 or 1, NaN
    from a pair that sums above 1 at a = 1, never +inf."""
    for shape in sc.SHAPES:
        c, V = sc.reference(oracle, variant, shape)
        kinds = sc.cell_kinds(V)
        total = {name: int((kinds == j).sum()) for j, name in enumerate(sc.CELL_KINDS)}
        print("%s/%s cells by kind: %r of %d" % (variant, shape, total, kinds.size))
        assert 2 * total["finite"] >= kinds.size, total
        for name, k in configurations(c, V).items():
            cnt = [int((k == j).sum()) for j in range(5)]
            print("    %-34s finite %4d, -inf only %3d, +inf only %3d, NaN only %3d, mixed %3d" % (name, *cnt))
            if variant == "hostile":
                assert min(cnt[1:4]) >= 8, (name, cnt)
            else:
                assert cnt[2] == 0 and (cnt[1] >= 8 or name.endswith("K = 1")), (name, cnt)
        nan_people = [i for i in range(c["n_grid"]) if c["pair_family"][i] == "infnan"]
        assert len(nan_people) == (2 if variant == "hostile" else 0) and all((kinds[i] >= 3).all() for i in nan_people)
        pos = V[np.isfinite(V)] > 0
        print("    positive per-site values (s > 1): %d" % int(pos.sum()))
        assert pos.any() == (variant == "hostile")


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_the_sums_of_the_finite_cells_are_exact_in_any_order(oracle, variant):
    """For every finite cell over the whole matrix -- hence over every tile, block and part of it -- sum |v| < 2^53 u with u the ulp of the
    smallest non-zero |v|: all partial sums are multiples of u below 2^53 u, so float64 addition is exact in any order and the expected
    sum is math.fsum of the float32 values, which is also what np.sum(vec, dtype=float) of the reference gives.  The cap on cells that
    fail is zero."""
    for shape in sc.SHAPES:
        c, V = sc.reference(oracle, variant, shape)
        kinds = sc.cell_kinds(V)
        want = sc.expected_sums(V)
        failing, checked, tightest = [], 0, math.inf
        for i, k in np.argwhere(kinds == 0):
            total, cap = sc.exact_sum_margin(V[i, k])
            checked += 1
            tightest = min(tightest, cap / total if total else math.inf)
            if not total < cap:
                failing.append((c["pair_family"][i], c["freq_family"][k], total, cap))
            assert want[i, k] == np.sum(V[i, k], dtype=float) and math.isfinite(want[i, k])
        print("%s/%s: %d finite cells, %d outside the exactness bound, the tightest has 2^53 u = %.1f x its sum |v|" % (variant, shape, checked, len(failing), tightest))
        assert not failing, failing[:5]
        with np.errstate(all="ignore"):
            assert sc.same_bits64(want, np.sum(V.astype(np.float64), axis=-1))        # the non-finite cells: the sign of the infinity, NaN


def test_the_ragged_shape_has_its_terms_in_the_ragged_tile_only(oracle):
    """score_cases.RAGGED: 192 neutral sites and five term sites, so every non-finite cell owes it to the ragged tile alone -- at least
    8 cells of each kind in every configuration that runs it (K = 6, 7, 23 shared, 4 per individual), most cells finite."""
    for variant in sc.VARIANTS:
        c, V = sc.reference(oracle, variant, sc.RAGGED)
        assert c["L"].shape[0] == 197 and list(np.flatnonzero(c["t_of"] >= 0)) == [192, 193, 194, 195, 196]
        assert not V[:, :, :192].any() and not np.signbit(V[:, :, :192]).any()
        kinds = sc.cell_kinds(V)
        configs = {"K = %d" % K: kinds[:, :K] for K in (5, 6, 7, 23)}
        configs["per individual, K = 4"] = np.stack([kinds[i, sc.permutation(i, 4)] for i in range(52)])
        for name, k in configs.items():
            cnt = [int((k == j).sum()) for j in range(5)]
            print("%s/ragged %-22s finite %4d, -inf only %3d, +inf only %3d, NaN only %3d, mixed %3d" % (variant, name, *cnt))
            assert 2 * cnt[0] >= k.size and cnt[1] >= 8 and (variant == "finite" or min(cnt[2], cnt[3]) >= 8), (variant, name, cnt)
        for i, k in np.argwhere(kinds == 0):
            total, cap = sc.exact_sum_margin(V[i, k])
            assert total < cap


def test_the_classes_per_snp_fit_a_table_of_sixteen_snps():
    """The coded sweep takes 16 SNPs per table while 16 x the 99th percentile of the classes per SNP stays within 616 rows
    (codes.hip: wgs_beagle_codes_plan): every site of these cases has at most 38 distinct pairs."""
    for variant in sc.VARIANTS:
        for shape in sc.SHAPES:
            cl = sc.classes_per_snp(sc.case_of(variant, shape)["L"])
            print("%s/%s classes per SNP: most %d, mean %.1f" % (variant, shape, cl.max(), cl.mean()))
            assert cl.max() * 16 <= 616


def test_an_extra_slab_raises_the_classes_per_snp():
    """build(extra=...): more individuals with a pair of their own each, at every site (36: a table of 8 SNPs; 48: of 4) or at chosen
    sites only (more classes there than the encoder's 64-slot tables hold: those SNPs stay uncoded, the others are untouched)."""
    for extra, lo, hi in ((36, 616 / 16, 616 / 8), (48, 616 / 8, 88)):
        c = sc.build("hostile", "grid", extra=extra)
        cl = sc.classes_per_snp(c["L"])
        assert c["L"].shape[1] == 2 * (52 + extra) and c["sizes"][-1] == extra and lo < cl.min() and cl.max() <= hi, (extra, cl.min(), cl.max())
    for variant in sc.VARIANTS:
        for shape in sc.SHAPES:
            at = sc.uncoded_sites(shape)
            base = sc.case_of(variant, shape)
            u = sc.build(variant, shape, extra=48, extra_at=at)
            cl, cl0 = sc.classes_per_snp(u["L"]), sc.classes_per_snp(base["L"])
            rest = np.setdiff1d(np.arange(len(cl)), at)
            assert (cl[at] > 56).all() and (cl[rest] <= cl0[rest] + 1).all() and (cl[rest] * 16 <= 616).all()
            assert u["L"][:, :104].tobytes() == base["L"].tobytes() and u["A"].tobytes() == base["A"].tobytes()
            # the uncoded sites carry a term of every reachable class, in both halves of a pair and in both pairs of a quad
            cls = sc.classify(sc.sums_of(u))[at][:, :52]
            for cnum in sc.reachable(variant):
                cols = {int(x) % 4 for x in base["col_of"][np.nonzero((cls == cnum).any(axis=(0, 2)))[0]]}
                assert cols == {0, 1, 2, 3}, (variant, shape, sc.S_CLASSES[cnum], cols)
            # a grid's 12 of 197 raise the 99th percentile over a table of 16 SNPs; a block's 11 of 4165 do not
            assert sc.table_snps(u["L"]) == {("finite", "grid"): 8, ("hostile", "grid"): 4}.get((variant, shape), 16)
            assert sc.table_snps(base["L"]) == 16


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_the_oracle_is_the_reference_on_the_recorded_inputs(oracle, golden, variant):
    """Bit for bit, NaN as NaN: glassy_cy.loglike into zeros and into the non-zero start vectors, glassy.assignLL, and
    utils.partition_loglikes for P = 1, 3 and 64 (the np.add.at sums), on the recorded individuals and populations."""
    g = golden("score_cases.npz")
    gen = sc.GOLDEN[variant]
    assert ast.literal_eval(str(g[variant + "_gen"])) == gen
    case, L, A, start = sc.golden_inputs(variant)
    assert sc.digest(case) == str(g[variant + "_digest"])
    mine = sc.golden_record(oracle.loglike, oracle.partition_loglikes, variant)
    with np.errstate(all="ignore"):
        mine["assignLL"] = oracle.assignLL(L, A.copy(), 1)
    for key, val in mine.items():
        ref = g[variant + "_" + key]
        bad = sc.first_difference(np.ascontiguousarray(val), ref)
        assert bad is None, "%s %s: flat index %d: oracle %r, reference %r" % (variant, key, bad, val.ravel()[bad], ref.ravel()[bad])
        assert sc.same_nan(ref, np.ascontiguousarray(val)), (variant, key)
    # ... and the module's own helpers on the oracle's values are the recorded ones too
    c, V = sc.reference(oracle, variant)
    sub = V[np.array(gen["individuals"])][:, list(gen["populations"])]
    assert sc.same_nan(g[variant + "_loglike"], np.ascontiguousarray(sub))
    for P in sc.GOLDEN_PARTS:
        assert sc.same_nan(g[variant + "_parts_%d" % P], sc.partition_sums(sub, P)), P
    with np.errstate(all="ignore"):
        assert sc.same_nan(g[variant + "_assignLL"], sc.expected_sums(sub).astype(F32))
    started = g[variant + "_started"]
    assert np.isnan(start).any() and np.isneginf(start).any() and np.isposinf(start).any() and (np.abs(start) > 1e38).any()
    assert np.isfinite(started).any() and np.isnan(started).any()
