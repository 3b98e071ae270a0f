"""CPU-only: the enumerated terms of tests/zstat_cases.py are what they claim to be, checked on the restatement (tests/zscore_cpu.py)
-- so that a passing comparison in tests/test_gpu_zstat_cases.py cannot hide a value class, a loop step, a table route or a place in
a tile that the terms never reach --; the restatement reproduces, bit for bit with NaN as NaN, what the real reference returned on
every one of them and on the pipeline case with frequencies of exactly 0 and 1 (tests/golden/zstat_cases.npz, made by
tests/golden/make_golden_zstat_cases.py); and a handful of subtly wrong variants of the statistic each differ from that record, so
the terms would catch a kernel that is wrong in the same way.  The counts are printed (pytest -s)."""
import ast
import os

import numpy as np
import pytest

import synth_depth
import zscore_cpu
import zstat_cases as zs
from conftest import GOLDEN
from test_zscore_cpu import same

F32 = np.float32


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "zstat_cases.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def grid():
    return zs.shared_grid()


@pytest.fixture(scope="module")
def recorded(gold, grid):
    """(slots, (wobs, wl, var) of the reference): the recorded subset of the grid."""
    assert zs.digest(grid) == str(gold["grid_digest"]), "the builders no longer reproduce the recorded inputs"
    slots = zs.recorded_slots(grid, **ast.literal_eval(str(gold["grid_gen"])))
    assert [len(s) for s in slots] == list(gold["grid_count"])
    return slots, tuple(gold["grid_" + k] for k in ("wobs", "wl", "var"))


# ---------------------------------------------------------------- the lists
def test_the_lists_hold_what_the_statistic_needs():
    assert all(zs.pool_holds(p) for p in zs.PAIRS), "a pair that none of the other case files holds"
    have = [zs.bits(zs.f32(p)).tolist() for p in zs.PAIRS]
    for p in ((1, 0), (0, 1), (0, 0), (1 - 2.0 ** -24, 2.0 ** -24), (0.666667, 0.333334), (-0.0, 0.0), (0.75, 0.75), (1.5, 0), (3e38, 3e38)):
        assert zs.bits(zs.f32(p)).tolist() in have, p
    pairs = zs.f32(zs.PAIRS)
    sub = (pairs != 0) & (np.abs(pairs) < zs.TINY)
    assert (sub & (pairs > 0)).any() and (sub & (pairs < 0)).any() and np.isinf(pairs).any() and np.isnan(pairs).any()
    assert ((pairs < 0) & np.isfinite(pairs) & ~sub).any() and (pairs[np.isfinite(pairs).all(axis=1)].astype(np.float64).sum(axis=1) > 1).sum() >= 3
    freqs = zs.f32(zs.FREQS)
    for v in (0.0, 1.0, 2.0 ** -149, 2.0 ** -126, 0.5, 1 / 3, 0.999999, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1 - 2.0 ** -24, 1 - 2.0 ** -23,
              2.0, -0.25, 1.5e19, 1e20, zs.INF):
        assert F32(v) in freqs, v
    assert np.isnan(freqs).sum() == 1 and (np.signbit(freqs) & (freqs == 0)).sum() == 1 and len(zs.FREQS) == 25
    for n_pop in (2, 16, 84):
        lo = F32(1 / (2 * (n_pop + 1)))
        assert lo in freqs and F32(1 - 1 / (2 * (n_pop + 1))) in freqs
    with np.errstate(all="ignore"):
        P = lambda a: (F32((1.0 - a) * (1.0 - a)), F32((2.0 * (1.0 - a)) * a))
        assert np.isfinite(P(float(F32(1.5e19)))[0]) and P(float(F32(1.5e19)))[1] == -np.inf
        assert P(float(F32(1e20))) == (np.inf, -np.inf)
    assert zs.DEPTHS == (0, 1, 2, 8, 21, 22, 23, 40) and max(zs.DENSE_DEPTHS) == zs.MAX_DENSE < min(zs.DEEP_DEPTHS)


def test_table_layout(grid):
    """Every hostile row is the only hostile row of its depth in its table; every one stands at a = 0, at a middle step and at
    a = dl, through the LDS table and through the deep rows; the index is written as the reference reads it; the device's tables hold
    the same rows."""
    fac0, like0, index = zs.ordinary_table()
    same(index, grid["index"], "index")
    assert index.dtype == np.int32 and np.isfinite(fac0).all() and np.isfinite(like0).all()
    assert 0 < fac0[zs.ROW0[21] + 21, 0] < zs.TINY, "AD_factorial of class (0, 21): a subnormal on real data"
    for d in zs.DEPTHS:
        for a in range(d + 1):
            r = index[a, d - a]
            assert r == zs.ROW0[d] + a
            g0, g1 = synth_deep_means(d - a, a)
            same(like0[r], np.array([g0, g1, (F32(1) - g0) - g1], dtype=F32), "class (%d, %d)" % (d - a, a))
    seen = set()
    for i, v in enumerate(grid["variant"]):
        changed = (zs.bits(grid["like"][i]) != zs.bits(like0)).any(axis=1) | (zs.bits(grid["fac"][i]) != zs.bits(fac0)).any(axis=1)
        if v == 0:
            assert not changed.any()
            continue
        assert len(zs.placements(int(v))) == len(zs.DEPTHS) and len({h for _, _, h in zs.placements(int(v))}) == len(zs.DEPTHS)
        for d, a, h in zs.placements(int(v)):
            rows = slice(zs.ROW0[d], zs.ROW0[d] + d + 1)
            assert list(np.flatnonzero(changed[rows])) == [a], (v, d)
            kind, row = zs.HOSTILE[h]
            same(zs.bits(grid[kind][i, zs.ROW0[d] + a]), zs.bits(zs.f32(row)), "hostile row")
            seen.add((h, "first" if a == 0 else "last" if a == d else "middle", d > zs.MAX_DENSE))
        assert changed.sum() == len(zs.DEPTHS)
        # what the device reads: the LDS table's rows and the deep rows are the reference's rows at AD_index[a, d - a]
        for d in zs.DEPTHS:
            for a in range(d + 1):
                want = np.concatenate((grid["like"][i, index[a, d - a]], grid["fac"][i, index[a, d - a]]))
                got = grid["tabs"][i, zs.class_index(d - a, a)] if d <= zs.MAX_DENSE else grid["deep_rows"][i, grid["deep_map"][i, d] + a, 2:]
                same(zs.bits(got), zs.bits(want), "row of depth %d step %d" % (d, a))
    assert sorted(set(grid["variant"])) == list(range(zs.N_VARIANTS + 1))
    assert seen >= {(h, where, deep) for h in range(zs.N_VARIANTS) for where in ("first", "middle", "last") for deep in (False, True)}


def synth_deep_means(Ar, Aa):
    import synth_deep
    g0, g1 = synth_deep.class_triple(Ar, Aa)
    return F32(g0), F32(g1)


def test_shape_and_placement(grid):
    L, AD, A, sites, n = grid["L"], grid["AD"], grid["A"], grid["sites"], len(grid["variant"])
    m = L.shape[0]
    assert m == 4096 + 64 + 5 and (m + 63) // 64 == 66 and A.shape == (m, n) and L.shape == AD.shape == (m, 2 * n)
    tiles, lanes = sites // 64, sites % 64
    for t in (0, 63, 64):
        assert (tiles == t).sum() == 64
    assert (tiles == 65).sum() == 5 and all(set(lanes[tiles == t]) == {0, 63} for t in range(1, 63)) and len(sites) == 321
    # population slabs of odd and even width, interleaved: both halves of a float4, a last odd column
    sizes = np.bincount(grid["group_of"])
    col = np.array([int((grid["group_of"][:i] == grid["group_of"][i]).sum()) for i in range(n)])
    assert {int(s) % 2 for s in sizes} == {0, 1} and set(col % 2) == {0, 1} and list(grid["group_of"][:6]) == [0, 1, 2, 3, 4, 0]
    assert any(col[i] == sizes[grid["group_of"][i]] - 1 and col[i] % 2 == 0 for i in range(n)), "no last odd column"
    for k in range(zs.N_SLABS):                                 # every slab holds ordinary and hostile tables
        assert {bool(v) for v in grid["variant"][grid["group_of"] == k]} == {False, True}
    assert len({A[:, i].tobytes() for i in range(n)}) == n, "a frequency column of its own for everybody"
    # the mask keeps exactly the term sites: in NumPy's words, per individual; without the deep table the dense ones
    hostile_dropped = 0
    dl_of = np.array(zs.DEPTHS)
    for i in range(n):
        keep = zs.expected_keep(L, AD, i, grid["key_mean"][i], grid["key_comp"][i], grid["deep_map"][i], grid["deep_rows"][i])
        assert np.array_equal(np.flatnonzero(keep), sites), i
        dense = zs.expected_keep(L, AD, i, grid["key_mean"][i], grid["key_comp"][i])
        assert np.array_equal(np.flatnonzero(dense), sites[dl_of[grid["t_depth"][i]] <= zs.MAX_DENSE]), i
        same(AD[sites, 2 * i] + AD[sites, 2 * i + 1], dl_of[grid["t_depth"][i]].astype(np.int32), "depths of the terms")
        other = np.setdiff1d(np.arange(m), sites)
        dl = AD[other, 2 * i] + AD[other, 2 * i + 1]
        assert set(dl) == {zs.DROP_DENSE_DEPTH, zs.DROP_DEEP_DEPTH, sum(zs.DROP_DENSE_CLASS), sum(zs.DROP_DEEP_CLASS)}
        hostile_dropped += int((~np.isfinite(L[other, 2 * i]) | ~np.isfinite(L[other, 2 * i + 1]) | ~np.isfinite(A[other, i])).sum())
        # kept classes take every component
        assert set(grid["key_comp"][i][grid["key_comp"][i] >= 0]) == {0, 1, 2}
    assert hostile_dropped > 1000
    # the ordinary table sees the whole product; every hostile table every (frequency, depth) with an ordinary pair and every pair at
    # 0, 0.5, 1 and a clamp bound
    ordinary = [zs.PAIRS.index(p) for p in zs.ORDINARY_PAIRS]
    four = {zs.FREQS.index(f) for f in zs.FREQS_FOR_EVERY_PAIR}
    assert len(four) == 4 and zs.FREQS_FOR_EVERY_PAIR[3] in zs.CLAMPS
    seen = set()
    for i, v in enumerate(grid["variant"]):
        terms = set(zip(grid["t_pair"][i].tolist(), grid["t_freq"][i].tolist(), grid["t_depth"][i].tolist()))
        if v == 0:
            seen |= terms
            continue
        assert {(f, d) for p, f, d in terms if p in ordinary} == {(f, d) for f in range(len(zs.FREQS)) for d in range(len(zs.DEPTHS))}, v
        assert {(p, f) for p, f, d in terms if f in four} >= {(p, f) for p in range(len(zs.PAIRS)) for f in four}, v
    assert seen == set(zs.product_terms()) and len(seen) == len(zs.PAIRS) * len(zs.FREQS) * len(zs.DEPTHS)
    # lanes: every pair and every frequency stands at lane 0 and at lane 63 of some tile
    for lane in (0, 63):
        at = np.flatnonzero(lanes == lane)
        assert set(grid["t_pair"][:, at].ravel()) == set(range(len(zs.PAIRS))) and set(grid["t_freq"][:, at].ravel()) == set(range(len(zs.FREQS)))


# ---------------------------------------------------------------- the claims, on the whole grid and on what is recorded
CLAIMS = ["s_obs " + c for c in zs.CLASS_NAMES] + ["s_exp %s at a %s step" % (c, w) for c in zs.CLASS_NAMES for w in ("first", "middle", "last")] + [
    "W_l finite", "W_l +inf", "W_l -inf", "W_l NaN", "var_W_l finite", "var_W_l +inf", "var_W_l NaN", "a product -inf * 0",
    "W_l a non-zero subnormal sum of subnormal products", "var_W_l a non-zero subnormal sum of subnormal products",
    "d * d overflows float32, not float64"]


@pytest.mark.parametrize("which", ["whole grid", "recorded"])
def test_value_classes_reached(grid, recorded, which):
    counts = zs.reached(grid, None if which == "whole grid" else recorded[0])
    print("\n" + which + ": terms per class")
    for k in CLAIMS:
        print("%8d  %s" % (counts[k], k))
        assert counts[k] > 0, k


@pytest.mark.parametrize("which", ["whole grid", "recorded"])
def test_where_precision_and_contraction_change_bits(grid, recorded, which):
    counts = zs.exact_counts(grid, None if which == "whole grid" else recorded[0])
    print("\n" + which + ": terms whose bits would change")
    for k, v in counts.items():
        print("%8d  %s" % (v, k))
        assert v > 0, k


def test_rounding_on_fractions():
    """zs.rnd is round-to-nearest-even at float32 and float64, subnormals included: held to NumPy's conversions."""
    from fractions import Fraction
    rng = np.random.Generator(np.random.PCG64(5))
    x = np.concatenate((rng.standard_normal(300) * 10.0 ** rng.integers(-46, 38, 300), [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 2.0 ** -150, 3 * 2.0 ** -150]))
    for v in x:
        assert zs.rnd(Fraction(float(v))) == Fraction(float(F32(v))), v
    for a, b in zip(x[:150], x[150:300]):
        assert zs.rnd64(Fraction(float(a)) * Fraction(float(b))) == Fraction(float(a * b))


# ---------------------------------------------------------------- the restatement is the reference; the mutants are not
def test_the_term_by_term_statistic_is_the_restatement(grid):
    for got, want, name in zip(zs.statistic(grid), zs.restatement(grid), ("W_l_obs", "W_l", "var_W_l")):
        assert not len(zs.differences(got, want)) and zs.same_nan(got, want), name     # (the sign of a NaN is nobody's claim)


def test_restatement_reproduces_every_recorded_term(grid, recorded):
    slots, ref = recorded
    assert sum(len(s) for s in slots) == len(ref[0]) >= 10000
    ind = np.concatenate([np.full(len(s), i) for i, s in enumerate(slots)])
    flat = np.concatenate(slots)
    for got, want, name in zip(zs.restatement(grid, slots), ref, ("W_l_obs", "W_l", "var_W_l")):
        bad = zs.differences(got, want)
        assert not len(bad), (name, len(bad), [(zs.describe(grid, ind[j], flat[j]), got[j], want[j]) for j in bad[:4]])
        assert zs.same_nan(got, want)


@pytest.mark.parametrize("mutant", zs.MUTANTS)
def test_a_subtly_wrong_statistic_differs_from_the_record(grid, recorded, mutant):
    slots, ref = recorded
    got = zs.statistic(grid, slots, mutant=mutant)
    counts = [len(zs.differences(a, b)) for a, b in zip(got, ref)]
    print("\n%s: differs from the record on %d W_l_obs, %d W_l, %d var_W_l of %d terms" % ((mutant,) + tuple(counts) + (len(ref[0]),)))
    assert sum(counts) > 0
    if mutant in ("fused", "untransposed", "running_wl"):
        assert counts[0] == 0                                    # (the loops alone)
    if mutant == "g2_f32":
        assert counts[1:] == [0, 0]


# ---------------------------------------------------------------- the mask builders
def test_deep_threshold_sites():
    t = zs.deep_threshold_sites()
    dl = t["AD"][:, 0::2] + t["AD"][:, 1::2]
    assert set(dl.ravel()) == {zs.THRESHOLD_DEEP_DEPTH, zs.THRESHOLD_DROPPED_DEPTH} and (t["key_comp"] == -1).all()
    assert (t["deep_map"] >= 0).sum() == 2 and (t["deep_map"][:, zs.THRESHOLD_DROPPED_DEPTH] == -1).all()
    for i in range(2):
        keep = zs.expected_keep(t["L"], t["AD"], i, t["key_mean"][i], t["key_comp"][i], t["deep_map"][i], t["deep_rows"])
        assert np.array_equal(keep, t["expect"][:, i]) and keep.sum() == 24 * 4 + 7
        assert (dl[t["dropped_sites"], i] == zs.THRESHOLD_DROPPED_DEPTH).all() and not keep[t["dropped_sites"]].any()
        assert keep[t["nan_sites"]].all()
        rows = t["deep_rows"][t["deep_map"][i, zs.THRESHOLD_DEEP_DEPTH]:][:zs.THRESHOLD_DEEP_DEPTH + 1]
        used = rows[np.unique(t["AD"][dl[:, i] == zs.THRESHOLD_DEEP_DEPTH, 2 * i + 1])]
        assert len(used) == 13 and set(used[:, 0]) == {0, 1, 2} and np.isnan(used[:, 1]).sum() == 1
    assert not np.array_equal(t["AD"][:, 0:2], t["AD"][:, 2:4])


def test_special_mask_values():
    s = zs.special_mask_values()
    keep = zs.expected_keep(s["L"], s["AD"], 0, s["key_mean"][0], s["key_comp"][0], s["deep_map"][0], s["deep_rows"])
    assert len(s["cells"]) == len(keep) == 90 and sorted(c[0] for c in s["cells"]) == list(range(90))
    for site, c, mean, v, deep in s["cells"]:
        assert (s["AD"][site].sum() > zs.MAX_DENSE) == deep
        with np.errstate(all="ignore"):
            g0, g1 = s["L"][site]
            at = (g0, g1, (F32(1) - g0) - g1)[c]
        assert (np.isnan(v) and np.isnan(at)) or at == F32(v) or (c == 2 and abs(at - F32(v)) < 1e-6), (site, c, v, at)
        if np.isnan(v) or (np.isinf(mean) and v == np.inf) or (mean == 0.0 and abs(v) < 1e-30):
            assert keep[site], (c, mean, v)
        elif np.isinf(v) or np.isinf(mean):
            assert not keep[site], (c, mean, v)
    assert sum(np.signbit(s["L"][site][c]) and s["L"][site][c] == 0 for site, c, _, v, _ in s["cells"] if c < 2) == 4


# ---------------------------------------------------------------- the pipeline case
def test_pipeline_case_against_the_reference_itself(gold):
    """zscore_cpu.assignment on frequencies of exactly 0 and 1: per individual the arrays the frequencies change against the record
    of this case, the others against the record of the same likelihoods and depths (zscore_classes.npz); stdout lines and file text."""
    import zscore_cases
    gen = ast.literal_eval(str(gold["pipeline_gen"]))
    assert gen == zs.PIPELINE_GEN
    L, AD, IDs, A = zs.boundary_frequencies(**gen)
    assert synth_depth.digest(L, AD, A) == str(gold["pipeline_digest"]), "the generator no longer reproduces the recorded inputs"
    assert (A[0::7][np.arange(len(A[0::7])) * 7 % 11 != 0] == 0).all() and (A[0::11] == 1).all()
    classes = np.load(os.path.join(GOLDEN, "zscore_classes.npz"), allow_pickle=False)
    with np.errstate(all="ignore"):
        want = zscore_cpu.assignment(L, AD, IDs, np.unique(IDs[:, 1]), A)
    lines = []
    for i, w in enumerate(want):
        for k in ("keys", "counts", "means", "AD_array", "keep", "fac", "like", "index"):
            same(w[k], classes["run0_i%d_%s" % (i, k)], "individual %d %s" % (i, k))
        for k in ("wobs", "wl", "var"):
            ref = gold["pipeline_i%d_%s" % (i, k)]
            bad = zs.differences(w[k], ref)
            assert not len(bad) and zs.same_nan(w[k], ref), (i, k, len(bad), w["keep"][bad[:4]], w[k][bad[:4]], ref[bad[:4]])
        sums = np.array([w["W_l_obs"], w["z_mu"], w["z_var"], w["z"]], dtype=F32)
        assert zs.same_nan(sums, gold["pipeline_i%d_sums" % i]), (i, sums, gold["pipeline_i%d_sums" % i])
        lines += zscore_cpu.stdout_lines(i, w)
    assert lines == str(gold["pipeline_stdout"]).splitlines()[:-1]
    assert zscore_cpu.file_text([w["z"] for w in want]) == str(gold["pipeline_file"])
    # what the case is for: log(0) at a kept site of a full individual, and a NaN that a class mean with a zero makes of -inf * 0
    for i in zscore_cases.FULL:
        assert np.isneginf(want[i]["wobs"]).sum() >= 1 and np.isnan(want[i]["wl"]).sum() >= 1
        at = want[i]["keep"][np.isneginf(want[i]["wobs"])]
        assert np.isin(A[at, int(np.argwhere(np.unique(IDs[:, 1]) == IDs[i, 1])[0][0])], (0, 1)).all()
