"""What tests/fast_cases.py claims about the float32 mode of the scoring kernels on the enumerated terms, held with no GPU: the
restatement stays within the derived bound of the real-arithmetic reference however wrong the measurement allows fast_log to be; the
terms left out of that comparison are exactly those whose real sum is not positive; the class table of `finite` is empty; the float64
sum of a cell of restated terms is exact in any order; and inside the command line's clamp every sum is a positive normal number."""
import math

import numpy as np
import pytest

import fast_cases as fc
import score_cases as sc

SHAPES = ("grid", "block", sc.RAGGED)


@pytest.mark.parametrize("shape", SHAPES)
def test_compared_terms_are_those_with_a_positive_real_sum(shape):
    """The counts of the terms that are NOT compared by bound, computed in exact rational arithmetic, and the condition number of
    those that are: at most 2 -- nothing in the data excuses a deviation."""
    r = fc.real_of(shape)
    positive = r["sign"] > 0
    print("%s: %d distinct products, %d of %d terms have a real sum that is not positive, largest condition number of the others %.6f" % (
        shape, r["distinct"], int((~positive).sum()), positive.size, float(r["kappa"][positive].max())))
    assert (int((~positive).sum()), positive.size) == fc.NOT_POSITIVE[shape]
    assert r["kappa"][positive].max() <= 2.0 and r["kappa"][positive].min() >= 1.0
    assert np.isfinite(r["log"][positive]).all()
    # the bound is infinite only where the underflow of the products may take the whole sum: S below the float32 subnormals
    unbounded = positive & ~np.isfinite(r["bound"])
    print("    %d compared terms have no finite bound, the largest of their sums is %.3e; the largest finite bound is %.3e" % (
        int(unbounded.sum()), float(r["S"][unbounded].max()), float(r["bound"][positive & ~unbounded].max())))
    assert unbounded.sum() == fc.UNBOUNDED[shape] and r["S"][unbounded].max() < 2.0 ** -150 and r["S"][positive & ~unbounded].min() > 2.0 ** -149
    # the terms that are not compared by bound have -inf or NaN in the float32 mode's restatement exactly as the reference's rounding
    # sequence has them
    case = sc.case_of("finite", shape)
    with np.errstate(all="ignore"):
        ref_v, fast_v = fc.log_correct(sc.sums_of(case)), fc.log_correct(fc.fast_sums_of(case))
    rest = ~positive
    assert (np.isnan(ref_v[rest]) | np.isneginf(ref_v[rest])).all()
    assert np.array_equal(np.isnan(ref_v[rest]), np.isnan(fast_v[rest])) and np.array_equal(np.isneginf(ref_v[rest]), np.isneginf(fast_v[rest]))


@pytest.mark.parametrize("sign", [-1, 0, 1], ids=["low", "correctly rounded", "high"])
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_within_bound_of_the_real_terms(shape, sign):
    """With fast_log correctly rounded, and as far off to either side as the recorded error allows."""
    case, r = sc.case_of("finite", shape), fc.real_of(shape)
    prim = fc.log_correct if sign == 0 else fc.perturbed_log(sign)
    v, distinct = fc.through(prim, fc.fast_sums_of(case))
    positive = (r["sign"] > 0) & np.isfinite(r["bound"])
    dev = np.abs(v.astype(np.float64) - r["log"])[positive]
    ratio = dev / r["bound"][positive]
    worst = int(np.argmax(ratio))
    print("%s, %s: %d distinct sums, %d terms compared, largest deviation %.3e, largest share of its bound %.4f (deviation %.3e of %.3e at log S = %.6g)" % (
        shape, sign, distinct, int(positive.sum()), float(dev.max()), float(ratio.max()), float(dev[worst]), float(r["bound"][positive][worst]), float(r["log"][positive][worst])))
    assert np.isfinite(v[positive]).all()
    assert (ratio <= 1.0).all()
    # where the real sum is below the subnormals and the bound says nothing, the class is the oracle's
    rest = (r["sign"] > 0) & ~positive
    assert np.array_equal(np.isneginf(v[rest]), np.isneginf(fc.log_correct(sc.sums_of(case))[rest])) and not np.isnan(v[rest]).any()


def test_the_bound_is_no_blanket():
    """An ordinary term may deviate by a few ulps of its log, and the term the parent got 12 % wrong is far outside its bound."""
    r = fc.real_terms(np.float32(0.25), np.float32(0.5), np.float32(0.1))
    assert r["bound"] < 24 * fc.ulp32(r["log"]) + 12 * fc.U
    g0, g1, a = np.float32(0.001), np.float32(0.999), np.float32(1 - 2.0 ** -24)
    r = fc.real_terms(g0, g1, a)
    old = fc.fast_sum(g0, g1, a, g2=(np.float32(1) - g0) - g1)
    new = fc.fast_sum(g0, g1, a)
    assert r["sign"] > 0 and r["kappa"] <= 2
    assert abs(math.log(float(old)) - float(r["log"])) > 0.1 > 1e3 * float(r["bound"])
    assert abs(float(fc.log_correct(new)) - float(r["log"])) <= float(r["bound"])
    # ... and at a = 1 its class is the reference's
    assert fc.fast_sum(g0, g1, np.float32(1)) < 0 and sc.like_sum(g0, g1, np.float32(1)) < 0 and ((np.float32(1) - g0) - g1) == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_class_table_of_finite_is_empty(shape):
    case = sc.case_of("finite", shape)
    table = fc.class_table(case)
    print(shape, table)
    assert table["by_result"] == {} and table["by_sum"] == {} and table["same"] == table["terms"]


def test_class_table_names_what_g2_in_float32_did():
    """The first mutation, on the CPU: with g2 formed in float32 the grid has the 696 terms whose reference sum is negative (NaN) and
    whose float32 sum is +0 (-inf)."""
    case = sc.case_of("finite", "grid")
    table = fc.class_table(case, fc.fast_sum(case["L"][:, 0::2, None], case["L"][:, 1::2, None], case["A"][:, None, :], g2=fc.g2_float32(case)))
    print(table)
    assert table["by_result"].get(("NaN", "-inf"), 0) == 696


def test_class_table_of_hostile_is_counted():
    """On `hostile` the float32 mode need not have the reference's classes (a float32 product overflows or underflows where the double
    one does not); the table says how many terms differ, and the GPU test holds the kernels to the restatement's bits on all of them."""
    table = fc.class_table(sc.case_of("hostile", "grid"))
    print(table)
    assert table["terms"] == 197 * 52 * 23 and table["same"] + sum(table["by_sum"].values()) == table["terms"]


@pytest.mark.parametrize("shape", SHAPES)
def test_float64_sums_of_the_restated_terms_are_exact_in_any_order(shape):
    """score_cases.exact_sum_margin for the restated float32-mode values of every finite cell, with fast_log as far off as it may be."""
    case = sc.case_of("finite", shape)
    tightest = math.inf
    for sign in (-1, 1):
        V, _ = fc.fast_terms(case, fc.perturbed_log(sign))
        kinds = sc.cell_kinds(V)
        assert (kinds == 0).sum() >= 400
        for i, k in zip(*np.nonzero(kinds == 0)):
            total, limit = sc.exact_sum_margin(V[i, k])
            tightest = min(tightest, limit / total if total else math.inf)
    print("%s: the tightest finite cell keeps a factor %.1f" % (shape, tightest))
    assert tightest >= 8


def test_sums_inside_the_clamp_are_positive_normal_numbers():
    """What entitles the command line to the mode: for valid likelihood pairs (g0, g1 >= 0, g2 >= 0) and frequencies inside the clamp
    of 1 to 10^6 individuals every like_j >= 0 and one of them is at least min(a, 1 - a)^2 / 3 >= 8e-14, far above 2^-126."""
    pairs = fc.valid_pairs()
    assert len(pairs) >= 3000
    freqs = np.concatenate([fc.clamp_frequencies(n) for n in (1, 2, 42, 2000, 10 ** 5, 10 ** 6)])
    s = fc.fast_sum(pairs[:, None, 0], pairs[:, None, 1], freqs[None, :])
    print("smallest sum inside the clamp %.3e, largest %.9f" % (float(s.min()), float(s.max())))
    assert np.isfinite(s).all() and (s >= fc.TINY).all() and (s >= 2.0 ** -46).all() and (s <= 1 + 8 * fc.U).all()
    assert set(np.unique(sc.classify(s)).tolist()) <= {0, 1}


# ---- the float32 EM update ---------------------------------------------------------------------------------------------------------------
def test_em_compared_sites_are_those_whose_enumerated_cell_has_a_positive_real_sum():
    """A (fit, site) is compared by bound when all its terms have a real sum S > 0 (and a bound: S not below the float32 subnormals).
    The enumerated cell of a site decides it but for the frequencies next to 1, where the ordinary pair (0.666667, 0.333334), whose
    g2 is negative, has a negative sum of its own: the compared sites are those whose ONE enumerated cell qualifies -- the count
    em_cases gives for its hot cells -- less those."""
    import em_cases as ec
    grid = ec.grid_of("finite")
    K, m = len(grid["sizes"]), grid["L"].shape[0]
    c = grid["cell"]
    hot = fc.real_quotients(grid["pairs_tab"][c, 0], grid["pairs_tab"][c, 1], grid["f_tab"][c])
    hot_ok = (hot["sign"] > 0) & np.isfinite(hot["err"])
    compared = np.stack([fc.em_real_of(k)[2] for k in range(K)], axis=1)
    t = ec.cell_terms(grid)
    print("float32 EM update: %d of %d (fit, site) compared by bound (%.1f %%); of the others the reference's float32 sum is negative at %d and subnormal at %d" % (
        int(compared.sum()), compared.size, 100.0 * compared.mean(), int((t["s"] < 0)[~compared].sum()), int(((t["s"] > 0) & (t["s"] < fc.TINY))[~compared].sum())))
    print("    enumerated cells that qualify: %d; sites an ordinary column takes out: %d" % (int(hot_ok.sum()), int((hot_ok & ~compared).sum())))
    assert compared.shape == (m, K) and not (compared & ~hot_ok).any()
    assert (int(compared.sum()), compared.size, int(hot_ok.sum())) == fc.EM_COMPARED


@pytest.mark.parametrize("sign", [-1, 0, 1], ids=["low", "correctly rounded", "high"])
def test_em_restatement_within_bound_of_the_real_update(sign):
    """One update of every population of em_cases' `finite` grid from the enumerated frequencies, with fast_rcp correctly rounded and as
    far off to either side as the recorded error allows."""
    import em_cases as ec
    grid = ec.grid_of("finite")
    rcp = fc.rcp_correct if sign == 0 else fc.rcp_perturbed(sign)
    worst = 0.0
    for k in range(len(grid["sizes"])):
        F, bound, compared = fc.em_real_of(k)
        f = fc.fast_update(ec.columns(grid["L"], grid["members"][k]), grid["f_old"][k], rcp)
        share = np.abs(f.astype(np.float64) - F)[compared] / bound[compared]
        assert np.isfinite(f[compared]).all() and (share <= 1.0).all(), (k, float(share.max()))
        worst = max(worst, float(share.max()))
    print("largest share of an update's bound: %.4f" % worst)


def test_em_scaling_is_what_keeps_subnormal_sums_within_bound():
    """A term whose float32 sum is subnormal -- (0, 0) at f = 1e-20: s = 1e-40 -- has the quotient 1 in real arithmetic.  With the
    hardware's reciprocal (a subnormal argument is a zero: +inf) the unscaled term is inf; scaled it is within its bound."""
    def hardware(x):
        x = np.asarray(x, dtype=np.float32)
        return fc.rcp_correct(np.where(np.abs(x) < fc.TINY, np.copysign(np.float32(0), x), x))
    g0, g1, f = np.float32(0), np.float32(0), np.float32(1e-20)
    r = fc.real_quotients(g0, g1, f)
    q_scaled, _ = fc.fast_quotients(g0, g1, f, hardware)
    q_plain, _ = fc.fast_quotients(g0, g1, f, hardware, scale=False)
    assert r["sign"] > 0 and abs(float(r["q"]) - 1.0) < 1e-12
    assert np.isinf(q_plain).all() and abs(float(q_scaled.ravel()[0]) - float(r["q"])) <= float(r["err"]) < 1e-3
