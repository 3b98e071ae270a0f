"""tests/synth_twin.py -- the NumPy restatement that tests/test_gpu_synth.py holds the device generator to, bit for bit -- held to the
model the generator is stated to follow (tests/synth.py), on the CPU.

Every count is taken on a fixed seed at depth 2 over 2 * 10^6 (site, individual) entries (2^20 sites for the population frequency)
and held to its exact expectation within 6 standard deviations of the binomial count: a false alarm of 2e-9 per count were the seed
not fixed.  Where the normal approximation does not hold (variance below 25: the cells of 9 and more reads) the exact binomial tails
are held to the same rate, 1e-9 a side.  For the two quantities that depend on the device's p (genotypes, classes per SNP) p is
pop_freq_ref rounded to float32; tests/test_gpu_synth.py bounds how far the device's p is from it.
"""
import math

import numpy as np
import pytest

import synth
import synth_twin as tw

SEED = 20260313
M, N, GROUPS = 50_000, 40, 4
DEPTH = 2.0


def held(obs, n, q):
    """A count of `obs` among n independent trials of probability q: within 6 sigma, or within the exact tails at 1e-9 a side."""
    n, obs = int(n), int(obs)
    var = n * q * (1.0 - q)
    if var >= 25.0:
        return abs(obs - n * q) <= 6.0 * math.sqrt(var)
    if q <= 0.0 or q >= 1.0:
        return obs == (0 if q <= 0.0 else n)
    def logpmf(k):
        return math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1) + k * math.log(q) + (n - k) * math.log1p(-q)
    mean = n * q
    if obs <= mean:
        tail = sum(math.exp(logpmf(k)) for k in range(0, obs + 1))
    else:
        hi = min(n, obs + 200 + int(20 * math.sqrt(var)))
        tail = sum(math.exp(logpmf(k)) for k in range(obs, hi + 1))
    return tail >= 1e-9


def test_held_is_a_six_sigma_test():
    assert held(5000, 10_000, 0.5) and held(5299, 10_000, 0.5) and not held(5301, 10_000, 0.5) and not held(4699, 10_000, 0.5)
    assert held(0, 16, 3 / 256) and held(2, 16, 3 / 256) and not held(9, 16, 3 / 256)        # P(X >= 9) = 4e-14
    assert held(16, 16, 253 / 256) and not held(7, 16, 253 / 256) and held(0, 5, 0.0) and not held(1, 5, 0.0)


@pytest.fixture(scope="module")
def sample():
    """The draws of M sites x N individuals in 4 interleaved groups, step by step."""
    gsnp = np.arange(M, dtype=np.uint64)[:, None]
    group_of = np.arange(N) % GROUPS
    p = tw.pop_freq_ref(SEED, gsnp, np.arange(GROUPS)[None, :]).astype(np.float32)[:, group_of]
    c = tw.gl_draws(SEED, gsnp, np.arange(N, dtype=np.uint64)[None, :])
    geno = tw.genotype(c, p)
    d = tw.poisson_depth(c, DEPTH, np.float32(tw.cdf0_ref(DEPTH)))
    alt, per_read = tw.alt_reads(c, geno, d)
    return dict(p=p, c=c, geno=geno, d=d, alt=alt, per_read=per_read, group_of=group_of)


# ---- the random stream ------------------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = [      # Random123's kat_vectors for philox4x32 with 10 rounds
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_philox_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        assert " ".join("%08x" % int(x) for x in tw.philox4x32_10(counter, key)) == want
    # vectorised: the three at once, through the broadcast
    out = tw.philox4x32_10([np.array([k[0][i] for k in KNOWN_ANSWERS], dtype=np.uint64) for i in range(4)],
                           [np.array([k[1][i] for k in KNOWN_ANSWERS], dtype=np.uint64) for i in range(2)])
    for j, (_, _, want) in enumerate(KNOWN_ANSWERS):
        assert " ".join("%08x" % int(x[j]) for x in out) == want


def test_u01_grid():
    """24 bits, centred: 2^-25 the smallest; from 2^23 on the sum x + 0.5 rounds to even, so the largest value is 1.0 itself (a depth
    draw of 1.0 still compares `> cdf`) and the grid has 2^23 + 2^22 + 1 distinct values."""
    g = tw.u01_grid()
    assert g.dtype == np.float32 and g[0] == 2.0 ** -25 and g[-1] == 1.0 and (np.diff(g) >= 0).all()
    assert len(np.unique(g)) == (1 << 23) + (1 << 22) + 1
    x = np.array([0, 255, 256, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint64)
    assert np.array_equal(tw.u01(x), g[(x >> np.uint64(8)).astype(np.int64)])
    assert abs(float(g.astype(np.float64).mean()) - 0.5) < 2.0 ** -25


def test_streams_differ_where_the_model_claims_independence(sample):
    """Two individuals of a pair, one individual at two neighbouring sites, one site in two groups: other words, and genotype draws
    that are uncorrelated -- the count of agreeing first-allele draws is binomial with the probability independence gives."""
    c, p = sample["c"], sample["p"]
    a = tw.u01(c[0]) < p
    for what, x, y, px, py in (("pair", a[:, 0::2], a[:, 1::2], p[:, 0::2], p[:, 1::2]),
                               ("neighbouring sites", a[0::2], a[1::2], p[0::2], p[1::2])):
        q = (px.astype(np.float64) * py + (1.0 - px.astype(np.float64)) * (1.0 - py)).mean()        # P(agree), up to the 24-bit grid
        assert held((x == y).sum(), x.size, q), what
    for k in range(4):
        assert (c[k][:, 0::2] != c[k][:, 1::2]).mean() > 0.999 and (c[k][0::2] != c[k][1::2]).mean() > 0.999
    # the same site in two groups: the ancestral draw is shared (that is the model), the drift's is not
    gsnp = np.arange(1 << 18, dtype=np.uint64)
    u0, v0, w0 = tw.pop_freq_draws(SEED, gsnp, 0)
    u1, v1, w1 = tw.pop_freq_draws(SEED, gsnp, 1)
    assert np.array_equal(u0, u1) and (v0 != v1).mean() > 0.999 and (w0 != w1).mean() > 0.999
    assert held(((v0 < 0.5) == (v1 < 0.5)).sum(), len(gsnp), 0.5) and held(((w0 < 0.5) == (w1 < 0.5)).sum(), len(gsnp), 0.5)
    z0 = (tw.pop_freq_ref(SEED, gsnp, 0, clip=False) - (0.5 - 0.5 * np.cos(np.pi * u0.astype(np.float64)))) / np.float64(np.float32(0.08))
    z1 = (tw.pop_freq_ref(SEED, gsnp, 1, clip=False) - (0.5 - 0.5 * np.cos(np.pi * u1.astype(np.float64)))) / np.float64(np.float32(0.08))
    assert abs(float((z0 * z1).mean())) <= 6.0 / math.sqrt(len(gsnp))                             # var(z0 z1) = 1
    # other seeds, either key word
    for other in (SEED + 1, SEED + (1 << 32)):
        assert (tw.gl_draws(other, gsnp[:1000], 0)[0] != tw.gl_draws(SEED, gsnp[:1000], 0)[0]).mean() > 0.99
    # the site index beyond 2^32 is another site
    assert (tw.gl_draws(SEED, gsnp[:1000] + np.uint64(1 << 32), 0)[0] != tw.gl_draws(SEED, gsnp[:1000], 0)[0]).mean() > 0.99


# ---- the value table --------------------------------------------------------------------------------------------------------------
def test_value_table_is_make_beagle_s():
    """Every (ref, alt) with ref + alt <= 15: the products multiplied up one read at a time, rint(x * 1e6) / 1e6, give the float32
    pair of tests/synth.py: make_beagle (powers, np.round(x, 6)) with e = 0.01 -- none differs -- and 120 distinct pairs among the 136:
    all that a matrix of the fixed-error generator can hold."""
    tab = tw.value_table()
    e = 0.01
    differ, pairs = [], set()
    for ref in range(tw.DMAX + 1):
        for alt in range(tw.DMAX + 1 - ref):
            d = ref + alt
            l0, l1, l2 = (1 - e) ** ref * e ** alt, 0.5 ** d, (1 - e) ** alt * e ** ref
            tot = l0 + l1 + l2
            want = (np.float32(np.round(l0 / tot, 6)), np.float32(np.round(l1 / tot, 6)))
            if want[0].tobytes() != tab[ref, alt, 0].tobytes() or want[1].tobytes() != tab[ref, alt, 1].tobytes():
                differ.append((ref, alt))
            pairs.add(tab[ref, alt].tobytes())
    assert differ == []
    assert len(pairs) == 120
    assert tab[0, 0].tobytes() == np.array([0.333333, 0.333333], dtype=np.float32).tobytes()


def test_matrix_holds_table_values_in_host_layout(sample):
    """matrix(): (g0, g1) pairs per individual in file order, whatever the groups; a row range at an offset is the slice."""
    group_of = sample["group_of"]
    L = tw.matrix(SEED, DEPTH, 300, group_of)
    tab = tw.value_table()
    want = tab[sample["d"][:300] - sample["alt"][:300], sample["alt"][:300]]
    assert L.shape == (300, 2 * N) and np.array_equal(L[:, 0::2], want[..., 0]) and np.array_equal(L[:, 1::2], want[..., 1])
    assert np.array_equal(tw.matrix(SEED, DEPTH, 100, group_of, site0=200), L[200:])
    assert np.array_equal(tw.matrix(SEED, DEPTH, 300, group_of, rows_per_step=7), L)
    Q = tw.matrix(SEED, DEPTH, 300, group_of, bins=tw.quality_bins())
    assert np.array_equal(tw.matrix(SEED, DEPTH, 100, group_of, site0=200, bins=tw.quality_bins()), Q[200:])
    assert np.array_equal((Q[:, 0::2] == np.float32(0.333333)) & (Q[:, 1::2] == np.float32(0.333333)), sample["d"][:300] == 0)


def test_quality_bins_as_the_host_prepares_them():
    e, cdf = tw.quality_bins()
    assert e.dtype == cdf.dtype == np.float32 and cdf[-1] == 1.0
    assert np.array_equal(e, np.array([10 ** -1.2, 10 ** -2.3, 10 ** -3.7]).astype(np.float32))
    assert np.array_equal(cdf, np.array([0.03, 0.03 + 0.12, 0.03 + 0.12 + 0.85]).astype(np.float32))
    e, cdf = tw.quality_bins((10, 20, 30, 40), (3.0, 0.5, 2.0, 1.5))
    assert np.allclose(cdf, [3 / 7, 3.5 / 7, 5.5 / 7, 1.0], rtol=1e-7, atol=0)
    for quals, probs in (((), ()), (tuple(range(9)), (1.0,) * 9), ((12, 23, 37), (0.0, 0.0, 0.0))):
        with pytest.raises(ValueError):
            tw.quality_bins(quals, probs)


# ---- the distributions ------------------------------------------------------------------------------------------------------------
def test_genotypes_are_hardy_weinberg_on_the_24_bit_grid(sample):
    """P(u01 < p) is exactly the share of the 2^24 grid values below p; the two allele draws are independent."""
    p, geno = sample["p"], sample["geno"]
    q = np.searchsorted(tw.u01_grid(), p.ravel(), side="left").reshape(p.shape) / float(1 << 24)
    assert np.abs(q - p).max() <= 2.0 ** -24
    for g, prob in ((0, (1 - q) ** 2), (1, 2 * q * (1 - q)), (2, q * q)):
        obs, mean, var = int((geno == g).sum()), prob.sum(), (prob * (1 - prob)).sum()
        print("genotype %d: %d observed, %.1f expected, %.2f sigma" % (g, obs, mean, (obs - mean) / math.sqrt(var)))
        assert abs(obs - mean) <= 6.0 * math.sqrt(var), g
    # ... also within every group and at the clip edges, where a wrong group's frequency would show
    for k in range(GROUPS):
        sel = sample["group_of"] == k
        prob = q[:, sel]
        obs = int((sample["c"][0][:, sel] >> np.uint64(8) < np.searchsorted(tw.u01_grid(), p[:, sel].ravel(), side="left").reshape(prob.shape)).sum())
        assert abs(obs - prob.sum()) <= 6.0 * math.sqrt((prob * (1 - prob)).sum()), k


def test_genotypes_follow_their_own_group(sample):
    """Drawn from another group's frequency the genotypes miss their expectation by hundreds of sigma: the statistic can tell."""
    geno, p = sample["geno"], sample["p"].astype(np.float64)
    wrong = np.roll(p, 1, axis=1)                                  # the neighbour's group
    for q, ok in ((p, True), (wrong, False)):
        prob = q * q
        # the alternative homozygotes where the neighbour's frequency is higher by more than 0.1
        sel = wrong - p > 0.1
        z = ((geno[sel] == 2).sum() - prob[sel].sum()) / math.sqrt((prob[sel] * (1 - prob[sel])).sum())
        assert (abs(z) <= 6.0) == ok, z


def poisson_pmf_truncated(lam):
    pmf = [math.exp(-lam) * lam ** k / math.factorial(k) for k in range(tw.DMAX)]
    return pmf + [1.0 - sum(pmf)]


def test_depth_is_poisson_2_truncated_at_15(sample):
    d = sample["d"]
    pmf = poisson_pmf_truncated(DEPTH)
    hist = np.bincount(d.ravel(), minlength=tw.DMAX + 1)
    print("depth histogram:", hist.tolist())
    for k in range(tw.DMAX + 1):
        assert held(hist[k], d.size, pmf[k]), (k, int(hist[k]), d.size * pmf[k])
    assert held((d >= 8).sum(), d.size, sum(pmf[8:]))
    # the float32 inversion is the exact one on the grid: its thresholds are the float64 cumulative sums to 2^-22
    c32 = p32 = np.float32(tw.cdf0_ref(DEPTH))
    for k in range(1, 13):
        p32 = np.float32(p32 * (np.float32(DEPTH) / np.float32(k)))
        c32 = np.float32(c32 + p32)
        assert abs(float(c32) - sum(pmf[:k + 1])) < 2.0 ** -22, k


def test_alternate_reads_are_binomial_at_the_8_bit_rates(sample):
    """Reads given genotype and depth: Binomial(d, {3, 128, 253} / 256) -- the effective error rate is 3/256 = 0.0117, not 0.01."""
    geno, d, alt = sample["geno"], sample["d"], sample["alt"]
    assert tuple(int((((np.arange(256, dtype=np.float32) + np.float32(0.5)) * np.float32(1 / 256)) < q).sum())
                 for q in (np.float32(0.01), np.float32(0.5), np.float32(0.99))) == tw.ALT_OF_256
    cells = 0
    for g in range(3):
        q = tw.ALT_OF_256[g] / 256.0
        for depth in range(1, int(d.max()) + 1):
            sel = (geno == g) & (d == depth)
            n = int(sel.sum())
            if n == 0:
                continue
            hist = np.bincount(alt[sel], minlength=depth + 1)
            assert held(alt[sel].sum(), n * depth, q), (g, depth)
            for a in range(depth + 1):
                assert held(hist[a], n, math.comb(depth, a) * q ** a * (1 - q) ** (depth - a)), (g, depth, a, int(hist[a]), n)
                cells += 1
    assert cells > 150
    n0 = int(((geno == 0) * d.astype(np.int64)).sum())
    obs = int(alt[geno == 0].sum())
    print("alternate reads of reference homozygotes: %d of %d = %.5f (3/256 = %.5f; 0.01 would be %.1f sigma away)" % (
        obs, n0, obs / n0, 3 / 256, (obs - 0.01 * n0) / math.sqrt(n0 * 0.01 * 0.99)))
    assert held(obs, n0, 3 / 256) and not held(obs, n0, 0.01)


def normal_cdf(x):
    return 0.5 * (1.0 + np.vectorize(math.erf)(np.asarray(x) / math.sqrt(2.0)))


def test_population_frequency_clip_shares_and_drift():
    """pop_freq_ref over 2^20 sites of one group: ancestral frequency Beta(1/2, 1/2) (mean 1/2, variance 1/8), drift N(0, 0.08^2),
    and the share clipped at either edge, P(anc + 0.08 z <= 0.01) integrated over the ancestral draw: 8.5 % each."""
    m = 1 << 20
    gsnp = np.arange(m, dtype=np.uint64)
    u, _, _ = tw.pop_freq_draws(SEED, gsnp, 1)
    anc = 0.5 - 0.5 * np.cos(np.pi * u.astype(np.float64))
    raw = tw.pop_freq_ref(SEED, gsnp, 1, clip=False)
    p = tw.pop_freq_ref(SEED, gsnp, 1)
    s = float(np.float32(0.08))
    drift = raw - anc
    assert abs(drift.mean()) <= 6.0 * s / math.sqrt(m)
    assert abs(drift.var() - s * s) <= 6.0 * s * s * math.sqrt(2.0 / m)
    assert abs(anc.mean() - 0.5) <= 6.0 * math.sqrt(0.125 / m)
    assert abs(anc.var() - 0.125) <= 6.0 * math.sqrt((3.0 / 128.0 - 1.0 / 64.0) / m)      # E(x - 1/2)^4 = 3/128 for the arcsine law
    grid = (np.arange(1 << 16) + 0.5) / (1 << 16)
    share = float(normal_cdf((0.01 - (0.5 - 0.5 * np.cos(np.pi * grid))) / s).mean())
    lo, hi = int((p == np.float64(np.float32(0.01))).sum()), int((p == np.float64(np.float32(0.99))).sum())
    print("clipped at 0.01: %d, at 0.99: %d of %d; expected share %.5f each; drift mean %.2e variance %.6f" % (lo, hi, m, share, drift.mean(), drift.var()))
    assert 0.08 < share < 0.09 and held(lo, m, share) and held(hi, m, share)
    assert p.min() == np.float64(np.float32(0.01)) and p.max() == np.float64(np.float32(0.99))


# ---- the reused words -------------------------------------------------------------------------------------------------------------
def test_word_reuse_touches_reads_7_and_11_and_only_entries_of_8_or_more_reads(sample):
    """Reads 4 to 14 come from the words that drew the genotype and the depth.  The frequency of the alternative allele at read r,
    given the genotype AND the outcome of the first (second) allele draw, against the rate of the genotype alone:

      reads 0-3   word 3, which nothing else uses                                         -> independent, within 6 sigma
      reads 4-6   bytes 0-2 of word 0: below the 8 bits that decide u01 < p               -> within 6 sigma
      read 7      byte 3 of word 0 = the top byte of the first allele's draw              -> a heterozygote's read 7 shows the
                  alternative allele in 86 % of the entries whose first allele is the reference's and in 14 % of the others (50 %
                  in the model): hundreds of sigma
      reads 8-10, read 11   the same for word 1 and the second allele's draw
      reads 12-14 bytes 0-2 of word 2, the depth draw's; u01 drops byte 0, and bytes 1 and 2 are the LOW 16 of its 24 bits.  MEASURED
                  on the sample: given the genotype and whether the depth draw lies above or below its median (and given either
                  allele draw) their frequency is the genotype's rate within 6 sigma -- no coarse dependence.  DERIVED, not
                  measured (the sample holds ONE entry of 13 or more reads): such an entry needs a depth draw within 2^-22 of 1,
                  which pins byte 2 to 0xFF and byte 1 to 0xFC-0xFF, so at depth 2 its reads 13 and 14 show the reference for
                  genotype 0 and the alternative for genotypes 1 and 2, always.  The scan of the 64 largest grid values at the end
                  of this test shows that on constructed draws.

    The correlation therefore needs 8 reads or more: 1.1e-3 of the entries at depth 2 for read 7, 1.5e-6 for read 11, 5e-7 for
    reads 12-14."""
    c, geno, d, p = sample["c"], sample["geno"], sample["d"], sample["p"]
    first, second = tw.u01(c[0]) < p, tw.u01(c[1]) < p
    deep_half = tw.u01(c[2]) > np.float32(0.5)                  # the outcome of the draw that reads 12-14 share their word with
    thr = np.array(tw.ALT_OF_256)[geno]
    worst = {}
    for r in range(tw.DMAX):
        alt_r = tw.read_byte(c, r) < thr                        # whether or not the entry has that many reads
        z = 0.0
        for cond in (first, second) + ((deep_half,) if r >= 12 else ()):
            for g in range(3):
                for val in (False, True):
                    sel = (geno == g) & (cond == val)
                    n = int(sel.sum())
                    if n:
                        q = tw.ALT_OF_256[g] / 256.0
                        z = max(z, abs(alt_r[sel].sum() - n * q) / math.sqrt(n * q * (1 - q)))
        worst[r] = z
        print("read %2d (word %d byte %d): used by %.2e of the entries; largest departure given a shared draw's outcome %.1f sigma" % (
            (r,) + tw.read_word_of(r) + ((d > r).mean(), z)))
    assert all(worst[r] <= 6.0 for r in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 13, 14)), worst
    assert worst[7] > 100 and worst[11] > 100
    assert [tw.read_word_of(r) for r in (7, 11)] == [(0, 3), (1, 3)] and all(tw.read_word_of(r)[0] == 2 for r in (12, 13, 14))
    het = geno == 1
    f7 = [(tw.read_byte(c, 7) < thr)[het & (first == v)].mean() for v in (False, True)]
    f11 = [(tw.read_byte(c, 11) < thr)[het & (second == v)].mean() for v in (False, True)]
    print("heterozygotes: read 7 alternative given first allele reference / alternative: %.4f / %.4f; read 11 given the second: %.4f / %.4f" % (
        f7[0], f7[1], f11[0], f11[1]))
    assert 0.8 < f7[0] < 0.9 and 0.1 < f7[1] < 0.2 and 0.8 < f11[0] < 0.9 and 0.1 < f11[1] < 0.2
    reach = (d >= 8).mean()
    print("entries with 8 or more reads: %.3e" % reach)
    assert held((d >= 8).sum(), d.size, sum(poisson_pmf_truncated(DEPTH)[8:])) and reach < 1.2e-3
    # reads 13 and 14 of an entry with 14 or 15 reads at depth 2: pinned
    v = np.arange((1 << 24) - 64, 1 << 24, dtype=np.uint64)
    words = (np.zeros_like(v),) * 2 + (v << np.uint64(8), np.zeros_like(v))
    deep = tw.poisson_depth(words, DEPTH, np.float32(tw.cdf0_ref(DEPTH))) >= 14
    assert deep.any() and not deep.all()
    for r in (13, 14):
        b = tw.read_byte(words, r)[deep]
        assert (b >= tw.ALT_OF_256[0]).all() and (b < tw.ALT_OF_256[1]).all(), r


# ---- classes per SNP --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins, mean, most", [(None, 26, 40), (tw.QUAL_BINS, 73, 105)])
def test_classes_per_snp_are_design_s(bins, mean, most):
    """DESIGN sections 2 and 3.9: distinct (g0, g1) pairs per SNP among 1000 individuals in 10 groups at depth 2, over 20 000 sites --
    26.28 on average (max 38; DESIGN quotes a maximum of 40) for the fixed error, 72.76 (max 105; DESIGN said 104 and now says what
    this sample shows) for the default quality bins."""
    n, K, m = 1000, 10, 20_000
    L = tw.matrix(SEED, DEPTH, m, np.arange(n) // (n // K), bins=None if bins is None else tw.quality_bins(*bins))
    cls = synth.classes_per_snp(L)
    print("classes per SNP over %d sites: mean %.2f, max %d" % (m, cls.mean(), cls.max()))
    assert round(float(cls.mean())) == mean and cls.max() <= most
