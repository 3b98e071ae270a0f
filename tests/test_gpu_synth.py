"""csrc/beagle_kernels.hip held to a NumPy twin: the synthetic generators (synth_kernel, synth_quality_kernel) against
tests/synth_twin.py, bit for bit over the whole downloaded matrix, and the movers (scatter_rows_kernel, gather_rows_kernel, the two
transposes) on matrices whose every element carries its own bit pattern.

The generator has one inexact step, the population frequency p (cospif, logf, sqrtf of the device math library) and
cdf0 = expf(-depth).  As tests/test_gpu_fast_cases.py does for fast_log, the device's own values of that step
(wgs_debug_synth_freq: the same device function the kernels call) are fed into the exact restatement, and the step itself is bounded
against its float64 reference separately (test_pop_freq_against_the_float64_reference, test_cdf0_against_exp).

That a second synth over a coded matrix drops the class codes was asserted nowhere (tests/test_gpu_codes.py only generates fresh
matrices): test_second_synth_drops_the_class_codes.
"""
import numpy as np
import pytest

import synth_twin as tw

pytestmark = pytest.mark.gpu

SEEDS = (20260313, (0x9E3779B9 << 32) | 0x7F4A7C15)          # the second needs both key words
# 41 individuals in 6 interleaved groups of 1, 2, 3, 16, 19 and 0: a lone column, one pair, an odd last pair, full quads, more than
# 16 columns, an empty group (launch_synth skips it)
SIZES = (1, 2, 3, 16, 19, 0)
GROUP_OF = np.random.default_rng(41).permutation(np.repeat(np.arange(6), SIZES)).astype(np.int32)
N, G = 41, 6

# Measured on an MI355X: the largest error of the device's p over 2^20 sites x 4 groups and of its expf(-depth), in float32
# ulps of the float64 reference.  The bounds asserted are these plus one ulp (another ROCm's math library may round one step
# differently); DESIGN section 3.7 quotes them.
P_ULPS_MEASURED = 49.773
CDF0_ULPS_MEASURED = 0.572


@pytest.fixture(scope="module")
def dev():
    from wgsassign_amd import device
    device.get_context()
    return device


def device_freq(dev, seed, site0, m, groups, depth):
    """The device's own p (m, groups) float32 and cdf0 (wgs_debug_synth_freq)."""
    from wgsassign_amd import _lib
    p = np.empty((groups, m), dtype=np.float32)
    cdf0 = np.zeros(1, dtype=np.float32)
    for g in range(groups):
        _lib.check(_lib.load().wgs_debug_synth_freq(dev.get_context().handle, int(seed), int(site0), int(m), g, float(depth), _lib.f32p(p[g]),
                                                    _lib.f32p(cdf0)))
    return np.ascontiguousarray(p.T), cdf0[0]


def device_matrix(dev, seed, depth, m, group_of=GROUP_OF, site0=0, bins=None, n=N):
    b = dev.DeviceBeagle(m, n, group_of, G, site0=site0)
    try:
        if bins is None:
            b.synth(seed, depth)
        else:
            b.synth_quality(seed, depth, quals=bins[0], probs=bins[1])
        return b.download_rows(0, m)
    finally:
        b.close()


def ulps_of(got, ref):
    """|got - ref| in float32 ulps of the float64 reference."""
    ref = np.asarray(ref, dtype=np.float64)
    _, e = np.frexp(ref)
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / np.ldexp(1.0, np.maximum(e, -125) - 24)


def freq_against_reference(p, seed, site0):
    """The device's p (m, groups) against tests/synth_twin.py: pop_freq_ref at the same seed, global sites and groups: every value within
    P_ULPS_MEASURED + 1 float32 ulps of the float64 reference, and the clip decisions (p = 0.01 or 0.99) the reference's except where
    the unclipped reference lies within that bound of the clip edge.  Returns the figures."""
    m, groups = p.shape
    gsnp = (np.uint64(site0) + np.arange(m, dtype=np.uint64))[:, None]
    raw = tw.pop_freq_ref(seed, gsnp, np.arange(groups)[None, :], clip=False)
    lo, hi = np.float64(np.float32(0.01)), np.float64(np.float32(0.99))
    ref = np.minimum(np.maximum(raw, lo), hi)
    clip_dev = np.where(p == np.float32(0.01), -1, 0) + np.where(p == np.float32(0.99), 1, 0)
    clip_ref = np.where(raw <= lo, -1, 0) + np.where(raw >= hi, 1, 0)
    agree = clip_dev == clip_ref
    err = np.where(agree, ulps_of(p, ref), 0.0)
    bound = P_ULPS_MEASURED + 1.0
    edge = np.where((clip_dev | clip_ref) < 0, lo, hi)
    off_edge = np.abs(raw - edge) / np.ldexp(1.0, np.frexp(edge)[1] - 24)
    at = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() <= bound, "p of seed %#x, site %d, group %d: %r on the device, %r in float64: %.3f ulps" % (
        seed, site0 + at[0], at[1], p[at], ref[at], err.max())
    assert (off_edge[~agree] <= bound).all(), "a clip decision differs from the reference's away from the edge (seed %#x, site0 %d)" % (seed, site0)
    return dict(worst=float(err.max()), at=at, differ=float((p != ref.astype(np.float32)).mean()), clipped_lo=float((clip_ref < 0).mean()),
                clipped_hi=float((clip_ref > 0).mean()), exceptions=int((~agree).sum()),
                farthest=float(off_edge[~agree].max()) if (~agree).any() else 0.0)


def twin_matrix(dev, seed, depth, m, group_of=GROUP_OF, site0=0, bins=None, n=N):
    """The twin's matrix from the device's own p and cdf0 -- which are first held to their float64 references at this very seed, offset
    and depth: the hook runs the pop_freq the kernels call, so a defect in how pop_freq forms its counter or key would otherwise be on
    both sides of the comparison."""
    groups = G if group_of is not None else 1
    p, cdf0 = device_freq(dev, seed, site0, m, groups, depth)
    freq_against_reference(p, seed, site0)
    assert float(ulps_of(cdf0, tw.cdf0_ref(depth))) <= CDF0_ULPS_MEASURED + 1.0, (depth, cdf0)
    return tw.matrix(seed, depth, m, np.zeros(n, dtype=np.int32) if group_of is None else group_of, site0, p=p, cdf0=cdf0,
                     bins=None if bins is None else tw.quality_bins(*bins))


def assert_same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, "%s: %d of %d elements differ, first at (row, column) %s: device %r, twin %r" % (
        what, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- the generators ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 4097])
def test_synth_equals_the_twin_at_every_shape(dev, m):
    """Below, at and above one tile of 64 sites, more than one block (4097 x 21 pairs), both seeds, the interleaved groups."""
    for seed in SEEDS:
        assert_same_bits(device_matrix(dev, seed, 2.0, m), twin_matrix(dev, seed, 2.0, m), "m = %d, seed %#x" % (m, seed))


@pytest.mark.parametrize("m", [1, 65, 4097])
def test_synth_of_a_single_group(dev, m):
    """group_of = None: one slab of 41 columns (20 pairs and a lone column), every individual drawn from group 0's frequency."""
    got = device_matrix(dev, SEEDS[0], 2.0, m, group_of=None)
    assert_same_bits(got, twin_matrix(dev, SEEDS[0], 2.0, m, group_of=None), "single group, m = %d" % m)
    grouped = device_matrix(dev, SEEDS[0], 2.0, m)
    members0 = np.flatnonzero(GROUP_OF == 0)
    cols = np.stack([2 * members0, 2 * members0 + 1], axis=1).ravel()
    assert_same_bits(np.ascontiguousarray(got[:, cols]), np.ascontiguousarray(grouped[:, cols]), "group 0's individuals")
    if m >= 65:
        assert got.tobytes() != grouped.tobytes()              # the other groups have frequencies of their own


def test_both_key_words_matter(dev):
    a, b, c = (device_matrix(dev, s, 2.0, 65) for s in (SEEDS[0], SEEDS[0] + (1 << 32), SEEDS[0] + 1))
    assert a.tobytes() != b.tobytes() and a.tobytes() != c.tobytes() and b.tobytes() != c.tobytes()


@pytest.mark.parametrize("site0", [0, 12345, (1 << 32) - 40])
def test_synth_at_a_site_offset(dev, site0):
    """The global site index is the Philox counter: the last offset carries it across the low counter word within the matrix (no
    benchmark shape gets there; a window or shard of a long file can)."""
    for seed in SEEDS:
        assert_same_bits(device_matrix(dev, seed, 2.0, 100, site0=site0), twin_matrix(dev, seed, 2.0, 100, site0=site0),
                         "site0 = %d, seed %#x" % (site0, seed))


def test_a_matrix_at_an_offset_is_the_slice(dev):
    """SNP shards are slices of the same matrix -- directly, for both generators."""
    s, m = 12345, 100
    for bins in (None, tw.QUAL_BINS):
        whole = device_matrix(dev, SEEDS[0], 2.0, s + m, bins=bins)
        part = device_matrix(dev, SEEDS[0], 2.0, m, site0=s, bins=bins)
        assert_same_bits(part, np.ascontiguousarray(whole[s:s + m]), "rows [%d, %d)" % (s, s + m))


@pytest.mark.parametrize("depth", [0.0, 1.5, 2.0, 30.0])
def test_synth_at_every_depth(dev, depth):
    """0: no reads anywhere; 1.5: tools/bench_zscore.py's; 2.0: the benchmark's; 30: the truncation at 15 (Poisson(30) stays below 15
    with probability 8e-4: all but a handful of the 10 537 entries are cut)."""
    m = 257
    for bins in (None, tw.QUAL_BINS):
        got = device_matrix(dev, SEEDS[1], depth, m, bins=bins)
        assert_same_bits(got, twin_matrix(dev, SEEDS[1], depth, m, bins=bins), "depth %g, bins %r" % (depth, bins))
        if depth == 0.0:
            assert (got.view(np.uint32) == np.float32(0.333333).view(np.uint32)).all()
    p, cdf0 = device_freq(dev, SEEDS[1], 0, m, G, depth)
    d = tw.poisson_depth(tw.gl_draws(SEEDS[1], np.arange(m, dtype=np.uint64)[:, None], np.arange(N, dtype=np.uint64)[None, :]), depth, cdf0)
    if depth == 0.0:
        assert cdf0 == 1.0 and (d == 0).all()
    if depth == 30.0:
        assert d.max() == 15 and (d == 15).mean() > 0.99
    if depth in (1.5, 2.0):
        assert d.min() == 0 and 2 <= d.max() < 15


QUALITY_CASES = {
    "default": tw.QUAL_BINS,
    "eight equal bins": ((20, 23, 26, 29, 32, 35, 38, 40), (0.125,) * 8),            # bench.py's
    "one bin": ((30,), (1.0,)),
    "not normalised": ((10, 20, 30, 40), (3.0, 0.5, 2.0, 1.5)),
}


@pytest.mark.parametrize("case", sorted(QUALITY_CASES))
def test_synth_quality_equals_the_twin(dev, case):
    bins = QUALITY_CASES[case]
    for m, seed in ((65, SEEDS[0]), (4097, SEEDS[1])):
        assert_same_bits(device_matrix(dev, seed, 2.0, m, bins=bins), twin_matrix(dev, seed, 2.0, m, bins=bins), "%s, m = %d" % (case, m))
    site0 = (1 << 32) - 40
    assert_same_bits(device_matrix(dev, SEEDS[0], 2.0, 100, site0=site0, bins=bins),
                     twin_matrix(dev, SEEDS[0], 2.0, 100, site0=site0, bins=bins), "%s, site0 = 2^32 - 40" % case)


def test_synth_quality_refusals_leave_the_matrix(dev):
    """0 bins, 9 bins, probabilities that sum to 0: an error, and the matrix and its class codes are what they were (the codes used to be
    dropped before the bins were looked at)."""
    m = 130
    b = dev.DeviceBeagle(m, N, GROUP_OF, G)
    try:
        b.synth(SEEDS[0], 2.0)
        before = b.download_rows(0, m)
        b.prepare_codes()
        assert b.codes_state() == 1
        for quals, probs in (((), ()), (tuple(range(20, 29)), (1.0,) * 9), ((12, 23, 37), (0.0, 0.0, 0.0))):
            with pytest.raises(ValueError, match="synthetic base qualities"):
                b.synth_quality(SEEDS[1], 2.0, quals=quals, probs=probs)
            with pytest.raises(ValueError):
                tw.quality_bins(quals, probs)
            assert_same_bits(b.download_rows(0, m), before, "after the refusal of %d bins" % len(quals))
            assert b.codes_state() == 1                        # ... and its class codes
    finally:
        b.close()


def test_second_synth_drops_the_class_codes(dev):
    """A matrix that has class codes and is generated again has none until they are rebuilt, and the rebuilt ones decode to the NEW
    matrix.  "None" is asserted as codes_state() == 0 and not as codes_info()["available"] being false: codes_info builds the codes when
    it is asked (wgs_beagle_codes_info calls wgs_beagle_codes), so it cannot report their absence; codes_state builds nothing."""
    m = 257
    b = dev.DeviceBeagle(m, N, GROUP_OF, G)
    try:
        b.synth(SEEDS[0], 2.0)
        b.prepare_codes()
        assert b.codes_state() == 1
        b.synth(SEEDS[1], 2.0)
        assert b.codes_state() == 0
        assert b.codes_info()["available"] and b.codes_state() == 1
        L = b.download_rows(0, m).view(np.uint32).reshape(m, N, 2)
        got = b.codes_download()
        assert (got["ncls"] > 0).all()
        rows = np.arange(m)[:, None]
        for g, slab in enumerate(got["slabs"]):
            members = np.flatnonzero(GROUP_OF == g)
            assert np.array_equal(got["dict"][rows, slab["codes"]], L[:, members]), g
    finally:
        b.close()


def test_pop_freq_against_the_float64_reference(dev):
    """p of 2^20 sites x 4 groups against tests/synth_twin.py: pop_freq_ref: the largest error in float32 ulps of the reference, and
    the clip decisions (p = 0.01 or 0.99) -- they agree except where the unclipped reference lies within the bound of a clip edge,
    on fewer than 1e-4 of the sites.  Measured: 49.773 ulps at p = 0.01007 (a p near 0.01 is the sum of terms of order 0.1 to 1, whose
    ulp is 16 to 64 of p's), 34.8 % of the values differ from the rounded reference, 8.55 % and 8.53 % of the entries are clipped at 0.01
    and 0.99, and no clip decision differs."""
    m, groups = 1 << 20, 4
    p, _ = device_freq(dev, SEEDS[0], 0, m, groups, 2.0)
    assert p.min() == np.float32(0.01) and p.max() == np.float32(0.99)
    f = freq_against_reference(p, SEEDS[0], 0)
    print("pop_freq over %d sites x %d groups: largest error %.3f float32 ulps of the reference at (site, group) %s, %.4f of the values "
          "differ from the rounded reference; clipped at 0.01: %.5f, at 0.99: %.5f; clip decisions that differ: %d (%.2e of the entries), "
          "the farthest %.3f ulps from its edge" % (m, groups, f["worst"], f["at"], f["differ"], f["clipped_lo"], f["clipped_hi"],
                                                     f["exceptions"], f["exceptions"] / p.size, f["farthest"]))
    assert f["exceptions"] < 1e-4 * p.size


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("site0", [0, 12345, (1 << 32) - 40, (1 << 32) - 300, 1 << 32, (1 << 40) + 7])
def test_pop_freq_at_every_offset_and_key(dev, seed, site0):
    """pop_freq has a counter and a key of its own: 600 sites x 6 groups held to the float64 reference with the same bound and clip rule,
    on both sides of the carry of the global site index into the high counter word and beyond it, and with a seed that needs the high
    key word.  A dropped word gives frequencies unrelated to the reference's: hundreds of thousands of ulps."""
    p, _ = device_freq(dev, seed, site0, 600, G, 2.0)
    f = freq_against_reference(p, seed, site0)
    assert f["exceptions"] <= 1 and 0.2 < f["differ"] < 0.5          # (about a third of the values are an ulp or more from the rounded reference)
    if site0 == (1 << 32) - 300:
        low, _ = device_freq(dev, seed, 300, 300, G, 2.0)            # the sites the dropped word would turn rows 300.. into
        assert (p[300:] != low).mean() > 0.5
    other, _ = device_freq(dev, seed ^ (1 << 32), site0, 600, G, 2.0)
    assert (p != other).mean() > 0.5                                 # the high key word alone makes another stream


def test_cdf0_against_exp(dev):
    worst = 0.0
    for depth in (0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 10.0, 20.0, 30.0):
        _, cdf0 = device_freq(dev, 1, 0, 1, 1, depth)
        worst = max(worst, float(ulps_of(cdf0, tw.cdf0_ref(depth))))
    print("expf(-depth) over 12 depths from 0 to 30: largest error %.3f float32 ulps" % worst)
    assert worst <= CDF0_ULPS_MEASURED + 1.0, worst


# ---- the movers -------------------------------------------------------------------------------------------------------------------
def pattern(m, cols, first=0):
    """Every element its own bit pattern, first + i * cols + j as uint32: subnormals from 1 on; with first = 0x7F7FFF00 infinity and NaN
    payloads, with first = 0x7FFFFF80 NaNs and, past 2^31, -0 and negative subnormals."""
    return (np.uint32(first) + np.arange(m * cols, dtype=np.uint32).reshape(m, cols)).view(np.float32)


FIRSTS = (0, 0x7F7FFF00, 0x7FFFFF80)


def test_download_rows_returns_exactly_the_rows(dev):
    m = 200
    for first in FIRSTS:
        L = pattern(m, 2 * N, first)
        b = dev.DeviceBeagle.from_host(L, GROUP_OF, G)
        try:
            for row0 in (0, 1, 63, 64, 65, 127):
                for nrows in (1, 63, 64, 65, 129):
                    if row0 + nrows <= m:
                        assert_same_bits(b.download_rows(row0, nrows), L[row0:row0 + nrows], "rows [%d, %d)" % (row0, row0 + nrows))
            assert_same_bits(b.download_rows(0, m), L, "the whole matrix")
            for row0, nrows in ((0, m + 1), (m, 1), (136, 65), (-1, 2)):
                with pytest.raises(ValueError, match="row range"):
                    b.download_rows(row0, nrows)
                with pytest.raises(ValueError, match="row range"):
                    b.upload_rows(np.zeros((nrows, 2 * N), dtype=np.float32), row0)
            assert_same_bits(b.download_rows(0, m), L, "after the refusals")
        finally:
            b.close()


def test_upload_rows_changes_those_rows_and_no_other(dev):
    m = 200
    L = pattern(m, 2 * N)
    second = pattern(m, 2 * N, 0x80000000)                      # -0 first, then the negative subnormals
    for group_of in (GROUP_OF, None):
        b = dev.DeviceBeagle.from_host(L, group_of, G)
        try:
            b.upload_rows(second[64:129], 64)
            want = L.copy()
            want[64:129] = second[64:129]
            assert_same_bits(b.download_rows(0, m), want, "after the upload of rows [64, 129)")
        finally:
            b.close()


def test_staging_loop_in_chunks_of_three_rows(dev):
    """wgs_beagle_upload_rows / wgs_beagle_download_rows stage through a 256 MB buffer: their loops run once for any matrix a test can
    afford.  With room for 3 rows, 200 rows take 67 rounds, the last of them short, through one buffer reused in stream order."""
    m = 200
    L = pattern(m, 2 * N, FIRSTS[1])
    second = pattern(m, 2 * N, 0x80000000)
    dev.debug_hook("staging_bytes", 3 * 2 * N * 4 + 7)
    try:
        b = dev.DeviceBeagle.from_host(L, GROUP_OF, G)
        try:
            assert_same_bits(b.download_rows(0, m), L, "200 rows, 3 per stage")
            assert_same_bits(b.download_rows(65, 100), L[65:165], "rows [65, 165), 3 per stage")
            b.upload_rows(second[1:200], 1)
            dev.debug_hook("staging_bytes", 0)
            want = L.copy()
            want[1:200] = second[1:200]
            assert_same_bits(b.download_rows(0, m), want, "uploaded 3 rows per stage, downloaded at once")
        finally:
            b.close()
    finally:
        dev.debug_hook("staging_bytes", 0)


def column_on_the_device(afs, k):
    """The m values at AFSet.col_dev(k), read back on the context's stream (wgs_debug_afset_col)."""
    from wgsassign_amd import _lib
    out = np.empty(afs.m, dtype=np.float32)
    _lib.check(_lib.load().wgs_debug_afset_col(afs.handle, int(k), _lib.f32p(out)))
    return out


@pytest.mark.parametrize("K", [1, 2, 5, 23])
def test_afset_round_trip_preserves_bits(dev, K):
    """mK_to_Km_kernel and Km_to_mK_kernel: (m, K) -> K columns of m -> (m, K); column k on the device IS column k."""
    for m in (1, 255, 256, 257, 4097):
        for first in FIRSTS[:2] if m < 4097 else FIRSTS[2:]:
            A = pattern(m, K, first)
            afs = dev.AFSet.from_host(A)
            try:
                assert_same_bits(afs.to_host(), A, "K = %d, m = %d" % (K, m))
                for k in sorted({0, K // 2, K - 1}):
                    assert afs.col_dev(k) is not None and afs.col_dev(K) is None and afs.col_dev(-1) is None
                    assert_same_bits(column_on_the_device(afs, k), np.ascontiguousarray(A[:, k]), "column %d of K = %d, m = %d" % (k, K, m))
                with pytest.raises(ValueError, match="column"):
                    column_on_the_device(afs, K)
            finally:
                afs.close()
