"""The device generator of synthetic Beagle matrices (csrc/beagle_kernels.hip: synth_kernel, synth_quality_kernel) restated in NumPy,
random stream included -- tests/synth.py is the twin of the model, this file of the bits.

The generator is a pure function of (seed, global site, global individual, group of the individual):

  pop_freq   two Philox-4x32-10 draws per (site, group) -> the population frequency p in float32, through cospif, logf and sqrtf of
             the device math library: the ONE inexact step.  pop_freq_ref below is its float64 reference; the GPU tests take the
             device's own p (wgs_debug_synth_freq) and bound it against the reference separately.  The same holds for
             cdf0 = expf(-depth), the probability of depth 0.
  synth_gl   one Philox draw per (site, individual): two genotype comparisons, a float32 Poisson inversion truncated at 15, up to 15
             read draws of 8 bits each, double products by repeated multiplication, rint(x * 1e6) / 1e6, (float).  The library is
             built without contraction and float32 / float64 division is correctly rounded, so all of this is plain IEEE arithmetic
             and gl() / gl_quality() below are exact, not approximate.

The model as it is, where it departs from its description:
  * a read's allele is drawn from 8 bits, (w + 0.5) / 256 < q: the effective error rates are 3/256, 128/256 and 253/256 (ALT_OF_256),
    not 0.01, 0.5, 0.99 -- the likelihoods are still computed with e = 0.01;
  * reads 4 to 14 of synth_gl reuse the three words that drew the genotype and the depth, xored with constants: read 7 shares its
    byte's position with the top byte of the first genotype draw, read 11 with the second, reads 12 to 14 with the low three bytes of
    the depth draw, of which u01 uses two (read_word_of).  Only entries with 8 or more reads are touched.

NumPy and the standard library only: no GPU, no library import.
"""
import math

import numpy as np

MASK = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
XOR = (None, np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0x85EBCA6B))     # bits[1..3] = c[0..2] ^ these
DMAX = 15
ALT_OF_256 = (3, 128, 253)          # bytes w of 256 with (w + 0.5) / 256 < {0.01f, 0.5f, 0.99f}
QUAL_BINS = ((12.0, 23.0, 37.0), (0.03, 0.12, 0.85))        # the defaults of DeviceBeagle.synth_quality
F32 = np.float32


def philox4x32_10(counter, key):
    """Philox-4x32-10 (Salmon et al., Random123): counter = 4 and key = 2 arrays (or scalars) of 32-bit words, broadcast against each
    other; returns the four output words as uint64 arrays below 2^32."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & MASK for x in counter)
    k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK for x in key)
    for _ in range(10):
        p0 = PHILOX_M0 * c0                     # 32 x 32 bits: fits uint64
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + PHILOX_W0) & MASK, (k1 + PHILOX_W1) & MASK
    return c0, c1, c2, c3


def u01(x):
    """((float)(x >> 8) + 0.5f) * 2^-24 in float32: the sum rounds (to even) from 2^23 on, so the grid has 2^23 + 2^22 + 1 distinct
    values, the largest of them 1.0."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(F32) + F32(0.5)) * F32(1.0 / 16777216.0)


def u01_grid():
    """u01 of all 2^24 values of x >> 8, ascending: np.searchsorted(grid, p, 'left') is the exact number of them with u01 < p."""
    return (np.arange(1 << 24, dtype=np.uint32).astype(F32) + F32(0.5)) * F32(1.0 / 16777216.0)


def _site_words(gsnp):
    g = np.asarray(gsnp, dtype=np.uint64)
    return g & MASK, g >> np.uint64(32)


def _key(seed):
    seed = int(seed)
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def pop_freq_draws(seed, gsnp, group):
    """The three uniforms of pop_freq, float32: u of the ancestral frequency (counter word 2 = 0xA5A5A5A5, word 3 = 0) and the two of
    the drift's Box-Muller (word 2 = 0x5A5A5A5A, word 3 = group)."""
    lo, hi = _site_words(gsnp)
    c = philox4x32_10((lo, hi, 0xA5A5A5A5, 0), _key(seed))
    d = philox4x32_10((lo, hi, 0x5A5A5A5A, np.asarray(group, dtype=np.uint64)), _key(seed))
    return u01(c[0]), u01(d[0]), u01(d[1])


def pop_freq_ref(seed, gsnp, group, clip=True):
    """pop_freq in float64 from the same draws and the kernel's own float32 constants (0.08f, 0.01f, 0.99f): ancestral frequency
    0.5 - 0.5 cos(pi u) (Beta(1/2, 1/2)), drift 0.08 N(0, 1) by Box-Muller, clipped to [0.01, 0.99].  clip=False: before the clip."""
    u, v, w = (x.astype(np.float64) for x in pop_freq_draws(seed, gsnp, group))
    anc = 0.5 - 0.5 * np.cos(np.pi * u)
    z = np.sqrt(-2.0 * np.log(v)) * np.cos(np.pi * (2.0 * w))
    p = anc + np.float64(F32(0.08)) * z
    if not clip:
        return p
    return np.minimum(np.maximum(p, np.float64(F32(0.01))), np.float64(F32(0.99)))


def cdf0_ref(depth):
    """exp(-(float)depth) in float64."""
    return math.exp(-float(F32(depth)))


def gl_draws(seed, gsnp, ind):
    """The four words of synth_gl's Philox draw (counter word 3 = 1) for every (site, individual) of the broadcast."""
    lo, hi = _site_words(gsnp)
    return philox4x32_10((lo, hi, np.asarray(ind, dtype=np.uint64), 1), _key(seed))


def genotype(c, p):
    return (u01(c[0]) < p).astype(np.int8) + (u01(c[1]) < p).astype(np.int8)


def poisson_depth(c, lam, cdf0):
    """The float32 Poisson inversion: while (ud > cdf && d < 15) { ++d; pm *= lam / (float)d; cdf += pm; }"""
    lam, cdf0 = F32(lam), F32(cdf0)
    ud = u01(c[2])
    cdf = np.full(ud.shape, cdf0, dtype=F32)
    pm = cdf.copy()
    d = np.zeros(ud.shape, dtype=np.int8)
    for k in range(1, DMAX + 1):
        go = (ud > cdf) & (d == k - 1)
        if not go.any():
            break
        d[go] = k
        pm = np.where(go, pm * (lam / F32(k)), pm).astype(F32)
        cdf = np.where(go, cdf + pm, cdf).astype(F32)
    return d


def read_words(c):
    return (c[3], c[0] ^ XOR[1], c[1] ^ XOR[2], c[2] ^ XOR[3])


def read_word_of(r):
    """(index of the Philox word, byte of it) that read r of synth_gl is drawn from: word 3 for reads 0-3, then words 0, 1, 2."""
    return ((3, 0, 1, 2)[r >> 2], r & 3)


def read_byte(c, r):
    """The byte read r of synth_gl compares: (w + 0.5) / 256 < qalt."""
    return ((read_words(c)[r >> 2] >> np.uint64((r & 3) * 8)) & np.uint64(0xFF)).astype(np.int64)


def alt_reads(c, geno, d):
    """Reads that show the alternative allele, and the same per read (15, ...) for the tests of the read draws."""
    qalt = np.array([0.01, 0.5, 0.99], dtype=F32)[geno]
    per_read = np.zeros((DMAX,) + np.shape(d), dtype=bool)
    for r in range(DMAX):
        ua = (read_byte(c, r).astype(F32) + F32(0.5)) * F32(1.0 / 256.0)
        per_read[r] = (r < d) & (ua < qalt)
    return per_read.sum(axis=0).astype(np.int8), per_read


def value_table():
    """(g0, g1) float32 of every (ref, alt) with ref + alt <= 15, [ref, alt]; the products multiplied up in the kernel's order."""
    tab = np.zeros((DMAX + 1, DMAX + 1, 2), dtype=F32)
    e1, e0 = 0.01, 0.99
    for ref in range(DMAX + 1):
        for alt in range(DMAX + 1 - ref):
            l0 = l1 = l2 = 1.0
            for _ in range(ref):
                l0 *= e0
                l2 *= e1
            for _ in range(alt):
                l0 *= e1
                l2 *= e0
            for _ in range(ref + alt):
                l1 *= 0.5
            tot = l0 + l1 + l2
            tab[ref, alt] = (F32(np.rint(l0 / tot * 1e6) / 1e6), F32(np.rint(l1 / tot * 1e6) / 1e6))
    return tab


_TABLE = None


def gl(seed, gsnp, ind, p, lam, cdf0):
    """synth_gl for every (site, individual) of the broadcast of gsnp, ind and p (float32): (g0, g1) float32."""
    global _TABLE
    if _TABLE is None:
        _TABLE = value_table()
    c = gl_draws(seed, gsnp, ind)
    geno = genotype(c, np.asarray(p, dtype=F32))
    d = poisson_depth(c, lam, cdf0)
    alt, _ = alt_reads(c, geno, d)
    v = _TABLE[d - alt, alt]
    return v[..., 0], v[..., 1]


def quality_bins(quals=QUAL_BINS[0], probs=QUAL_BINS[1]):
    """The host preparation of launch_synth_quality: (e, cdf) float32 per bin -- e = (float)pow(10, -Q / 10), cdf = the running sum of
    probs / sum(probs) in double, rounded to float32.  Raises ValueError where the library refuses."""
    nq = len(quals)
    if not 1 <= nq <= 8 or len(probs) != nq:
        raise ValueError("synthetic base qualities: 1 to 8 bins")
    tot = 0.0
    for x in probs:
        tot += float(x)
    if not tot > 0:
        raise ValueError("synthetic base qualities: probabilities sum to zero")
    run, e, cdf = 0.0, [], []
    for q, x in zip(quals, probs):
        run += float(x) / tot
        e.append(F32(math.pow(10.0, -float(q) / 10.0)))
        cdf.append(F32(run))
    return np.array(e, dtype=F32), np.array(cdf, dtype=F32)


def gl_quality(seed, gsnp, ind, p, lam, cdf0, bins):
    """synth_gl_quality: 16 bits per read (low byte: the allele, high byte: the base quality) from the words of the first draw and of
    a second one (counter word 3 = 2); bins = quality_bins(...)."""
    qe, qcdf = bins
    nq = len(qe)
    c = gl_draws(seed, gsnp, ind)
    geno = genotype(c, np.asarray(p, dtype=F32))
    d = poisson_depth(c, lam, cdf0)
    lo, hi = _site_words(gsnp)
    words = read_words(c)
    if d.max() > 8:
        words = words + philox4x32_10((lo, hi, np.asarray(ind, dtype=np.uint64), 2), _key(seed))
    from_alt = geno.astype(F32) * F32(0.5)
    l0 = np.ones(d.shape)
    l1 = np.ones(d.shape)
    l2 = np.ones(d.shape)
    for k in range(int(d.max())):
        live = k < d
        w = (words[k >> 1] >> np.uint64((k & 1) * 16)) & np.uint64(0xFFFF)
        uq = (((w >> np.uint64(8)) & np.uint64(0xFF)).astype(F32) + F32(0.5)) * F32(1.0 / 256.0)
        q = np.zeros(d.shape, dtype=np.int64)
        for j in range(nq - 1):                                  # while (q + 1 < nq && uq > cdf[q]) ++q
            q += (q == j) & (uq > qcdf[j])
        e = qe[q]
        ua = ((w & np.uint64(0xFF)).astype(F32) + F32(0.5)) * F32(1.0 / 256.0)
        p_alt = from_alt * (F32(1.0) - e) + (F32(1.0) - from_alt) * e
        alt = ua < p_alt
        ok = 1.0 - e.astype(np.float64)
        bad = e.astype(np.float64) / 3.0
        l0 = l0 * np.where(live, np.where(alt, bad, ok), 1.0)
        l1 = l1 * np.where(live, 0.5 * ok + 0.5 * bad, 1.0)
        l2 = l2 * np.where(live, np.where(alt, ok, bad), 1.0)
    tot = l0 + l1 + l2
    return (np.rint(l0 / tot * 1e6) / 1e6).astype(F32), (np.rint(l1 / tot * 1e6) / 1e6).astype(F32)


def matrix(seed, depth, m, group_of, site0=0, p=None, cdf0=None, bins=None, rows_per_step=None):
    """The (m, 2n) host-layout matrix of DeviceBeagle(m, n, group_of, site0=site0).synth(seed, depth) -- or .synth_quality with
    bins = quality_bins(...).  Keyed by global site (site0 + row) and global individual index; a group is nothing but whose frequency
    an individual is drawn from.  p: (m, groups) float32 (the device's own, wgs_debug_synth_freq), None: pop_freq_ref rounded to
    float32; cdf0 likewise."""
    group_of = np.asarray(group_of, dtype=np.int64)
    n = group_of.shape[0]
    n_groups = int(group_of.max()) + 1 if n else 1
    gsnp = np.uint64(site0) + np.arange(m, dtype=np.uint64)
    if p is None:
        p = pop_freq_ref(seed, gsnp[:, None], np.arange(n_groups)[None, :]).astype(F32)
    p = np.asarray(p, dtype=F32).reshape(m, -1)
    if cdf0 is None:
        cdf0 = F32(cdf0_ref(depth))
    L = np.empty((m, 2 * n), dtype=F32)
    step = rows_per_step or max(1, 200_000 // max(1, n))
    ind = np.arange(n, dtype=np.uint64)[None, :]
    for r0 in range(0, m, step):
        r1 = min(m, r0 + step)
        args = (seed, gsnp[r0:r1, None], ind, p[r0:r1][:, group_of], F32(depth), cdf0)
        g0, g1 = gl(*args) if bins is None else gl_quality(*args, bins)
        L[r0:r1, 0::2] = g0
        L[r0:r1, 1::2] = g1
    return L
