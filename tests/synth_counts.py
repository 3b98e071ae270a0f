"""Seeded ANGSD -dumpCounts 4 tables (reads of A, C, G, T per individual and site) and the files that go with them, for the
depth-ingest tests and their golden vector.  Test infrastructure (NumPy), next to tests/synth_depth.py."""
import gzip

import numpy as np


def make_counts(m, n, seed, depth=1.5):
    """(counts int64 (m, 4n), majmin int64 (m, 2) with major != minor).  Mostly the two selected bases carry reads, a few reads fall
    on the others, and a handful of cells hold the values where the digit count changes (9, 10, 99, 100, 255)."""
    rng = np.random.Generator(np.random.PCG64(seed + 7919 * m + 104729 * n))
    majmin = np.empty((m, 2), dtype=np.int64)
    majmin[:, 0] = rng.integers(0, 4, size=m)
    majmin[:, 1] = (majmin[:, 0] + rng.integers(1, 4, size=m)) % 4
    counts = rng.poisson(0.05, size=(m, n, 4))
    rows = np.arange(m)[:, None]
    cols = np.arange(n)[None, :]
    counts[rows, cols, majmin[:, :1]] = rng.poisson(depth * 0.7, size=(m, n))
    counts[rows, cols, majmin[:, 1:]] = rng.poisson(depth * 0.3, size=(m, n))
    flat = counts.reshape(m, 4 * n)
    for k, v in enumerate((9, 10, 99, 100, 255, 0)):
        flat[(k * 37) % m, (k * 11) % (4 * n)] = v
    return np.ascontiguousarray(flat), majmin


def write_counts(path, counts):
    """As ANGSD writes it: a header line, tab-separated, every line ending in a tab; gzipped."""
    n = counts.shape[1] // 4
    with gzip.open(path, "wt") as fh:
        fh.write("".join("ind%dTotDepth%s\t" % (i, b) for i in range(n) for b in "ACGT") + "\n")
        for row in counts:
            fh.write("".join("%d\t" % v for v in row) + "\n")


def write_majmin(path, majmin):
    """One header line; the selectors in the columns at positions 1 and 2 (allele_counts_beagle.py:14: usecols=(1, 2))."""
    with open(path, "w") as fh:
        fh.write("site\tmajor\tminor\n")
        for s, (a, b) in enumerate(majmin):
            fh.write("%d\t%d\t%d\n" % (s + 1, a, b))


def pick(counts, majmin):
    """What the conversion must give, restated: per individual (reads of the major, reads of the minor allele)."""
    m, n = counts.shape[0], counts.shape[1] // 4
    c = counts.reshape(m, n, 4)
    out = np.empty((m, 2 * n), dtype=np.int32)
    out[:, 0::2] = np.take_along_axis(c, np.broadcast_to(majmin[:, None, :1], (m, n, 1)), 2)[:, :, 0]
    out[:, 1::2] = np.take_along_axis(c, np.broadcast_to(majmin[:, None, 1:], (m, n, 1)), 2)[:, :, 0]
    return out
