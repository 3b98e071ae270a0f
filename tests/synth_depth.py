"""Seeded allele-depth tables and the genotype likelihoods that go with them, for the z-score tests and golden vectors.

The z-score options (reference zscore.py) read, next to the Beagle matrix, a table AD of m x 2n int32: per individual the reads
carrying the reference and the alternative allele.  This generator draws HWE genotypes from per-population frequencies, Poisson
depths and reads with sequencing error e = 0.01, and writes the likelihoods as a PURE FUNCTION of the depth pair (what ANGSD's
fixed-error model gives), rounded to 6 decimals like the text of a Beagle file; `jitter` perturbs them so that the reference's
0.01 filter around the per-key mean drops sites.  Test infrastructure (NumPy), the twin of tests/synth.py.
"""
import hashlib

import numpy as np

import synth

E = 0.01


def make_depth(m, n, K, seed=synth.SEED, depth=1.5, jitter=0.0, sizes=None):
    """Return (L float32 (m, 2n), AD int32 (m, 2n), IDs (n, 2) str, A float32 (m, K) population frequencies).

    sizes: individuals per population (sums to n); default: equal contiguous blocks (synth.pop_labels)."""
    rng = np.random.Generator(np.random.PCG64(seed + 15485863 * m + 32452843 * n + K))
    p_anc = rng.beta(0.8, 0.8, size=m)
    p_pop = np.clip(p_anc[:, None] + rng.normal(0.0, 0.08, size=(m, K)), 0.02, 0.98)
    if sizes is None:
        IDs = synth.pop_labels(n, K)
    else:
        assert sum(sizes) == n and len(sizes) == K
        IDs = np.array([("Ind%d" % i, "pop%02d" % k) for i, k in enumerate(np.repeat(np.arange(K), sizes))], dtype=str)
    pop_of = np.searchsorted(np.unique(IDs[:, 1]), IDs[:, 1])
    f = p_pop[:, pop_of]                                   # (m, n)
    G = rng.binomial(2, f)
    D = rng.poisson(depth, size=(m, n))
    p_alt = np.array([E, 0.5, 1.0 - E])[G]
    Aa = rng.binomial(D, p_alt)
    Ar = D - Aa
    l0 = (1.0 - E) ** Ar * E ** Aa
    l1 = 0.5 ** D
    l2 = (1.0 - E) ** Aa * E ** Ar
    s = l0 + l1 + l2
    g0, g1 = l0 / s, l1 / s
    if jitter:
        g0 = np.clip(g0 + rng.normal(0.0, jitter, g0.shape) * (D > 0), 0.0, 1.0)
        g1 = np.clip(g1 + rng.normal(0.0, jitter, g1.shape) * (D > 0), 0.0, 1.0 - g0)
    L = np.empty((m, 2 * n), dtype=np.float32)
    L[:, 0::2] = np.round(g0, 6)
    L[:, 1::2] = np.round(g1, 6)
    AD = np.empty((m, 2 * n), dtype=np.int32)
    AD[:, 0::2] = Ar
    AD[:, 1::2] = Aa
    return L, AD, IDs, np.ascontiguousarray(p_pop, dtype=np.float32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def write_beagle(path, L):
    """The matrix as gzipped Beagle text (three likelihoods per individual, 6 decimals: exact for these values)."""
    import gzip
    m, n = L.shape[0], L.shape[1] // 2
    g2 = (np.float32(1) - L[:, 0::2]) - L[:, 1::2]
    with gzip.open(path, "wt") as fh:
        fh.write("marker\tallele1\tallele2" + "".join("\tInd%d\tInd%d\tInd%d" % (i, i, i) for i in range(n)) + "\n")
        for s in range(m):
            row = ["chr1_%d" % (s + 1), "0", "1"]
            for i in range(n):
                row += ["%.6f" % L[s, 2 * i], "%.6f" % L[s, 2 * i + 1], "%.6f" % g2[s, i]]
            fh.write("\t".join(row) + "\n")


def write_inputs(prefix, L, AD, IDs, A=None, npy_depths=False):
    """Files of one CLI run: returns dict(beagle, ids, names, ad, af)."""
    paths = dict(beagle=prefix + ".beagle.gz", ids=prefix + ".IDs.txt", names=prefix + ".pop_names.txt",
                 ad=prefix + (".ad.npy" if npy_depths else ".ad.txt"), af=prefix + ".pop_af.npy")
    write_beagle(paths["beagle"], L)
    np.savetxt(paths["ids"], IDs, fmt="%s", delimiter="\t")
    np.savetxt(paths["names"], np.unique(IDs[:, 1]), fmt="%s")
    if npy_depths:
        np.save(paths["ad"], AD)
    else:
        np.savetxt(paths["ad"], AD, fmt="%d")
    if A is not None:
        np.save(paths["af"], A)
    return paths
