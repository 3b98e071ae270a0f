"""--loo (glassy.py:47-112) at FULL size, held to the oracle over the WHOLE matrix.

Two shapes, each on a device-resident matrix (DeviceBeagle.synth):
  * A: configs[3] of BASELINE.json, 2M x 500, K=8 in contiguous blocks (62 x 7 + 66), --partition_sites 3;
  * B: the reference README's --loo shape, 5M x 180, K=5, one partition (need_parts: glassy.py:108-109), populations of 29, 33, 36,
    39 and 43 individuals INTERLEAVED in file order (a slab's local column is not the global index, the most recent earlier member
    of a population lies anywhere before), scored on a second, differently seeded matrix (--loo_downsampled_beagle).
Four runs per shape:
  1. glassy.loo_device(..., inspect=) in one batch with the codes forced: the re-fits through em_coded_group_kernel;
  2. the same with WGSASSIGN_LOO_CODES=0: em_sweep_group_kernel (wgs_debug_em_sweep_paths tells which kernels swept);
  3. the one-call C path (wgs_loo) with the cost models' own decisions;
  4. wgs_loo in batches of 61 fits, which split populations: the sticky columns are handed from batch to batch.
What must hold, bit for bit:
  (a) runs 1 and 2: the same iterations and the same clamped re-fits on every SNP of every fit (digests per fit and 8192-site chunk);
  (b) every re-fit on a 1.25 % sample of the chunks (with the first and the last) equals the oracle's emMAF_update, iterated as many
      times as the device reports on the population without the individual, clamped with n_pop - 1;
  (c) at least four re-fits per population -- first and last member, the first fit of the last wavefront group of 4 and of 16, the
      one with the most iterations -- equal the oracle on EVERY SNP, and the reported iteration is the reference's: its serial
      float32 convergence sum, continued from block to block, says `diff < tole` there and at no iteration before;
  (d) the n x K sums and the n x P x K partition chains of run 1 equal the oracle's scoring with the sticky overwrite in file order
      (oracle.loglike per (individual, population), np.sum's running float64 total over 8192-site chunks, serial float32 chains);
  (e) ll, parts, iters and the final af (each population's last re-fit, glassy.py:89) are the same in all four runs;
  (f) iterations lie in [1, 200]; at shape A every individual is assigned to its own population.
The device runs and the oracle's scoring (which needs run 1's re-fits while they live) happen once per shape, in a module fixture.
"""
import contextlib
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import synth
from test_gpu_parity import quiet, same
from test_gpu_whole_matrix import blocks_of, check_stopping_iterations, ids_of, sample_chunks, serial_f32

pytestmark = pytest.mark.gpu

CHUNK = 8192
BLOCK = 16 * CHUNK                 # rows per pass over the matrix (a multiple of the chunk: chunk sums and digests stay whole)
MAX_ITER, TOLE = 200, 1e-4
FORCED = {"WGSASSIGN_EM_CODES_SWEEPS": "0", "WGSASSIGN_SCORE_CODES_ALWAYS": "1", "WGSASSIGN_CODES_ALLOC_WAIT_MS": "-1"}   # = tests/conftest.py
COST_MODELS = {"WGSASSIGN_EM_CODES_SWEEPS": None, "WGSASSIGN_SCORE_CODES_ALWAYS": None, "WGSASSIGN_CODES_ALLOC_WAIT_MS": "-1"}
LOO_VARS = ("WGSASSIGN_LOO_CODES", "WGSASSIGN_LOO_BATCH", "WGSASSIGN_LOO", "WGSASSIGN_PARTS", "WGSASSIGN_CODES", "WGSASSIGN_EM_LOOP")


def interleaved(sizes, seed):
    return np.random.default_rng(seed).permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


SHAPES = {
    "A_config4_2Mx500_K8_P3": dict(m=2_000_000, group_of=blocks_of(500, 8), K=8, P=3, seed=synth.SEED + 4, scored_seed=None),
    "B_readme_loo_5Mx180_K5": dict(m=5_000_000, group_of=interleaved((29, 33, 36, 39, 43), 11), K=5, P=1, seed=synth.SEED + 5,
                                   scored_seed=synth.SEED + 6),
}


@contextlib.contextmanager
def environment(**kw):
    """Exactly these variables (None: unset) for the duration; the previous values come back afterwards."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_env(base, **loo):
    env = dict(base)
    env.update({k: None for k in LOO_VARS})
    env.update(loo)
    return env


def digest(v):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(v).tobytes(), digest_size=16).digest(), dtype=np.uint8)


def spans(r0, nr):
    """(chunk index, local start, local end) of the 8192-site chunks of rows [r0, r0 + nr); r0 is a multiple of CHUNK."""
    return [((r0 + s) // CHUNK, s, min(nr, s + CHUNK)) for s in range(0, nr, CHUNK)]


def where(r0, s):
    return "SNP %d (tile %d)" % (r0 + s, (r0 + s) // 64)


def chunk_where(c, m):
    hi = min(m, (c + 1) * CHUNK)
    return "chunk %d: SNPs %d..%d, tiles %d..%d" % (c, c * CHUNK, hi - 1, c * CHUNK // 64, (hi - 1) // 64)


def sticky_sources(group_of, K):
    """src[i, k]: the re-fit whose column individual i is scored against for population k -- its own for its population, else the
    most recent earlier individual's of that population (glassy.py:87-89, never restored), -1 = the initial af's column."""
    src = np.empty((len(group_of), K), dtype=np.int64)
    cur = np.full(K, -1, dtype=np.int64)
    for i, g in enumerate(group_of):
        cur[g] = i
        src[i] = cur
    return src


def refit_picks(group_of, K, iters):
    """Per population: first and last member, the first fit of its last wavefront group of 4 and of 16 (em_fits_per_group, and
    em_coded_group_kernel's walk; the first sweep lists a slab's fits in file order), the fit with the most iterations -- and where
    these coincide, the last fit of the last full group of 16, then the second member, so that there are four at least."""
    picks = []
    for g in range(K):
        mem = np.flatnonzero(group_of == g)
        c = len(mem)
        last16 = (c - 1) // 16 * 16
        mine = list(dict.fromkeys([0, c - 1, (c - 1) // 4 * 4, last16, int(np.argmax(iters[mem]))]))
        for j in (last16 - 1, 1, 2):
            if len(mine) < min(4, c) and 0 <= j < c and j not in mine:
                mine.append(j)
        picks += [int(mem[j]) for j in mine]
    return picks


class LooScoring:
    """The oracle's scoring of glassy.py:87-109 over a matrix walked in blocks of whole chunks: per (individual, population) the
    per-site vector of oracle.loglike against the sticky columns, np.sum(dtype=float) of every 8192-site chunk folded in order into
    the running float64 total (NumPy's own result, cf. test_gpu_whole_matrix.py), and the P partition chains (label = global site
    index % P, utils.py:147) as serial float32 sums carried from block to block."""

    def __init__(self, oracle, group_of, K, P, pool):
        self.oracle, self.K, self.P, self.pool = oracle, K, P, pool
        self.n = len(group_of)
        self.src = sticky_sources(group_of, K)
        self.tot = np.zeros((self.n, K), dtype=np.float64)
        self.chains = np.zeros((self.n * P, K), dtype=np.float32)

    def block(self, r0, rows, A0, F):
        """rows: (nr, 2n) of the scored matrix; A0: (nr, K) of the initial af; F: (n, nr) of the clamped re-fits."""
        orc, K, P, nr = self.oracle, self.K, self.P, rows.shape[0]
        full = nr // CHUNK * CHUNK

        def one(i):
            A = np.empty((nr, K), dtype=np.float32)
            for k in range(K):
                A[:, k] = F[self.src[i, k]] if self.src[i, k] >= 0 else A0[:, k]
            Li = orc.gather(rows, [i], 1)
            for k in range(K):
                vec = np.zeros(nr, dtype=np.float32)
                with np.errstate(all="ignore"):
                    orc.loglike(Li, A, vec, 1, 0, k)
                    sums = list(np.sum(vec[:full].reshape(-1, CHUNK), axis=1, dtype=float))
                    if full < nr:
                        sums.append(np.sum(vec[full:], dtype=float))
                t = self.tot[i, k]
                for s in sums:
                    t = t + s
                self.tot[i, k] = t
                for p in range(P):
                    self.chains[i * P + p, k] = serial_f32(self.chains[i * P + p, k], vec[(p - r0) % P::P])
        list(self.pool.map(one, range(self.n)))


class Inspector:
    """inspect= of glassy.loo_device: walks the converged, clamped re-fits of the (single) batch block by block -- digests per (fit,
    chunk), the columns on the sampled rows, and (with `scoring`) the oracle's scoring of the block."""

    def __init__(self, b, scored, af0, sample, pool, scoring=None):
        self.b, self.scored, self.af0, self.sample, self.pool, self.scoring = b, scored, af0, sample, pool, scoring
        self.paths = None

    def __call__(self, em, i0, i1):
        m, n = self.b.m, self.b.n
        assert (i0, i1) == (0, n), "one batch expected, got [%d, %d)" % (i0, i1)
        self.paths = em.sweep_paths()
        nchunks = (m + CHUNK - 1) // CHUNK
        self.digests = np.empty((n, nchunks, 16), dtype=np.uint8)
        pos = {c: j for j, c in enumerate(self.sample)}
        self.sampled = np.empty((n, sum(min(CHUNK, m - c * CHUNK) for c in self.sample)), dtype=np.float32)
        offs = np.concatenate(([0], np.cumsum([min(CHUNK, m - c * CHUNK) for c in self.sample])))
        for r0 in range(0, m, BLOCK):
            nr = min(BLOCK, m - r0)
            F = np.empty((n, nr), dtype=np.float32)
            for i in range(n):
                F[i] = em.get_f_range(i, r0, nr)

            def hashes(i):
                for c, lo, hi in spans(r0, nr):
                    self.digests[i, c] = digest(F[i, lo:hi])
            list(self.pool.map(hashes, range(n)))
            for c, lo, hi in spans(r0, nr):
                if c in pos:
                    self.sampled[:, offs[pos[c]]:offs[pos[c] + 1]] = F[:, lo:hi]
            if self.scoring is not None:
                self.scoring.block(r0, self.scored.download_rows(r0, nr), np.ascontiguousarray(self.af0[r0:r0 + nr]), F)


@pytest.fixture(scope="module", params=sorted(SHAPES))
def loo(request, oracle):
    from wgsassign_amd import device, emMAF, glassy
    from wgsassign_amd.comm import usable_cpus
    device.get_context()
    sh = SHAPES[request.param]
    m, group_of, K, P = sh["m"], sh["group_of"], sh["K"], sh["P"]
    n = len(group_of)
    pool = ThreadPoolExecutor(usable_cpus())
    b = device.DeviceBeagle(m, n, group_of, K)
    b.synth(sh["seed"], 2.0)
    scored = b
    if sh["scored_seed"] is not None:
        scored = device.DeviceBeagle(m, n, group_of, K)
        scored.synth(sh["scored_seed"], 2.0)
    with environment(**run_env(FORCED)):
        (_, af0, _), _ = quiet(emMAF.emMAF_populations, None, ids_of(group_of), MAX_ITER, TOLE, beagle=b)
    assert b.codes_state() == 1                    # the re-fits of run 1 find the class codes (with the slabs' own numbering) in place
    nchunks = (m + CHUNK - 1) // CHUNK
    npairs = sorted({(int(c) + 1) // 2 for c in np.bincount(group_of, minlength=K)})
    sample = sample_chunks(nchunks, npairs, (m + 63) // 64, 80)
    assert {0, nchunks - 1} <= set(sample) and len(sample) >= 0.0125 * nchunks
    runs = {}

    def run(name, env, inspect=None):
        af = af0.copy()
        tm = {}
        with environment(**env):
            (ll, parts), _ = quiet(glassy.loo_device, b, scored, af, group_of, MAX_ITER, TOLE, P, timings=tm, need_parts=True,
                                   inspect=inspect)
        assert tm.get("one_call", False) == (inspect is None), name
        runs[name] = dict(ll=ll, parts=parts, iters=np.asarray(tm["iters"]).copy(), af=af)

    scoring = LooScoring(oracle, group_of, K, P, pool)
    coded = Inspector(b, scored, af0, sample, pool, scoring)
    run("1 coded group kernel", run_env(FORCED, WGSASSIGN_LOO_CODES="1", WGSASSIGN_LOO_BATCH=str(n)), coded)
    direct = Inspector(b, scored, af0, sample, pool)
    run("2 float32 group kernel", run_env(FORCED, WGSASSIGN_LOO_CODES="0", WGSASSIGN_LOO_BATCH=str(n)), direct)
    run("3 wgs_loo, cost models", run_env(COST_MODELS))
    run("4 wgs_loo, batches of 61", run_env(FORCED, WGSASSIGN_LOO_BATCH="61"))

    class NS:
        pass
    ns = NS()
    ns.name, ns.b, ns.m, ns.n, ns.K, ns.P, ns.group_of = request.param, b, m, n, K, P, group_of
    ns.af0, ns.sample, ns.runs, ns.coded, ns.direct, ns.scoring, ns.pool = af0, sample, runs, coded, direct, scoring, pool
    ns.iters = runs["1 coded group kernel"]["iters"]
    ns.counts = np.bincount(group_of, minlength=K)
    yield ns
    pool.shutdown()
    if scored is not b:
        scored.close()
    b.close()


def who(ns, i):
    return "individual %d (population %d)" % (i, ns.group_of[i])


def test_a_two_group_kernels_agree_on_every_snp(loo):
    """Run 1 swept through em_coded_group_kernel, run 2 through em_sweep_group_kernel; same iterations, same re-fits everywhere."""
    c1, c2 = loo.coded.paths, loo.direct.paths
    # [em_sweep_kernel, em_sweep_group_kernel, em_coded_kernel, em_coded_group_kernel]: every sweep of run 1 through the codes, every
    # sweep of several fits per slab through the coded group kernel; in run 2 those through the float32 group kernel.  (Late sweeps
    # that list at most one fit per slab take the single-fit kernels: em_coded_kernel in both runs.)
    assert c1[0] == 0 and c1[1] == 0 and c1[3] >= 1, c1
    assert c2[3] == 0 and c2[1] >= 1, c2
    diff = np.argwhere(np.any(loo.coded.digests != loo.direct.digests, axis=2))
    assert diff.size == 0, "%d (fit, chunk) pairs differ between the two group kernels, first %s at %s" % (
        len(diff), who(loo, diff[0][0]), chunk_where(diff[0][1], loo.m))
    it1, it2 = loo.runs["1 coded group kernel"]["iters"], loo.runs["2 float32 group kernel"]["iters"]
    bad = np.flatnonzero(it1 != it2)
    assert bad.size == 0, "%s: %d iterations through the codes, %d over the float32 slab" % (who(loo, bad[0]), it1[bad[0]], it2[bad[0]])


def test_b_every_refit_on_sampled_chunks(loo, oracle):
    """All n re-fits on 1.25 % of the chunks (first and last included) against the oracle on the population without the individual."""
    m = loo.m
    rows = np.concatenate([loo.b.download_rows(c * CHUNK, min(CHUNK, m - c * CHUNK)) for c in loo.sample])
    snp = np.concatenate([np.arange(c * CHUNK, min(m, (c + 1) * CHUNK)) for c in loo.sample])
    members = [np.flatnonzero(loo.group_of == g) for g in range(loo.K)]

    def one(i):
        g = loo.group_of[i]
        Lp = oracle.gather(rows, members[g][members[g] != i], 1)
        f = np.full(rows.shape[0], 0.25, dtype=np.float32)
        for _ in range(int(loo.iters[i])):
            oracle.emMAF_update(Lp, f, 1)
        f = oracle.clamp(f, int(loo.counts[g]) - 1)
        bad = np.flatnonzero(f.view(np.uint32) != loo.coded.sampled[i].view(np.uint32))
        if bad.size:
            return "%s: %d of %d sampled SNPs differ, first %s: %r != oracle %r" % (
                who(loo, i), bad.size, f.size, where(0, snp[bad[0]]), loo.coded.sampled[i][bad[0]], f[bad[0]])
        return None
    errors = [e for e in loo.pool.map(one, range(loo.n)) if e]
    assert not errors, "%d of %d re-fits differ from the oracle:\n%s" % (len(errors), loo.n, "\n".join(errors[:10]))


def test_c_refits_on_every_snp_with_stopping_iterations(loo, oracle):
    """>= 4 re-fits per population on ALL rows: the oracle's columns equal the device's (digests per chunk), and the iteration the
    device reports is where the reference's serial float32 convergence sum first says `diff < tole`."""
    m = loo.m
    picks = refit_picks(loo.group_of, loo.K, loo.iters)
    assert np.all(np.bincount(loo.group_of[picks], minlength=loo.K) >= 4)
    its = [int(loo.iters[i]) for i in picks]
    carry = np.zeros((len(picks), max(its) + 1), dtype=np.float32)
    members = [np.flatnonzero(loo.group_of == g) for g in range(loo.K)]
    errors = []
    for r0 in range(0, m, BLOCK):
        nr = min(BLOCK, m - r0)
        rows = loo.b.download_rows(r0, nr)

        def one(j):
            i = picks[j]
            g = loo.group_of[i]
            Lp = oracle.gather(rows, members[g][members[g] != i], 1)
            f = np.full(nr, 0.25, dtype=np.float32)
            prev = f.copy()
            for t in range(1, its[j] + 1):
                oracle.emMAF_update(Lp, f, 1)
                d = f - prev
                carry[j, t] = serial_f32(carry[j, t], d * d)
                prev[:] = f
            f = oracle.clamp(f, int(loo.counts[g]) - 1)
            return ["%s, %s: the oracle's re-fit differs from the device's" % (who(loo, i), chunk_where(c, m))
                    for c, lo, hi in spans(r0, nr) if not np.array_equal(digest(f[lo:hi]), loo.coded.digests[i, c])]
        for e in loo.pool.map(one, range(len(picks))):
            errors += e
    assert not errors, "%d (fit, chunk) pairs differ:\n%s" % (len(errors), "\n".join(errors[:10]))
    with np.errstate(invalid="ignore"):
        diff = np.sqrt((carry / np.float32(m)).astype(np.float64))
    for j, i in enumerate(picks):
        try:
            check_stopping_iterations(diff[j:j + 1], its[j:j + 1])
        except AssertionError as e:
            raise AssertionError("%s: stopping iteration %d is not the reference's: %s" % (who(loo, i), its[j], e))


def test_d_scoring_over_the_whole_matrix(loo):
    """Run 1's n x K sums and n x P x K partition chains against the oracle's scoring of every SNP with the sticky columns."""
    r1 = loo.runs["1 coded group kernel"]
    K, P = loo.K, loo.P
    want = loo.scoring.tot.astype(np.float32)
    bad = np.argwhere(want.view(np.uint32) != r1["ll"].view(np.uint32))
    assert bad.size == 0, "%d of %d sums differ, first %s against population %d: %r != oracle %r (float64 %r)" % (
        len(bad), want.size, who(loo, bad[0][0]), bad[0][1], r1["ll"][tuple(bad[0])], want[tuple(bad[0])], loo.scoring.tot[tuple(bad[0])])
    assert r1["parts"].shape == (loo.n * P, K)
    bad = np.argwhere(loo.scoring.chains.view(np.uint32) != r1["parts"].view(np.uint32))
    assert bad.size == 0, "%d of %d partition sums differ, first %s, partition %d, population %d: %r != oracle %r" % (
        len(bad), loo.scoring.chains.size, who(loo, bad[0][0] // P), bad[0][0] % P, bad[0][1], r1["parts"][tuple(bad[0])],
        loo.scoring.chains[tuple(bad[0])])


def test_e_four_runs_one_result(loo):
    """The C path, the cost models' choice and the multi-batch hand-over land on the oracle-checked values of run 1; the final af
    holds each population's last re-fit."""
    names = sorted(loo.runs)
    ref = loo.runs[names[0]]
    for name in names[1:]:
        r = loo.runs[name]
        bad = np.flatnonzero(r["iters"] != ref["iters"])
        assert bad.size == 0, "%s: %s iterates %d times, run 1 %d" % (name, who(loo, bad[0]), r["iters"][bad[0]], ref["iters"][bad[0]])
        for key in ("ll", "parts"):
            bad = np.argwhere(r[key].view(np.uint32) != ref[key].view(np.uint32))
            i = bad[0][0] // (loo.P if key == "parts" else 1) if bad.size else 0
            assert bad.size == 0, "%s: %d %s values differ from run 1, first %s, population %d: %r != %r" % (
                name, len(bad), key, who(loo, i), bad[0][1], r[key][tuple(bad[0])], ref[key][tuple(bad[0])])
        bad = np.argwhere(r["af"].view(np.uint32) != ref["af"].view(np.uint32))
        assert bad.size == 0, "%s: final af differs from run 1 at %d places, first %s, population %d" % (
            name, len(bad), where(0, bad[0][0]), bad[0][1])
    last = {int(g): i for i, g in enumerate(loo.group_of)}
    for g, i in sorted(last.items()):
        col = np.ascontiguousarray(ref["af"][:, g])
        for c in range((loo.m + CHUNK - 1) // CHUNK):
            assert np.array_equal(digest(col[c * CHUNK:(c + 1) * CHUNK]), loo.coded.digests[i, c]), \
                "final af of population %d is not the re-fit of its last member %d, %s" % (g, i, chunk_where(c, loo.m))
    assert not same(ref["af"], loo.af0)


def test_f_iterations_and_assignment(loo):
    it = loo.iters
    assert it.min() >= 1 and it.max() <= MAX_ITER, (it.min(), it.max())
    if loo.name.startswith("A_"):
        ll = loo.runs["1 coded group kernel"]["ll"]
        wrong = np.flatnonzero(np.argmax(ll, axis=1) != loo.group_of)
        assert wrong.size == 0, "%s is assigned to population %d" % (who(loo, wrong[0]), np.argmax(ll[wrong[0]]))
