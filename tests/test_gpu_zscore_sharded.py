"""GPU: the two z-score options over SNP shards.  Two or three ranks share the one GPU as subprocesses over SocketComm (the pattern
of tests/test_gpu_multirank.py; tests/zscore_shard_worker.py is a rank); what rank 0 returns is held, bit for bit, to the outputs
recorded from the real reference (tests/golden/zscore.npz, zscore_deep.npz) and to the CPU restatement those records pin
(tests/zscore_cpu.py) -- never to the one-process device path.  Covered: the class sums handed from shard to shard with cuts
inside tiles, first sites beyond shard 0, a shard in which an individual keeps nothing, masked chains longer than a 4096-site block
on both sides of a cut, deep sites on both sides of a cut and next to it, every depth class up to 21 reads on
both sides of a cut, the depth file's row range, the command line with `--gpus` and under a launcher's RANK / WORLD_SIZE, and
ranks that fall out of step."""
import io
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import synth_counts
import synth_depth
import zscore_cpu
import zscore_shard_worker as worker
from conftest import GOLDEN, ROOT
from test_zscore_cpu import case_inputs, compare_individual, runs, same

pytestmark = pytest.mark.gpu

STEP_TIMEOUT = 240          # seconds a group of ranks may take: the guard against a hang, far above what a step needs
KEYS = ("keys", "counts", "means", "AD_array", "keep", "fac", "like", "index", "A", "wobs", "wl", "var")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "zscore.npz"), allow_pickle=False)


def start_ranks(tmp_path, case, world, batch=64):
    """The ranks of one case; (exit statuses, outputs, what rank 0 left)."""
    from wgsassign_amd.comm import free_port_pair
    port = free_port_pair()
    out = str(tmp_path / ("%s_%d_%d.pkl" % (case, world, batch)))
    env = dict(os.environ, WGSASSIGN_DEVICE="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "zscore_shard_worker.py"), case, str(r), str(world), str(port),
                               out, str(batch)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=STEP_TIMEOUT)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return [p.returncode for p in procs], outs, out


def ranks(tmp_path, case, world, batch=64):
    codes, outs, out = start_ranks(tmp_path, case, world, batch)
    for r, (c, o) in enumerate(zip(codes, outs)):
        assert c == 0, "rank %d of %d failed (%s):\n%s" % (r, world, case, o[-3000:])
    with open(out, "rb") as fh:
        return pickle.load(fh)


def restatement(inputs, spec, oracle):
    L, AD, IDs, A = inputs
    if spec["flavour"] == "assignment":
        return zscore_cpu.assignment(L, AD, IDs, np.unique(IDs[:, 1]), A, spec["thr"], spec["srt"], spec["lo"], spec["hi"])
    return zscore_cpu.reference(L, AD, IDs, lambda Lp, it, tol: oracle.emMAF(Lp, it, tol, 8), 200, 1e-4, spec["thr"], spec["srt"],
                                spec["lo"], spec["hi"])


def against_restatement(result, inputs, spec, oracle):
    """Every key tests/test_gpu_zscore.py: against_restatement compares, the iterations of the subset fits, z and the printed lines."""
    z, details, lines = result
    L, AD, IDs, A = inputs
    want = restatement(inputs, spec, oracle)
    pops = np.unique(IDs[:, 1])
    first = spec["lo"] or 0
    assert len(details) == len(want) > 0
    printed = []
    for j, (d, w) in enumerate(zip(details, want)):
        tag = "individual %d " % (first + j)
        if spec["flavour"] == "assignment":
            d = dict(d, A=np.ascontiguousarray(A[d["keep"], int(np.argwhere(pops == IDs[first + j, 1])[0][0])]))
        for k in KEYS:
            same(d[k], w[k], tag + k)
        for k in ("W_l_obs", "z_mu", "z_var", "z"):
            same(np.float32(d[k]), np.float32(w[k]), tag + k)
        if spec["flavour"] == "reference":
            assert d["it"] == w["extra"], tag + "iteration of the subset fit"
        printed += zscore_cpu.stdout_lines(first + j, w)
    assert lines == printed
    assert zscore_cpu.file_text(z[:, 0]) == zscore_cpu.file_text([w["z"] for w in want])
    return want


# ---------------------------------------------------------------- 1. the recorded runs
@pytest.mark.parametrize("world, batch", [(2, 64), (2, 3), (3, 64), (3, 3)])
def test_recorded_runs(tmp_path, gold, world, batch):
    """Every run of zscore.npz through the library path; the cuts (m r / world) are no multiples of 64."""
    results = ranks(tmp_path, "recorded", world, batch)
    assert len(results) == len(list(runs(gold))) > 0
    for (r, spec), (z, details, lines) in zip(runs(gold), results):
        L, AD, IDs, A = case_inputs(gold, spec["case"])
        assert all(c % 64 for c in worker.even_cuts(L.shape[0], world))
        pops = np.unique(IDs[:, 1])
        lo = spec["ind_start"] or 0
        assert len(details) == (spec["ind_end"] or L.shape[1] // 2) - lo
        for j, d in enumerate(details):
            if spec["flavour"] == "assignment":
                d = dict(d, A=np.ascontiguousarray(A[d["keep"], int(np.argwhere(pops == IDs[lo + j, 1])[0][0])]))
            compare_individual(gold, r, lo + j, d, d.get("it"))
        assert lines == str(gold["run%d_stdout" % r]).splitlines()[:-1]
        assert zscore_cpu.file_text(z[:, 0]) == str(gold["run%d_file" % r])


# ---------------------------------------------------------------- 2. odd shapes
def test_odd_shapes_three_ranks(tmp_path, oracle):
    """5003 sites cut at 1667 and 3335 (inside tiles), populations of 5 / 2 / 6, threshold 3, batches of 4 inside an individual range;
    --single_read_threshold once.  The dictionary's order is decided across the ranks: classes first seen beyond shard 0."""
    inputs = worker.odd_inputs()
    assert worker.even_cuts(5003, 3) == [1667, 3335]
    AD = inputs[1]
    beyond = 0
    for i in range(2, 11):
        _, first = np.unique(AD[:, 2 * i].astype(np.int64) * 1000 + AD[:, 2 * i + 1], return_index=True)
        beyond += int((first >= 1667).sum())
    assert beyond > 0, "no class of any tested individual has its first site outside shard 0"
    results = ranks(tmp_path, "odd", 3)
    jobs = worker.jobs("odd", 3, 64)
    assert len(results) == len(jobs) == 3
    for result, (_, _, spec) in zip(results, jobs):
        against_restatement(result, inputs, spec, oracle)


# ---------------------------------------------------------------- 3. an individual that keeps nothing in a shard
def test_a_shard_where_an_individual_keeps_nothing(tmp_path, oracle):
    (inputs, cuts, spec), = worker.jobs("empty", 2, 64)
    result = ranks(tmp_path, "empty", 2)[0]
    want = against_restatement(result, inputs, spec, oracle)
    w = want[worker.EMPTY_IND - spec["lo"]]
    assert len(w["keep"]) > 0 and w["keep"].max() < cuts[0], "the individual was meant to keep sites in shard 0 only"
    assert w["extra"] > 0, "its fit converged: the chain's carry passed through the empty shard"
    assert all((x["keep"] >= cuts[0]).any() for x in want if x is not w)


# ---------------------------------------------------------------- 4. chains longer than a block on both sides of a cut
def test_masked_chains_longer_than_a_block_in_both_shards(tmp_path, oracle):
    (inputs, cuts, spec), = worker.jobs("blocks", 2, 64)
    assert cuts[0] % 4096 and cuts[0] % 64
    result = ranks(tmp_path, "blocks", 2)[0]
    want = against_restatement(result, inputs, spec, oracle)
    assert len(want) == 3
    for w in want:
        assert (w["keep"] < cuts[0]).sum() > 4096 and (w["keep"] >= cuts[0]).sum() > 4096
        assert w["extra"] > 0


# ---------------------------------------------------------------- 5. deep sites across a cut
def test_deep_sites_on_both_sides_of_a_cut(tmp_path, oracle):
    jobs = worker.jobs("deep", 2, 64)
    inputs, cuts, _ = jobs[0]
    L, AD, IDs, A = inputs
    cut = cuts[0]
    dl = AD[:, 0::2] + AD[:, 1::2]
    for i in (1, 2):                                        # a dropped and the kept individual
        deep = np.flatnonzero(dl[:, i] > 21)
        assert {cut - 1, cut} <= set(deep) and (deep < cut - 1).any() and (deep > cut).any()
    code = AD[:, 4].astype(np.int64) * 1000 + AD[:, 5]
    split = [c for c in np.unique(code[dl[:, 2] > 21]) if (code[:cut] == c).any() and (code[cut:] == c).any()]
    assert split, "no deep class of the kept individual has sites in both shards"
    assert dl[:, 1].max() > 23                              # a deeper depth that is dropped
    results = ranks(tmp_path, "deep", 2)
    for result, (_, _, spec) in zip(results, jobs):
        want = against_restatement(result, inputs, spec, oracle)
        kept = want[2 - spec["lo"]]
        assert 22 in kept["AD_array"][:, 2] and kept["index"].shape[0] >= 23 and kept["index"].shape[1] >= 23
        deep2 = np.flatnonzero(dl[:, 2] > 21)
        assert np.isin(deep2[deep2 < cut], kept["keep"]).any() and np.isin(deep2[deep2 >= cut], kept["keep"]).any()


# ---------------------------------------------------------------- 5b. every depth class up to 21 reads across a cut
def test_every_class_on_both_sides_of_a_cut(tmp_path, oracle):
    """The class sums of the classes 64 .. 252 -- three of the class sweep's four wavefronts -- go on in shard 1 from what shard 0
    handed over: classes with all their sites before the cut (handed on untouched), all behind it (shard 0 hands on zeros) and on
    both sides; the depths 11 .. 21 are kept whole and their sites lie in both shards."""
    import zscore_cases
    jobs = worker.jobs("classes", 2, 64)
    inputs, cuts, _ = jobs[0]
    L, AD, IDs, A = inputs
    cut = cuts[0]
    assert cut % 64 and [spec["flavour"] for _, _, spec in jobs] == ["assignment", "reference"]
    for i in zscore_cases.FULL:
        before, after, both = zscore_cases.sides_of_cut(AD, i, cut)
        assert len(before) and len(after) and len(both) >= 100
    results = ranks(tmp_path, "classes", 2)
    for result, (_, _, spec) in zip(results, jobs):
        want = against_restatement(result, inputs, spec, oracle)
        for i in zscore_cases.FULL:
            assert sorted(set(want[i]["AD_array"][:, 2])) == list(range(1, 22))
            deep = np.flatnonzero(AD[:, 2 * i] + AD[:, 2 * i + 1] >= 11)
            assert np.isin(deep[deep < cut], want[i]["keep"]).any() and np.isin(deep[deep >= cut], want[i]["keep"]).any()


# ---------------------------------------------------------------- 6. the depth file's rows of a range
@pytest.mark.parametrize("fmt", ["text", "gzip", "bgzf"])
def test_depth_rows_of_a_range(tmp_path, fmt):
    from test_gpu_depth_ingest import Shape, edge_table, write_as
    from wgsassign_amd import zscore
    m, n = 1000, 5
    AD = edge_table(m, n, seed=4)
    rows = [" ".join(str(v) for v in r) for r in AD]
    lines = ["# head"] + rows[:100] + ["", "# before"] + rows[100:400] + ["# inside"] + rows[400:500] + [""] + rows[500:] + ["# tail"]

    def file_of(ls, name):
        return write_as(tmp_path / (name + "." + fmt), ("\n".join(ls) + "\n").encode(), fmt, block=900)

    path = file_of(lines, "ad")
    want = np.loadtxt(io.StringIO("\n".join(lines)), dtype=np.int32)
    assert np.array_equal(want, AD)
    for lo, hi in ((0, 333), (333, 667), (667, 1000), (391, 455), (999, 1000)):
        with Shape(hi - lo, n) as b:
            for chunk in (None, 1):
                t = zscore.DepthTable.from_file(b, path, first_row=lo, m_total=m, chunk_bytes=chunk)
                assert np.array_equal(t.download_rows(), want[lo:hi]), (lo, hi, chunk)
                t.close()
    with Shape(300, n) as b:
        # a bad token BEFORE the range is still reported, with its line of the file (behind a comment line: 1-based line 52)
        bad = list(lines)
        bad[51] = bad[51].replace(" ", " 1x ", 1)
        with pytest.raises(ValueError, match=r"line 52, column 2: not an integer"):
            zscore.DepthTable.from_file(b, file_of(bad, "junk"), first_row=400, m_total=m)
        bad = list(lines)
        bad[51] = bad[51].rsplit(" ", 1)[0]
        with pytest.raises(ValueError, match=r"line 52 has fewer than 10 columns"):
            zscore.DepthTable.from_file(b, file_of(bad, "short"), first_row=400, m_total=m)
        bad = list(lines)
        bad[51] = "256 " + bad[51].split(" ", 1)[1]
        with pytest.raises(ValueError, match=r"line 52: allele depths outside 0\.\.255"):
            zscore.DepthTable.from_file(b, file_of(bad, "big"), first_row=400, m_total=m)
        # too few and too many lines: both numbers, whatever the range
        with pytest.raises(ValueError, match=r"has 999 data lines, 1000 sites were expected"):
            zscore.DepthTable.from_file(b, file_of(lines[:-2], "fewer"), first_row=400, m_total=m)
        with pytest.raises(ValueError, match=r"has 1005 data lines, 1000 sites were expected"):
            zscore.DepthTable.from_file(b, file_of(lines + rows[:5], "more"), first_row=400, m_total=m)
        with pytest.raises(ValueError, match=r"outside its 1000 sites"):
            zscore.DepthTable.from_file(b, path, first_row=701, m_total=m)
        t = zscore.DepthTable.from_file(b, path, first_row=400, m_total=m)              # ... and the matrix still takes a good file
        assert np.array_equal(t.download_rows(), want[400:700])
        t.close()
        if fmt == "text":
            np.save(str(tmp_path / "ad.npy"), AD)
            t = zscore.DepthTable.from_file(b, str(tmp_path / "ad.npy"), first_row=400, m_total=m)
            assert np.array_equal(t.download_rows(), want[400:700])
            t.close()


def test_counts_rows_of_a_range(tmp_path):
    """Counts mode: the selectors handed in are the range's rows, majmin[lo:hi]."""
    from test_gpu_depth_ingest import Shape
    from wgsassign_amd import zscore
    m, n = 700, 4
    counts, majmin = synth_counts.make_counts(m, n, seed=9)
    cpath = str(tmp_path / "x.counts.gz")
    synth_counts.write_counts(cpath, counts)
    want = synth_counts.pick(counts, majmin)
    for lo, hi in ((0, 233), (233, 466), (466, 700)):
        with Shape(hi - lo, n) as b:
            t = zscore.DepthTable.from_file(b, cpath, counts=True, majmin=majmin[lo:hi].astype(np.uint8), first_row=lo, m_total=m)
            assert np.array_equal(t.download_rows(), want[lo:hi]), (lo, hi)
            t.close()
            with pytest.raises(ValueError, match="selectors have shape"):
                zscore.DepthTable.from_file(b, cpath, counts=True, majmin=majmin.astype(np.uint8), first_row=lo, m_total=m)


# ---------------------------------------------------------------- 7. the command line
KEEP = ("Finished individual", "z_mu", "z_var", "z_obs", "Loci used", "Z-score")


def cli(tmp_path, argv, world, launcher):
    """`--gpus world`, or `world` ranks started the way a launcher does (RANK / WORLD_SIZE); (root's z-score lines, status)."""
    env = dict(os.environ, WGSASSIGN_COMM="socket", WGSASSIGN_DEVICE="0", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    base = [sys.executable, "-m", "wgsassign_amd.WGSassign"]
    if not launcher:
        r = subprocess.run(base + ["--gpus", str(world)] + argv, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=STEP_TIMEOUT)
        return r.returncode, r.stdout, r.stderr
    from wgsassign_amd.comm import free_port_pair
    port = free_port_pair()
    procs = [subprocess.Popen(base + argv, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(env, RANK=str(k), LOCAL_RANK=str(k), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                                       MASTER_PORT=str(port))) for k in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=STEP_TIMEOUT))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for k in range(1, world):
        assert not [ln for ln in outs[k][0].splitlines() if ln.startswith(KEEP)], "rank %d printed z-score lines" % k
    return max(p.returncode for p in procs), outs[0][0], "".join(o[1] for o in outs)


def z_lines(stdout, tmp_path):
    return [ln.replace(str(tmp_path) + os.sep, "") for ln in stdout.splitlines()
            if ln.startswith(KEEP) or (ln.startswith("Saved ") and "z-scores" in ln)]


def recorded_argv(tmp_path, gold, r, spec, depth_args=None):
    """The inputs and arguments of tests/test_gpu_zscore.py: cli_run for recorded run r."""
    L, AD, IDs, A = case_inputs(gold, spec["case"])
    paths = synth_depth.write_inputs(str(tmp_path / ("in%d" % r)), L, AD, IDs, A)
    argv = ["--beagle", paths["beagle"], "--pop_af_IDs", paths["ids"], "--pop_names", paths["names"], "--out", "run%d" % r,
            "--get_%s_z_score" % spec["flavour"]] + (depth_args(paths, AD) if depth_args else ["--ind_ad_file", paths["ad"]])
    if spec["flavour"] == "assignment":
        argv += ["--pop_af_file", paths["af"]]
    if spec["thr"]:
        argv += ["--allele_count_threshold", str(spec["thr"])]
    if spec["srt"]:
        argv += ["--single_read_threshold"]
    if spec["ind_start"] is not None:
        argv += ["--ind_start", str(spec["ind_start"])]
    if spec["ind_end"] is not None:
        argv += ["--ind_end", str(spec["ind_end"])]
    return argv, "run%d" % r + (".z_ind.txt" if spec["flavour"] == "assignment" else ".reference_z_ind.txt")


def counts_files(tmp_path):
    """ANGSD counts that hold the same depths (reference allele on the major base), as tests/test_gpu_depth_ingest.py builds them."""
    def make(paths, AD):
        m, n = AD.shape[0], AD.shape[1] // 2
        rng = np.random.default_rng(8)
        majmin = np.empty((m, 2), dtype=np.int64)
        majmin[:, 0] = rng.integers(0, 4, size=m)
        majmin[:, 1] = (majmin[:, 0] + rng.integers(1, 4, size=m)) % 4
        counts = rng.poisson(0.1, size=(m, n, 4))
        counts[np.arange(m)[:, None], np.arange(n)[None, :], majmin[:, :1]] = AD[:, 0::2]
        counts[np.arange(m)[:, None], np.arange(n)[None, :], majmin[:, 1:]] = AD[:, 1::2]
        cpath, mpath = str(tmp_path / "in.counts.gz"), str(tmp_path / "in.majmin.txt")
        synth_counts.write_counts(cpath, counts.reshape(m, 4 * n))
        synth_counts.write_majmin(mpath, majmin)
        return ["--ind_counts_file", cpath, "--ind_majmin_file", mpath]
    return make


@pytest.mark.parametrize("flavour, world, launcher, counts", [("assignment", 2, False, False), ("reference", 3, True, False),
                                                              ("assignment", 3, True, True), ("reference", 2, False, True)])
def test_cli_matches_the_recorded_reference_cli(tmp_path, gold, flavour, world, launcher, counts):
    r, spec = next((r, s) for r, s in runs(gold) if s["flavour"] == flavour and not s["srt"])
    argv, name = recorded_argv(tmp_path, gold, r, spec, counts_files(tmp_path) if counts else None)
    code, stdout, stderr = cli(tmp_path, argv, world, launcher)
    assert code == 0, stdout[-2000:] + stderr[-3000:]
    assert z_lines(stdout, tmp_path) == str(gold["run%d_stdout" % r]).splitlines()
    assert open(tmp_path / name).read() == str(gold["run%d_file" % r])


@pytest.mark.parametrize("r, flavour", [(0, "assignment"), (1, "reference")])
def test_cli_deep_recorded_case_two_ranks(tmp_path, r, flavour):
    from test_zscore_deep_cpu import deep_inputs
    gold = np.load(os.path.join(GOLDEN, "zscore_deep.npz"), allow_pickle=False)
    L, AD, IDs, A, _ = deep_inputs(gold)
    paths = synth_depth.write_inputs(str(tmp_path / "in"), L, AD, IDs, A)
    argv = ["--beagle", paths["beagle"], "--pop_af_IDs", paths["ids"], "--pop_names", paths["names"], "--ind_ad_file", paths["ad"],
            "--out", "run%d" % r, "--get_%s_z_score" % flavour]
    argv += ["--pop_af_file", paths["af"]] if flavour == "assignment" else ["--ind_end", "5"]
    code, stdout, stderr = cli(tmp_path, argv, 2, False)
    assert code == 0, stdout[-2000:] + stderr[-3000:]
    assert z_lines(stdout, tmp_path) == str(gold["run%d_stdout" % r]).splitlines()
    name = "run%d" % r + (".z_ind.txt" if flavour == "assignment" else ".reference_z_ind.txt")
    assert open(tmp_path / name).read() == str(gold["run%d_file" % r])


# ---------------------------------------------------------------- 8. out of step
def test_ranks_out_of_step_end_with_a_mismatch(tmp_path):
    """Two ranks call assignment_z_scores with different batch sizes: both find it at the first collective and end with the status
    of a CollectiveMismatch (76); neither hangs -- the step's time limit is the guard."""
    codes, outs, out = start_ranks(tmp_path, "outofstep", 2)
    assert codes == [76, 76], "\n".join(o[-1500:] for o in outs)
    assert all("collective mismatch" in o for o in outs)
    assert not os.path.exists(out)
