"""GPU: the z-score path (wgsassign_amd/zscore.py over csrc/zscore_*.hip) against the outputs recorded from the real reference
(tests/golden/zscore.npz) and, on generated shapes, against the CPU restatement that those records pin (tests/zscore_cpu.py):
depth classes, L_keep, the subset fits' frequencies and stopping iterations, the per-site arrays, the three sums and z -- bit for
bit; the CLI's stdout lines and output files byte for byte."""
import ast
import contextlib
import io
import os

import numpy as np
import pytest

import synth_depth
import zscore_cpu
from conftest import GOLDEN
from test_zscore_cpu import case_inputs, compare_individual, runs, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "zscore.npz"), allow_pickle=False)


def device_run(L, AD, IDs, A, flavour, thr, srt, lo, hi, batch=64, site0=0):
    from wgsassign_amd import zscore
    from wgsassign_amd.device import AFSet, DeviceBeagle
    pops = np.unique(IDs[:, 1])
    group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
    n = L.shape[1] // 2
    lo, hi = zscore.ind_range(n, lo, hi)
    if flavour == "reference":
        b = DeviceBeagle.from_host(L, group_of, len(pops), site0=site0)
    else:
        b = DeviceBeagle.from_host(L, site0=site0)
    depth = zscore.DepthTable(b, AD, chunk_rows=1000)
    details, lines = [], []
    if flavour == "reference":
        z = zscore.reference_z_scores(b, depth, IDs, group_of, 200, 1e-4, thr, srt, lo, hi, batch=batch, say=lines.append, details=details)
    else:
        afs = AFSet.from_host(A)
        z = zscore.assignment_z_scores(b, depth, IDs, pops, afs, thr, srt, lo, hi, batch=batch, say=lines.append, details=details)
        for d, i in zip(details, range(lo, hi)):
            d["A"] = np.ascontiguousarray(A[d["keep"], int(np.argwhere(pops == IDs[i, 1])[0][0])])
        afs.close()
    depth.close()
    b.close()
    return z, details, [ln for ln in lines if not ln.startswith("EM (MAF)")]


@pytest.mark.parametrize("batch", [64, 3])
def test_recorded_runs_through_the_c_abi(gold, batch):
    """Every recorded run; batch = 3 puts batch boundaries inside the populations of 4 and 3 and splits the population of two."""
    for r, spec in runs(gold):
        L, AD, IDs, A = case_inputs(gold, spec["case"])
        z, details, lines = device_run(L, AD, IDs, A, spec["flavour"], spec["thr"], spec["srt"], spec["ind_start"], spec["ind_end"], batch)
        lo = spec["ind_start"] or 0
        for j, d in enumerate(details):
            d = dict(d, sums=None)
            compare_individual(gold, r, lo + j, d, d.get("it"))
        assert lines == str(gold["run%d_stdout" % r]).splitlines()[:-1]
        assert zscore_cpu.file_text(z[:, 0]) == str(gold["run%d_file" % r])


def against_restatement(L, AD, IDs, A, flavour, oracle, thr=0, srt=False, lo=None, hi=None, batch=64, site0=0, sample=None):
    z, details, lines = device_run(L, AD, IDs, A, flavour, thr, srt, lo, hi, batch, site0)
    pops = np.unique(IDs[:, 1])
    if flavour == "assignment":
        want = zscore_cpu.assignment(L, AD, IDs, pops, A, thr, srt, lo, hi)
    else:
        want = zscore_cpu.reference(L, AD, IDs, lambda Lp, it, tol: oracle.emMAF(Lp, it, tol, 8), 200, 1e-4, thr, srt, lo, hi)
    first = lo or 0
    for j, (d, w) in enumerate(zip(details, want)):
        tag = "individual %d " % (first + j)
        for k in ("keys", "counts", "means", "AD_array", "keep", "fac", "like", "index", "A", "wobs", "wl", "var"):
            same(d[k], w[k], tag + k)
        for k in ("W_l_obs", "z_mu", "z_var", "z"):
            same(np.float32(d[k]), np.float32(w[k]), tag + k)
        if flavour == "reference":
            assert d["it"] == w["extra"], tag + "iteration of the subset fit"
    assert len(details) == len(want) > 0
    return details


def test_odd_shapes_against_the_restatement(oracle):
    """A site count that is not a multiple of 64, site0 != 0, populations of 5, 2 and 6, a batch boundary inside a population, an
    individual range, perturbed likelihoods and a threshold -- both flavours."""
    L, AD, IDs, A = synth_depth.make_depth(5003, 13, 3, seed=77, depth=2.5, jitter=0.01, sizes=(5, 2, 6))
    against_restatement(L, AD, IDs, A, "assignment", oracle, thr=3, batch=4, site0=12345)
    against_restatement(L, AD, IDs, A, "reference", oracle, thr=3, lo=2, hi=11, batch=4, site0=12345)
    against_restatement(L, AD, IDs, A, "assignment", oracle, srt=True)
    against_restatement(L, AD, IDs, A, "reference", oracle, srt=True, lo=4, hi=8)


def test_million_sites_against_the_restatement(oracle):
    """1,000,003 sites: the class sums run over hundreds of thousands of sites each (binade crossings of the float32 chains), the
    subset fits' convergence chains over ~700k kept sites take the block-parallel walk with its marked blocks.  Every array is
    compared whole for the individuals tested (no sampling)."""
    L, AD, IDs, A = synth_depth.make_depth(1000003, 6, 2, seed=5, depth=1.5, sizes=(2, 4))
    d = against_restatement(L, AD, IDs, A, "reference", oracle, lo=1, hi=4)
    assert min(len(x["keep"]) for x in d) > 500000
    against_restatement(L, AD, IDs, A, "assignment", oracle, lo=1, hi=3)


def test_deeper_than_the_classes_is_an_error_not_a_number():
    from wgsassign_amd import zscore
    from wgsassign_amd.device import DeviceBeagle
    L, AD, IDs, A = synth_depth.make_depth(640, 4, 2, seed=3)
    AD = AD.copy()
    AD[17, 2:4] = (15, 9)
    b = DeviceBeagle.from_host(L)
    depth = zscore.DepthTable(b, AD)
    with pytest.raises(ValueError, match="deeper than 21"):
        zscore.AD_summary(depth, 0, 4, 0, False)
    assert len(zscore.AD_summary(depth, 0, 4, 0, True)) == 4          # depth 1 only: such data is accepted
    AD[3, 0] = 256
    with pytest.raises(ValueError, match="do not fit"):
        zscore.DepthTable(b, AD)
    bad = zscore.DepthTable(b)
    with pytest.raises(ValueError, match="do not fit"):
        bad.upload_rows(AD, 0)
    b.close()                       # the tables go with their matrix; closing them afterwards is a no-op
    depth.close()
    bad.close()


def cli_run(tmp_path, gold, r, spec, npy=False):
    from wgsassign_amd import WGSassign
    L, AD, IDs, A = case_inputs(gold, spec["case"])
    paths = synth_depth.write_inputs(str(tmp_path / ("in%d" % r)), L, AD, IDs, A, npy_depths=npy)
    out = str(tmp_path / ("run%d" % r))
    argv = ["--beagle", paths["beagle"], "--pop_af_IDs", paths["ids"], "--pop_names", paths["names"], "--ind_ad_file", paths["ad"],
            "--out", out, "--get_%s_z_score" % spec["flavour"]]
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
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        WGSassign.main(argv)
    name = out + (".z_ind.txt" if spec["flavour"] == "assignment" else ".reference_z_ind.txt")
    keep = ("Finished individual", "z_mu", "z_var", "z_obs", "Loci used", "Z-score", "Saved ")
    lines = [ln.replace(str(tmp_path) + os.sep, "") for ln in buf.getvalue().splitlines() if ln.startswith(keep) and "z-scores" in ln or
             ln.startswith(keep[:-1])]
    return lines, open(name).read()


@pytest.mark.parametrize("r", range(8))
def test_cli_matches_the_recorded_reference_cli(tmp_path, gold, r):
    spec = ast.literal_eval(str(gold["run%d" % r]))
    lines, text = cli_run(tmp_path, gold, r, spec, npy=(r % 2 == 1))
    assert lines == str(gold["run%d_stdout" % r]).splitlines()
    assert text == str(gold["run%d_file" % r])


def test_cli_assertions(tmp_path, gold):
    spec = dict(ast.literal_eval(str(gold["run1"])), thr=100000)
    with pytest.raises(AssertionError) as e:
        cli_run(tmp_path, gold, 1, spec)
    assert str(e.value) in str(gold["fail_none_message"])
    spec = dict(ast.literal_eval(str(gold["run1"])), ind_start=0)
    with pytest.raises(AssertionError) as e:
        cli_run(tmp_path, gold, 1, spec)
    assert str(e.value) in str(gold["fail_start0_message"])
    from wgsassign_amd import WGSassign
    with pytest.raises(SystemExit, match="outside the scope"):
        WGSassign.main(["--get_mcmc_mix", "--out", str(tmp_path / "x")])


def test_thin_mirror(gold):
    """zscore_cy.expected_W_l / variance_W_l with the reference's arguments."""
    from wgsassign_amd import zscore_cy
    L, AD, IDs, A = case_inputs(gold, "b")
    i = 3
    g = lambda k: gold["run4_i%d_%s" % (i, k)]
    keep = g("keep")
    wobs, wl, var = (np.zeros(len(keep), dtype=np.float32) for _ in range(3))
    zscore_cy.expected_W_l(L, keep, g("A"), AD, g("AD_array"), g("fac"), g("like"), g("index"), 1, i, wobs, wl)
    zscore_cy.variance_W_l(L, keep, g("A"), AD, g("AD_array"), g("fac"), g("like"), g("index"), 1, i, var, wl)
    same(wobs, g("wobs"), "W_l_obs")
    same(wl, g("wl"), "W_l")
    same(var, g("var"), "var_W_l")
