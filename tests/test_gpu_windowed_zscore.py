"""GPU: --get_assignment_z_score in site windows (wgsassign_amd/zscore.py: assignment_z_scores_windowed) held bit for bit to the
resident run on the same data and to the CPU restatement (tests/zscore_cpu.py): z, the three sums, kept counts, the dictionary
(keys, counts, means) and AD_array.  No tolerance anywhere.

The case: 20011 sites x 6 individuals against K = 3 frequency columns, the individuals in two populations of 4 and 2; windows of 8192
sites, so three windows with the last one ragged (3627 sites).  The inputs are tests/synth_deep.py's (depth 1.5, jitter 0.01: the 0.01
filter keeps about half the sites), with
  individual 2   every class of the depths 22 and 23 (kept deep depths), its deep sites on both sides of site 8192 and in window 3;
  individual 0   a class, (9, 3), whose only sites lie in window 2 and one, (3, 9), whose only sites lie in window 3;
  individual 5   no reads at all in window 2 (its depths are zeroed there): it keeps nothing in that window.
Every reference (the restatement, the resident run) is computed once per option set and shared."""
import contextlib
import io
import os

import numpy as np
import pytest

import synth
import synth_counts
import synth_deep
import synth_depth
import zscore_cpu
from test_zscore_cpu import same

pytestmark = pytest.mark.gpu

M, N, K, W = 20011, 6, 3, 8192
ROLES, SIZES = ("none", "dropped", "kept", "single", "dropped", "none"), (4, 2, 0)
LATE = {(9, 3): (9000, 9001, 12345), (3, 9): (17000, 20000)}        # individual 0: classes that first appear in window 2 / window 3
_case, _want, _resident, _files = [], {}, {}, {}


def case():
    if not _case:
        L, AD, IDs, A, deep = synth_deep.make_deep(M, N, K, 11, ROLES, sizes=SIZES)
        AD[W:2 * W, 10:12] = 0                                           # individual 5 has no reads in window 2
        for (Ar, Aa), sites in LATE.items():
            g0, g1 = synth_deep.class_triple(Ar, Aa)
            for s in sites:
                AD[s, 0:2] = (Ar, Aa)
                L[s, 0:2] = np.round(g0, 6), np.round(g1, 6)
        for a in (L, AD, A):
            a.setflags(write=False)
        _case.append((L, AD, IDs, A, deep))
    return _case[0]


def pops_of(IDs):
    return np.unique(IDs[:, 1])


def restatement(thr=0, srt=False, lo=None, hi=None):
    key = (thr, srt, lo, hi)
    if key not in _want:
        L, AD, IDs, A, _ = case()
        _want[key] = zscore_cpu.assignment(L, AD, IDs, pops_of(IDs), A, thr, srt, lo, hi)
    return _want[key]


def resident(thr=0, srt=False, lo=0, hi=None):
    """The resident run's (z, details, lines), once per option set."""
    key = (thr, srt, lo, hi)
    if key not in _resident:
        from wgsassign_amd import zscore
        from wgsassign_amd.device import AFSet, DeviceBeagle
        L, AD, IDs, A, _ = case()
        b = DeviceBeagle.from_host(L)
        depth = zscore.DepthTable(b, AD)
        afs = AFSet.from_host(A)
        details, lines = [], []
        try:
            z = zscore.assignment_z_scores(b, depth, IDs, pops_of(IDs), afs, thr, srt, lo, hi, batch=4, say=lines.append, details=details)
        finally:
            afs.close()
            depth.close()
            b.close()
        _resident[key] = (z, details, lines)
    return _resident[key]


def files(tmp_path_factory):
    """The case's files, written once: Beagle (gzip), frequencies, IDs, names, and the depth table as text, BGZF, .npy and as ANGSD
    counts with their selectors."""
    if not _files:
        L, AD, IDs, A, _ = case()
        d = tmp_path_factory.mktemp("zwin")
        paths = synth_depth.write_inputs(str(d / "in"), L, AD, IDs, A)
        text = open(paths["ad"], "rb").read()
        paths["ad_bgzf"] = str(d / "in.ad.bgzf.gz")
        synth.write_bgzf(paths["ad_bgzf"], text, block=20000)
        paths["ad_npy"] = str(d / "in.ad.npy")
        np.save(paths["ad_npy"], AD)
        short = text[:text.rstrip(b"\n").rfind(b"\n") + 1]
        paths["ad_short"] = str(d / "short.ad.txt")
        open(paths["ad_short"], "wb").write(short)
        rng = np.random.default_rng(8)
        majmin = np.empty((M, 2), dtype=np.int64)
        majmin[:, 0] = rng.integers(0, 4, size=M)
        majmin[:, 1] = (majmin[:, 0] + rng.integers(1, 4, size=M)) % 4
        counts = rng.poisson(0.1, size=(M, N, 4))
        counts[np.arange(M)[:, None], np.arange(N)[None, :], majmin[:, :1]] = AD[:, 0::2]
        counts[np.arange(M)[:, None], np.arange(N)[None, :], majmin[:, 1:]] = AD[:, 1::2]
        paths["counts"], paths["majmin"] = str(d / "in.counts.gz"), str(d / "in.majmin.txt")
        synth_counts.write_counts(paths["counts"], counts.reshape(M, 4 * N))
        synth_counts.write_majmin(paths["majmin"], majmin)
        paths["majmin_array"] = majmin.astype(np.uint8)
        paths["ad_text_bytes"] = len(text)
        _files.update(paths)
    return _files


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return files(tmp_path_factory)


def windowed(paths, depth="ad", thr=0, srt=False, lo=0, hi=None, window_sites=W, **kw):
    from wgsassign_amd import zscore
    L, AD, IDs, A, _ = case()
    details, lines = [], []
    Am = np.load(paths["af"], mmap_mode="r")
    z = zscore.assignment_z_scores_windowed(paths["beagle"], paths[depth], Am, IDs, pops_of(IDs), thr, srt, lo, hi, window_sites=window_sites,
                                            say=lines.append, details=details, **kw)
    return z, details, lines, dict(zscore.assignment_z_scores_windowed.stats)


def compare(got, thr=0, srt=False, lo=0, hi=None):
    z, details, lines, stats = got
    rz, rdetails, rlines = resident(thr, srt, lo, hi)
    want = restatement(thr, srt, lo or None, hi)
    assert len(details) == len(rdetails) == len(want) > 0
    assert z.dtype == rz.dtype and z.tobytes() == rz.tobytes()
    assert lines == rlines
    for i, (d, r, w) in enumerate(zip(details, rdetails, want)):
        tag = "individual %d " % (lo + i)
        for k in ("keys", "counts", "means", "AD_array", "fac", "like", "index"):
            same(d[k], r[k], tag + k + " (resident)")
            same(d[k], w[k], tag + k + " (restatement)")
        assert d["kept"] == len(r["keep"]) == len(w["keep"]), tag + "kept"
        for k in ("W_l_obs", "z_mu", "z_var", "z"):
            same(np.float32(d[k]), np.float32(r[k]), tag + k + " (resident)")
            same(np.float32(d[k]), np.float32(w[k]), tag + k + " (restatement)")
        assert not {"keep", "wobs", "wl", "var", "A"} & set(d), tag + "a per-site array"
    assert zscore_cpu.file_text(z[:, 0]) == zscore_cpu.file_text([w["z"] for w in want])


def test_the_case_is_what_it_claims():
    """Conditions on the inputs, checked on the restatement."""
    L, AD, IDs, A, deep = case()
    want = restatement()
    assert len(pops_of(IDs)) == 2 and A.shape == (M, K) and (M + W - 1) // W == 3 and M % W
    kept = [len(w["keep"]) for w in want]
    assert all(0.30 * M <= k <= 0.75 * M for k in kept[:5]), kept     # the filter keeps 30 - 75 % of the generated sites;
    assert 0.30 * (M - W) <= kept[5] <= 0.75 * (M - W), kept          # of individual 5's, outside the window that was emptied
    assert max(kept) > W
    per_window = [[int(((w["keep"] >= lo) & (w["keep"] < lo + W)).sum()) for lo in (0, W, 2 * W)] for w in want]
    assert per_window[5][1] == 0 and per_window[5][0] > 0 and per_window[5][2] > 0
    for (Ar, Aa), sites in LATE.items():
        where = np.flatnonzero((AD[:, 0] == Ar) & (AD[:, 1] == Aa))
        assert list(where) == list(sites)
        assert any((k == (Ar, Aa)).all() for k in want[0]["keys"])
    assert all(W <= s < 2 * W for s in LATE[(9, 3)]) and all(2 * W <= s for s in LATE[(3, 9)])
    assert sorted(set(int(d) for d in want[2]["AD_array"][:, 2] if d > 21)) == [22, 23]
    in_keep = deep[2][np.isin(deep[2], want[2]["keep"])]
    assert (in_keep < W).any() and ((in_keep >= W) & (in_keep < 2 * W)).any() and (in_keep >= 2 * W).any()


def test_three_windows(paths):
    got = windowed(paths, depth_chunk_bytes=65536)             # (chunks of the depth file straddle both window edges)
    compare(got)
    stats = got[3]
    assert stats["windows"] == 3 and stats["window_sites"] == W and stats["rounds"] == 1
    for key in ("depth_a", "depth_b"):                          # the depth file is read once per pass
        assert stats[key][0]["text_bytes"] == paths["ad_text_bytes"] and stats[key][0]["lines"] == M
        assert stats[key][0]["chunks"] > 6
    assert 0 < stats["downloaded_bytes"] <= N * (3 * 8191 * 4 + 3 * 4 + 3 * (253 * 20 + 4)) + 3 * 400 * 20


def test_threshold(paths):
    compare(windowed(paths, thr=3), thr=3)


def test_single_read_threshold(paths):
    compare(windowed(paths, srt=True), srt=True)


def test_individuals_inside_the_range(paths):
    compare(windowed(paths, lo=1, hi=4), lo=1, hi=4)


def test_rounds_of_individuals(paths):
    got = windowed(paths, batch=4)
    assert got[3]["rounds"] == 2 and got[2][0].startswith("wgsassign_amd: the z-scores of 6 individuals run in 2 rounds")
    compare((got[0], got[1], got[2][1:], got[3]))


def test_one_window(paths):
    got = windowed(paths, window_sites=24576)
    assert got[3]["windows"] == 1
    compare(got)


@pytest.mark.parametrize("depth", ["ad_bgzf", "ad_npy", "counts"])
def test_depth_file_formats(paths, depth):
    kw = dict(counts=True, majmin=paths["majmin_array"]) if depth == "counts" else {}
    got = windowed(paths, depth=depth, depth_chunk_bytes=65536, **kw)
    compare(got)
    if depth == "ad_bgzf":
        # the device-resident ingest counts the one newline it puts behind the file's last member (csrc/ingest.hip: size_chunk), as
        # it does for a resident table: the file's text once per pass and that byte, not a multiple of the text
        for key in ("depth_a", "depth_b"):
            assert got[3][key][0]["text_bytes"] == paths["ad_text_bytes"] + 1 and got[3][key][0]["lines"] == M
    if depth == "counts":
        assert got[3]["depth_a"][0]["lines"] == M


def test_a_depth_file_one_line_short(paths):
    with pytest.raises(ValueError, match=r"short\.ad\.txt has %d data lines, %d sites were expected" % (M - 1, M)):
        windowed(paths, depth="ad_short")


def test_command_line(paths, tmp_path, monkeypatch, capfd):
    """WGSASSIGN_Z_WINDOW_SITES=8192 against the resident run of the same command: the bytes of .z_ind.txt and the stdout lines."""
    from wgsassign_amd import WGSassign
    runs = {}
    for tag in ("resident", "windowed"):
        out = str(tmp_path / tag)
        argv = ["--beagle", paths["beagle"], "--pop_af_IDs", paths["ids"], "--pop_names", paths["names"], "--ind_ad_file", paths["ad"],
                "--out", out, "--get_assignment_z_score", "--pop_af_file", paths["af"]]
        if tag == "windowed":
            monkeypatch.setenv("WGSASSIGN_Z_WINDOW_SITES", str(W))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            WGSassign.main(argv)
        err = capfd.readouterr().err
        runs[tag] = (open(out + ".z_ind.txt", "rb").read(), buf.getvalue().replace(out, "OUT").splitlines(), err)
    assert runs["windowed"][0] == runs["resident"][0]
    assert runs["windowed"][1] == runs["resident"][1]
    assert "z-scores in 1 rounds of 2 passes over 3 windows of 8192 sites" in runs["windowed"][2]
    assert "z-scores in" not in runs["resident"][2]
    assert runs["resident"][0].decode() == zscore_cpu.file_text([w["z"] for w in restatement()])
