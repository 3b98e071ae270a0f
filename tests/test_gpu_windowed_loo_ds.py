"""--get_reference_af --loo --loo_downsampled_beagle in site windows (reader_cy.stream_windows(keep=), emMAF.emMAF_windowed(keep=),
glassy.loo_windowed(keep=, scored_path=, scored_keep=), device.LooStream.push(scored=), wgs_loo_stream_push_scored): two Beagle files
under two site masks, taken in windows of KEPT sites, give the log-likelihoods, partition sums, iteration counts, frequencies and
command-line outputs of the two resident masked matrices BIT FOR BIT -- every comparison here is of bytes, no tolerance.  The
yardstick is glassy.loo_device(beagle, scored, ...) on the two reader_cy.stream_to_device(..., keep=...) matrices with the resident
fit's frequencies; it is held to the oracle's leave-one-out run with downsampled_L once, at 5000 kept sites.

The files: a reference file and a downsampled file with the same site names, another seed and another depth (scoring the wrong
matrix changes every cell).  The downsampled file lacks the reference file's first row, its last row, the rows on either side of
kept sites 8191 and 8192 (so the window edge lies among dropped rows), and two runs of 400 and 500 consecutive rows; it holds rows of
its own (other names) at its start, at its end, around its own window edge and in a run.  Both masks are non-trivial."""
import contextlib
import gzip
import io
import os
import re

import numpy as np
import pytest

import synth
from conftest import GOLDEN
from test_gpu_windowed import beagle_text

pytestmark = pytest.mark.gpu
W1 = 8192
N, K = 12, 3
EDGE_MARGIN = 4         # first horizons of the re-fits of populations of four: see test_gpu_windowed_loo.py
KEPT = [20000, 16384, 5000]         # two full windows and a short one, an exact multiple, one window


def dropped_rows(kept):
    """File rows of the reference file (kept + len(rows) rows) that the downsampled file lacks."""
    m_ref = kept + 902 + (3 if kept > W1 + 2 else 0)
    drop = np.zeros(m_ref, dtype=bool)
    drop[0] = drop[m_ref - 1] = True
    drop[3000:3400] = True                      # a run of 400
    drop[m_ref - 700:m_ref - 200] = True        # a run of 500 in the last window
    if kept > W1 + 2:
        for j in (W1 - 2, W1 - 1, W1):          # the row after kept site 8190, after 8191 and after 8192, each as the masks stand then
            drop[np.flatnonzero(~drop)[j] + 1] = True
    assert int((~drop).sum()) == kept
    return drop


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """case(kept) -> (reference file, downsampled file, IDs, keep_ref, keep_ds)."""
    from wgsassign_amd import utils
    root = tmp_path_factory.mktemp("windowed_loo_ds")
    made = {}

    def case(kept):
        if kept not in made:
            drop = dropped_rows(kept)
            m_ref = len(drop)
            L, IDs = synth.make_beagle(m_ref, N, K, seed=4100 + N, interleave=True)
            D, _ = synth.make_beagle(m_ref, N, K, seed=977, depth=0.5, interleave=True)
            X, _ = synth.make_beagle(16, N, K, seed=31, depth=6.0, interleave=True)
            ref = beagle_text(L).split(b"\n")[:-1]
            ds = beagle_text(D).split(b"\n")[:-1]
            own = [ln.replace(b"chr1_", b"chrX_", 1) for ln in beagle_text(X).split(b"\n")[1:-1]]
            lines = [ds[0], own[0]]             # the downsampled file begins with a row the reference file lacks
            shared = 0
            for r in range(m_ref):
                if drop[r]:
                    continue
                if shared in (W1 - 1, W1, W1 + 1):
                    lines.append(own[1 + shared - (W1 - 1)])       # rows of its own on both sides of its window edge
                if shared == 1000:
                    lines.extend(own[4:9])                          # a run of five
                lines.append(ds[1 + r])
                shared += 1
            lines.append(own[9])                # ... and ends with one
            p_ref, p_ds = str(root / ("ref%d.beagle.gz" % kept)), str(root / ("ds%d.beagle.gz" % kept))
            with gzip.open(p_ref, "wb", compresslevel=1) as fh:
                fh.write(b"\n".join(ref) + b"\n")
            with gzip.open(p_ds, "wb", compresslevel=1) as fh:
                fh.write(b"\n".join(lines) + b"\n")
            names_ref = [ln.split(b"\t", 1)[0].decode() for ln in ref[1:]]
            names_ds = [ln.split(b"\t", 1)[0].decode() for ln in lines[1:]]
            keep_ref = utils.site_mask(names_ref, names_ds)
            keep_ds = utils.site_mask(names_ds, [x for x, k in zip(names_ref, keep_ref) if k])
            assert (keep_ref == ~drop).all() and int(keep_ds.sum()) == kept and not keep_ds[0] and not keep_ds[-1]
            assert not keep_ref.all() and not keep_ds.all()
            made[kept] = (p_ref, p_ds, IDs, keep_ref, keep_ds, names_ref, names_ds)
        return made[kept][:5]
    case.root = root
    case.names = lambda kept: made[kept][5:]
    return case


@pytest.fixture(autouse=True)
def _private_index_cache(files, monkeypatch):
    monkeypatch.setenv("WGSASSIGN_INDEX_DIR", str(files.root))
    for name in ("WGSASSIGN_WINDOW_SITES", "WGSASSIGN_LOO_WINDOW_SITES", "WGSASSIGN_LOO_DS_WINDOW_SITES"):
        monkeypatch.delenv(name, raising=False)


def groups(IDs):
    pops = np.unique(IDs[:, 1])
    return np.searchsorted(pops, IDs[:, 1]).astype(np.int32)


_fits, _resident = {}, {}


def resident_fit(path, IDs, keep, maf_iter=200, tole=1e-4):
    """(af clamped, population iters) of emMAF_populations on the resident masked matrix: once per file, never changed."""
    from wgsassign_amd import emMAF, reader_cy
    key = (path, maf_iter, tole)
    if key not in _fits:
        beagle, _, _, m = reader_cy.stream_to_device(path, groups(IDs), K, keep=keep)
        with contextlib.redirect_stdout(io.StringIO()):
            _, af, iters = emMAF.emMAF_populations(None, IDs, maf_iter, tole, beagle=beagle)
        beagle.close()
        assert af.shape == (int(keep.sum()), K) and m == af.shape[0]
        af.setflags(write=False)
        _fits[key] = (af, np.asarray(iters).copy())
    return _fits[key]


def resident_loo(case, P, scored=True, maf_iter=200, tole=1e-4):
    """(af, population iters, logl, parts, iters) of glassy.loo_device over the two resident masked matrices (scored=False: the
    reference file's matrix is scored, the mistake the inputs must be able to show): once per case and setting, never changed."""
    from wgsassign_amd import glassy, reader_cy
    p_ref, p_ds, IDs, keep_ref, keep_ds = case
    key = (p_ref, P, scored, maf_iter, tole)
    if key not in _resident:
        af, pop_iters = resident_fit(p_ref, IDs, keep_ref, maf_iter, tole)
        group_of = groups(IDs)
        beagle, _, _, _ = reader_cy.stream_to_device(p_ref, group_of, K, keep=keep_ref)
        other = reader_cy.stream_to_device(p_ds, group_of, K, keep=keep_ds)[0] if scored else beagle
        tm = {}
        logl, parts = glassy.loo_device(beagle, other, af.copy(), group_of, maf_iter, tole, P, verbose=False, timings=tm)
        if other is not beagle:
            other.close()
        beagle.close()
        for a in (logl, parts):
            a.setflags(write=False)
        _resident[key] = (af, pop_iters, logl, parts, np.asarray(tm["iters"]).copy())
    return _resident[key]


def check(case, P, margin=EDGE_MARGIN):
    from wgsassign_amd import glassy
    p_ref, p_ds, IDs, keep_ref, keep_ds = case
    af, pop_iters, logl_r, parts_r, iters_r = resident_loo(case, P)
    first = glassy.loo_first_iters(groups(IDs), pop_iters, 200, margin=margin)
    before = af.tobytes()
    logl, parts, iters = glassy.loo_windowed(p_ref, af, IDs, 200, 1e-4, W1, P, first_iters=first, keep=keep_ref, scored_path=p_ds,
                                             scored_keep=keep_ds)
    stats = glassy.loo_windowed.stats
    print("windowed", list(iters), "resident", list(iters_r), "stats", {k: v for k, v in stats.items() if k != "round_seconds"})
    assert list(iters) == list(iters_r)
    assert logl.dtype == np.float32 and logl.shape == (N, K) and logl.tobytes() == logl_r.tobytes()
    assert parts.dtype == np.float32 and parts.shape == (N * P, K) and parts.tobytes() == parts_r.tobytes()
    assert af.tobytes() == before
    assert stats["refit_bytes_to_host"] == 0 and stats["scored_passes"] == 1 and stats["matrices"] <= 4
    assert glassy.loo_windowed.info["m"] == int(keep_ref.sum())
    return stats


@pytest.mark.parametrize("kept", KEPT)
def test_stream_windows_under_a_mask(files, kept):
    """Every window's rows are the resident masked matrix's rows of that range, for both files; site0, m, the window count and the
    eight names are those of kept sites."""
    from wgsassign_amd import reader_cy
    p_ref, p_ds, IDs, keep_ref, keep_ds = files(kept)
    group_of = groups(IDs)
    for path, keep, names in zip((p_ref, p_ds), (keep_ref, keep_ds), files.names(kept)):
        beagle, _, resident_names, m = reader_cy.stream_to_device(path, group_of, K, keep=keep)
        assert m == kept and beagle.m == kept
        info, seen = {}, 0
        gen = reader_cy.stream_windows(path, W1, info=info, group_of=group_of, n_groups=K, keep=keep)
        for w, b in enumerate(gen):
            assert b.site0 == w * W1 == seen and b.m == min(W1, kept - seen) and b.n == N
            assert b.download_rows(0, b.m).tobytes() == beagle.download_rows(seen, b.m).tobytes(), (path, w)
            seen += b.m
        gen.close()
        beagle.close()
        kept_names = [x for x, k in zip(names, keep) if k]
        assert seen == kept and info["m"] == kept and info["windows"] == -(-kept // W1) and info["matrices"] == min(2, info["windows"])
        assert info["site_names"] == kept_names[:4] + kept_names[-4:] == resident_names[:4] + resident_names[-4:]
        assert info["n"] == N and len(info["sample_names"]) == N


def test_masks_that_cannot_be(files):
    from wgsassign_amd import emMAF, glassy, reader_cy
    p_ref, p_ds, IDs, keep_ref, keep_ds = files(5000)
    with pytest.raises(ValueError, match="the site mask has %d entries, .* holds %d sites" % (len(keep_ref) - 1, len(keep_ref))):
        next(reader_cy.stream_windows(p_ref, W1, keep=keep_ref[:-1]))
    with pytest.raises(ValueError, match="holds no sites"):
        next(reader_cy.stream_windows(p_ref, W1, keep=np.zeros(len(keep_ref), dtype=bool)))
    with pytest.raises(ValueError, match="the site mask has"):
        emMAF.emMAF_windowed(p_ref, IDs, 200, 1e-4, W1, keep=keep_ds)
    af = resident_fit(p_ref, IDs, keep_ref)[0]
    with pytest.raises(ValueError, match="scored_keep is the site mask of scored_path"):
        glassy.loo_windowed(p_ref, af, IDs, 200, 1e-4, W1, keep=keep_ref, scored_keep=keep_ds)
    fewer = keep_ds.copy()
    fewer[np.flatnonzero(fewer)[7]] = False
    with pytest.raises(ValueError, match="Site names in full and downsampled Beagle do not match after filtering."):
        glassy.loo_windowed(p_ref, af, IDs, 200, 1e-4, W1, keep=keep_ref, scored_path=p_ds, scored_keep=fewer)
    renamed = str(files.root / "renamed.beagle.gz")
    text = gzip.open(p_ds, "rb").read()
    with gzip.open(renamed, "wb", compresslevel=1) as fh:
        fh.write(text.replace(b"\tInd3\tInd3\tInd3\t", b"\tIndX\tIndX\tIndX\t", 1))
    with pytest.raises(ValueError, match="Sample names in downsampled Beagle file do not match original."):
        glassy.loo_windowed(p_ref, af, IDs, 200, 1e-4, W1, keep=keep_ref, scored_path=renamed, scored_keep=keep_ds)


@pytest.mark.parametrize("kept", KEPT)
def test_fit_under_a_mask(files, kept):
    from wgsassign_amd import emMAF
    p_ref, _, IDs, keep_ref, _ = files(kept)
    af_r, iters_r = resident_fit(p_ref, IDs, keep_ref)
    af, iters = emMAF.emMAF_windowed(p_ref, IDs, 200, 1e-4, W1, keep=keep_ref)
    info, stats = emMAF.emMAF_windowed.info, emMAF.emMAF_windowed.stats
    assert list(iters) == list(iters_r) and all(i > 0 for i in iters)
    assert af.shape == (kept, K) and af.dtype == np.float32 and af.tobytes() == af_r.tobytes()
    assert info["m"] == kept and stats["windows"] == -(-kept // W1) and stats["matrices"] == min(2, stats["windows"])


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("kept, windows", [(20000, 3), (16384, 2), (5000, 1)])
def test_window_edges(files, monkeypatch, kept, windows, P):
    from wgsassign_amd import device
    from wgsassign_amd import windows as wplan

    def never(self, *a, **kw):
        raise AssertionError("EMStream.push copies final fits to the host")
    monkeypatch.setattr(device.EMStream, "push", never)
    case = files(kept)
    stats = check(case, P)
    assert stats["windows"] == windows and stats["window_sites"] == W1 and stats["rounds"] >= 2
    assert stats["matrices"] == 2 * min(2, windows)
    counts = np.unique(case[2][:, 1], return_counts=True)[1]
    assert 0 < stats["largest_matrix_bytes"] <= W1 * wplan.loo_ds_site_bytes(N, K, counts, P)


def test_more_partitions_than_the_block_parallel_chains_take(files):
    from wgsassign_amd import device
    check(files(16384), device.MAX_BLOCK_PARALLEL_PARTS + 1)


@pytest.mark.parametrize("P", [1, 3])
def test_scoring_the_reference_windows_by_mistake_shows(files, P):
    """Without the scored file the windows of the reference file are scored: the bytes of THAT resident run, and not one cell of the
    downsampled run's -- so a stream that scored the wrong matrix could not pass the tests above."""
    from wgsassign_amd import glassy
    case = files(20000)
    p_ref, p_ds, IDs, keep_ref, keep_ds = case
    af, pop_iters, logl_r, parts_r, iters_r = resident_loo(case, P)
    _, _, logl_own, parts_own, _ = resident_loo(case, P, scored=False)
    first = glassy.loo_first_iters(groups(IDs), pop_iters, 200, margin=EDGE_MARGIN)
    logl, parts, iters = glassy.loo_windowed(p_ref, af, IDs, 200, 1e-4, W1, P, first_iters=first, keep=keep_ref)
    assert glassy.loo_windowed.stats["scored_passes"] == 0 and glassy.loo_windowed.stats["matrices"] == 2
    assert list(iters) == list(iters_r)
    assert logl.tobytes() == logl_own.tobytes() and parts.tobytes() == parts_own.tobytes()
    assert (logl != logl_r).all() and (parts != parts_r).all()


def test_held_to_the_oracle(files, oracle):
    """The yardstick against the oracle's leave-one-out run with downsampled_L, over the kept rows as the host reader parses them."""
    from wgsassign_amd import reader_cy
    case = files(5000)
    p_ref, p_ds, IDs, keep_ref, keep_ds = case
    L = np.ascontiguousarray(reader_cy.readBeagle(p_ref)[0][keep_ref])
    D = np.ascontiguousarray(reader_cy.readBeagle(p_ds)[0][keep_ds])
    _, af_o, _, pop_iters_o = oracle.fit_reference_af(L, IDs, 200, 1e-4, t=2)
    for P in (1, 3):
        af, pop_iters, logl, parts, _ = resident_loo(case, P)
        assert list(pop_iters) == list(pop_iters_o) and af.tobytes() == af_o.tobytes()
        logl_o, parts_o = oracle.loo(L, af_o.copy(), IDs, 2, 200, 1e-4, downsampled_L=D, num_partitions=P)
        assert logl.tobytes() == logl_o.tobytes() and parts.tobytes() == parts_o.tobytes()


def test_push_scored_refusals_launch_nothing():
    from wgsassign_amd import device, glassy
    P = 3
    group_of = np.asarray([i % K for i in range(N)], dtype=np.int32)
    b = device.DeviceBeagle(W1, N, group_of, K, site0=0)
    b.synth(11, 2.0)
    em = b.window_em = device.EMBatch(b, group_of, np.arange(N, dtype=np.int32))
    twin = device.DeviceBeagle(W1, N, group_of, K, site0=0)
    twin.synth(12, 0.5)
    A = np.random.default_rng(5).uniform(0.05, 0.95, size=(W1, K)).astype(np.float32)
    afs = device.AFSet.from_host(A)
    st = device.LooStream(N, K, W1, P)
    short = device.DeviceBeagle(100, N, group_of, K, site0=0)
    with pytest.raises(ValueError, match="the scored window holds 100 sites, the fitted window 8192"):
        st.push(em, afs, scored=short)
    short.close()
    twin.set_window(W1)
    with pytest.raises(ValueError, match="the scored window starts at site 8192, the fitted window at site 0"):
        st.push(em, afs, scored=twin)
    twin.set_window(0)
    other_groups = np.roll(group_of, 1)
    regrouped = device.DeviceBeagle(W1, N, other_groups, K, site0=0)
    with pytest.raises(ValueError, match="individual 0 is of population 2 in the scored window, of population 0 in the fitted one"):
        st.push(em, afs, scored=regrouped)
    regrouped.close()
    one_group = device.DeviceBeagle(W1, N, site0=0)
    with pytest.raises(ValueError, match="the scored window has 1 population slabs, the fitted window 3"):
        st.push(em, afs, scored=one_group)
    one_group.close()
    other_n = device.DeviceBeagle(W1, N + 1, np.append(group_of, 0).astype(np.int32), K, site0=0)
    with pytest.raises(ValueError, match="the scored window holds 13 individuals, the fitted window 12"):
        st.push(em, afs, scored=other_n)
    other_n.close()
    with pytest.raises(ValueError, match="only 0 of the 8192 sites were pushed"):
        st.finish()
    assert em.sweep_paths() == [0, 0, 0, 0] and st.windows == 0 and twin.codes_state() == 0 and b.codes_state() == 0    # nothing was swept
    # the stream is as it was: the proper push ends in the bits of the step-wise resident scoring of the twin
    fits = device.EMStream(N, 10, W1)
    lo = np.float32(1 / (2 * (np.bincount(group_of)[group_of] - 1 + 1)))
    fits.push_keep(em, np.full(N, 5, dtype=np.int32), np.ones(N, dtype=np.int32), lo, np.float32(1) - lo, sums_from=np.zeros(N, dtype=np.int32))
    want, want_parts = glassy.score_loo_batch(twin, afs, em, group_of, 0, N, P)
    own, own_parts = glassy.score_loo_batch(b, afs, em, group_of, 0, N, P)
    st.push(em, afs, scored=twin)
    out, parts = st.finish()
    assert out.tobytes() == want.tobytes() and parts.tobytes() == want_parts.tobytes()
    assert (out != own).all() and (parts != own_parts).all()
    # ... and scored = the fitted matrix itself is the plain push
    again = device.LooStream(N, K, W1, P)
    again.push(em, afs, scored=b)
    out, parts = again.finish()
    assert out.tobytes() == own.tobytes() and parts.tobytes() == own_parts.tobytes()
    for obj in (again, st, fits, afs, em, twin, b):
        obj.close()


def run_cli(argv):
    from wgsassign_amd import WGSassign
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        WGSassign.main(argv)
    return out.getvalue(), err.getvalue()


def same_files(a, b, P):
    for name in (".pop_af.npy", ".pop_names.txt", ".pop_like_LOO_downsampled.tsv"):
        assert open(a + name, "rb").read() == open(b + name, "rb").read(), name
    if P > 1:
        name = ".pop_like_LOO_downsampled_partitions_%d.tsv.gz" % P
        assert gzip.open(a + name, "rb").read() == gzip.open(b + name, "rb").read()


def test_command_line_on_the_recorded_run(tmp_path, monkeypatch, golden):
    """Both amre files with WGSASSIGN_LOO_DS_WINDOW_SITES=8192: stdout, .pop_af.npy and the TSV of the reference's own record, and the files of
    the resident run.  With --partition_sites 3
    against the resident run, file for file."""
    g = golden("amre_cli_downsampled.npz")
    data = os.path.join(GOLDEN, "data")
    breed = os.path.join(data, "amre.breeding.ind85.ds_2x.sites-filter.top_50_each.beagle.gz")
    ds = os.path.join(data, "amre.breeding.ind85.ds_2x.sites-filter.top_50_each_subset_80percent_sites.beagle.gz")
    ids = os.path.join(data, "amre.breeding.ind85.reference_k5.IDs.txt")
    argv = ["--beagle", breed, "--pop_af_IDs", ids, "--get_reference_af", "--loo", "--loo_downsampled_beagle", ds, "--threads", "2"]
    res, win = str(tmp_path / "res"), str(tmp_path / "win")
    out1, err1 = run_cli(argv + ["--out", res])
    monkeypatch.setenv("WGSASSIGN_LOO_DS_WINDOW_SITES", "8192")
    out2, err2 = run_cli(argv + ["--out", win])
    assert "window" not in err1
    said = [l for l in err2.splitlines() if "window" in l]
    assert len(said) == 1 and re.fullmatch(r"wgsassign_amd: leave-one-out on downsampled likelihoods in \d+ rounds of 1 windows of 8192 kept sites "
                                           r"\(the downsampled file read 1 time\)", said[0]), said
    assert np.load(win + ".pop_af.npy").tobytes() == g["pop_af_npy"].tobytes()
    assert [l.replace(str(tmp_path) + "/win", "ds") for l in out2.splitlines()] == str(g["stdout"]).replace("<TMP>/", "").splitlines()
    assert out1.replace(res, "OUT") == out2.replace(win, "OUT")
    same_files(res, win, 1)
    assert open(win + ".pop_like_LOO_downsampled.tsv").read() == str(g["loo_tsv"])
    res3, win3 = str(tmp_path / "res3"), str(tmp_path / "win3")
    out4, _ = run_cli(argv + ["--partition_sites", "3", "--out", win3])
    monkeypatch.delenv("WGSASSIGN_LOO_DS_WINDOW_SITES")
    out3, err3 = run_cli(argv + ["--partition_sites", "3", "--out", res3])
    assert "window" not in err3 and out3.replace(res3, "OUT") == out4.replace(win3, "OUT")
    same_files(res3, win3, 3)


def test_command_line_on_three_windows(files, tmp_path, monkeypatch):
    """The synthetic pair of 20000 kept sites through the command line, resident and in windows: the same stdout and files; other
    variables route nothing; with --ne_obs beside the options the run stays resident."""
    p_ref, p_ds, IDs, keep_ref, keep_ds = files(20000)
    ids = str(tmp_path / "ids.txt")
    np.savetxt(ids, IDs, fmt="%s", delimiter="\t")
    argv = ["--beagle", p_ref, "--pop_af_IDs", ids, "--get_reference_af", "--loo", "--loo_downsampled_beagle", p_ds, "--partition_sites", "3",
            "--threads", "2"]
    monkeypatch.setenv("WGSASSIGN_LOO_WINDOW_SITES", "8192")
    monkeypatch.setenv("WGSASSIGN_WINDOW_SITES", "8192")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    out1, err1 = run_cli(argv + ["--out", a])
    assert "window" not in err1
    monkeypatch.setenv("WGSASSIGN_LOO_DS_WINDOW_SITES", "8192")
    out2, err2 = run_cli(argv + ["--out", b])
    said = [l for l in err2.splitlines() if "window" in l]
    assert len(said) == 1 and re.fullmatch(r"wgsassign_amd: leave-one-out on downsampled likelihoods in \d+ rounds of 3 windows of 8192 kept sites "
                                           r"\(the downsampled file read 1 time\)", said[0]), said
    assert out1.replace(a, "OUT") == out2.replace(b, "OUT")
    assert out2.count("EM (MAF) converged at iteration") == K + N and out2.count("Filtered out") == 2
    assert "\tFiltered out %d sites" % int((~keep_ref).sum()) in out2 and "\tFiltered out %d sites" % int((~keep_ds).sum()) in out2
    same_files(a, b, 3)
    assert np.load(b + ".pop_af.npy").shape == (20000, K)
    c = str(tmp_path / "c")
    out3, err3 = run_cli(argv + ["--ne_obs", "--out", c])
    assert "window" not in err3
    assert open(a + ".pop_like_LOO_downsampled.tsv", "rb").read() == open(c + ".pop_like_LOO_downsampled.tsv", "rb").read()
