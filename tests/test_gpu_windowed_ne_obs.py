"""--ne_obs in site windows (fisher.fisher_obs_windowed, device.FisherStream, wgs_fisher_stream_*, fisher_window_kernel): a Beagle
file taken in consecutive windows, in one pass, gives f_obs, ne_obs, the population means and the per-individual means of its resident
matrix BIT FOR BIT -- every comparison here is of bytes, no tolerance.  The yardstick is fisher.fisher_obs / fisher.fisher_obs_ind on
the matrix reader_cy.stream_to_device makes of the same file, with the same frequencies, and np.mean(ne_obs, axis=0) of its result;
tests/test_gpu_fisher.py holds those to the golden vectors of the reference."""
import contextlib
import gzip
import io
import os

import numpy as np
import pytest

import synth
from test_gpu_windowed import beagle_text

pytestmark = pytest.mark.gpu
W1 = 8192
N, K = 12, 3
ODD = [2, 1, 2, 0, 2, 1, 2, 1, 2, 2, 1, 2]               # populations of 1, 4 and 7: two odd slabs, a population of one


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """case(m, odd_first=False, odd=False) -> (gzipped Beagle file, IDs, L): populations interleaved in file order, so a total filed
    under the slab column instead of the individual shows; odd_first: the first 8192 sites are of another depth than the rest; odd:
    populations of 1, 4 and 7."""
    root = tmp_path_factory.mktemp("windowed_ne")
    made = {}

    def case(m, odd_first=False, odd=False):
        key = (m, odd_first, odd)
        if key not in made:
            if odd:
                L, IDs = synth.make_beagle_for_labels(m, ODD, K, seed=5200 + N)
            else:
                L, IDs = synth.make_beagle(m, N, K, seed=5200 + N, interleave=True)
            if odd_first:
                L[:W1] = synth.make_beagle(W1, N, K, seed=78, depth=12.0, interleave=True)[0]
            path = str(root / ("m%d_%d_%d.beagle.gz" % (m, odd_first, odd)))
            with gzip.open(path, "wb", compresslevel=1) as fh:
                fh.write(beagle_text(L))
            made[key] = (path, IDs, L)
        return made[key]
    case.root = root
    return case


@pytest.fixture(autouse=True)
def _private_index_cache(files, monkeypatch):
    monkeypatch.setenv("WGSASSIGN_INDEX_DIR", str(files.root))
    for name in ("WGSASSIGN_WINDOW_SITES", "WGSASSIGN_LOO_WINDOW_SITES", "WGSASSIGN_NE_WINDOW_SITES"):
        monkeypatch.delenv(name, raising=False)


def frequencies(m, IDs, bounds=False):
    """(m, K) float32 inside the clamp of WGSassign.py:236-240; bounds: every seventh site at the lower bound and every eleventh at the
    upper one, per population."""
    counts = np.unique(IDs[:, 1], return_counts=True)[1]
    lo = (1.0 / (2.0 * counts)).astype(np.float32)
    hi = (np.float32(1) - lo).astype(np.float32)
    rng = np.random.default_rng(m + 17 * len(counts))
    af = np.clip(rng.random((m, len(counts))).astype(np.float32), lo, hi).astype(np.float32)
    if bounds:
        for k in range(len(counts)):
            af[k::7, k] = lo[k]
            af[k + 3::11, k] = hi[k]
    return af


_resident = {}


def resident(path, IDs, af, tag=""):
    """(f_obs, ne_obs, np.mean(ne_obs, axis=0), ne_ind) of the resident matrix of the file: computed once per file and frequencies,
    never changed."""
    from wgsassign_amd import fisher, reader_cy
    key = (path, tag)
    if key not in _resident:
        pops = np.unique(IDs[:, 1])
        group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
        beagle, _, _, m = reader_cy.stream_to_device(path, group_of, len(pops), names="ends")
        f_obs, ne_obs = fisher.fisher_obs(None, af, IDs, 1, beagle=beagle)
        ne_ind = fisher.fisher_obs_ind(None, af, IDs, 1, beagle=beagle)
        beagle.close()
        out = (f_obs, ne_obs, np.mean(ne_obs, axis=0), ne_ind)
        for a in out:
            a.setflags(write=False)
        _resident[key] = out
    return _resident[key]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(path, IDs, window=W1, bounds=False, out=None):
    from wgsassign_amd import fisher
    m = resident_sites(path)
    af = frequencies(m, IDs, bounds)
    want = resident(path, IDs, af, "bounds" if bounds else "")
    got = fisher.fisher_obs_windowed(path, af, IDs, window, out=out)
    stats = fisher.fisher_obs_windowed.stats
    print("windowed --ne_obs:", {k: v for k, v in stats.items()})
    for name, g, w in zip(("f_obs", "ne_obs", "ne_obs_mean", "ne_ind"), got, want):
        g = np.asarray(g)
        assert g.dtype == np.float32 and g.shape == w.shape, name
        bad = np.flatnonzero(g.view(np.uint32).ravel() != w.view(np.uint32).ravel())
        assert bad.size == 0, "%s: %d of %d values differ from the resident run, first at flat index %d: %r != %r" % (
            name, bad.size, w.size, bad[0], g.ravel()[bad[0]], w.ravel()[bad[0]])
    assert np.isfinite(want[3]).all() and (want[3] > 0).all()
    return stats, got


_sites = {}


def resident_sites(path):
    from wgsassign_amd import reader_cy
    if path not in _sites:
        _sites[path] = reader_cy.ensure_index(path)[2]
    return _sites[path]


@pytest.mark.parametrize("m, window, windows", [(20000, W1, 3), (16384, W1, 2), (8193, W1, 2), (8199, W1, 2), (8200, W1, 2), (8321, W1, 2),
                                                (5000, W1, 1), (24576, 2 * W1, 2)])
def test_window_edges(files, m, window, windows):
    """20000: three windows, a last chunk of 3616 sites (irregular leaves, a partial tile); 16384: no row route at all; 8193, 8199,
    8200: last chunks of 1, 7 and 8 sites (the leaf of fewer than 8 elements and the first with accumulators); 8321: 129, the first
    split; 5000: one short window, the fused sweep gives f_obs / ne_obs only; 24576 in windows of 16384: two chunks inside a push,
    then a one-chunk window."""
    from wgsassign_amd import windows as wplan
    path, IDs, _ = files(m)
    stats, _ = check(path, IDs, window)
    assert stats["windows"] == windows and stats["window_sites"] == window
    assert stats["matrices"] == min(2, windows) and stats["seconds"] > 0 and len(stats["sweep_ms"]) == windows
    counts = np.unique(IDs[:, 1], return_counts=True)[1]
    assert 0 < stats["largest_matrix_bytes"] <= window * wplan.ne_site_bytes(N, K, counts)


@pytest.mark.parametrize("m", [20000, 16384, 8193])
def test_odd_slabs_and_a_population_of_one(files, m):
    path, IDs, _ = files(m, odd=True)
    assert sorted(np.unique(IDs[:, 1], return_counts=True)[1]) == [1, 4, 7]
    check(path, IDs)


def test_a_first_window_unlike_the_rest(files):
    path, IDs, _ = files(20000, odd_first=True)
    check(path, IDs)


def test_frequencies_at_both_clamp_bounds(files):
    path, IDs, _ = files(20000)
    check(path, IDs, bounds=True)
    path, IDs, _ = files(20000, odd=True)
    check(path, IDs, bounds=True)


def test_bgzf(files, tmp_path):
    src, IDs, _ = files(20000)
    path = str(tmp_path / "copy.beagle.gz")
    synth.write_bgzf(path, gzip.open(src, "rb").read(), block=50000)
    check(path, IDs)


def test_results_written_window_by_window(files, tmp_path):
    """With `out` the two (m, K) results are .npy files np.load reads, byte for byte what np.save writes of the resident arrays."""
    path, IDs, _ = files(20000)
    out = str(tmp_path / "w")
    _, got = check(path, IDs, out=out)
    want = resident(path, IDs, None)
    del got
    for suffix, w in ((".fisher_obs.npy", want[0]), (".ne_obs.npy", want[1])):
        ref = str(tmp_path / "r") + suffix
        np.save(ref, w)
        assert open(out + suffix, "rb").read() == open(ref, "rb").read(), suffix


def test_against_the_oracle(files, oracle):
    """m = 20000 against the reference's arithmetic itself, not only the resident path."""
    from wgsassign_amd import fisher
    path, IDs, L = files(20000)
    af = frequencies(20000, IDs)
    f_obs, ne_obs, mean, ne_ind = fisher.fisher_obs_windowed(path, af, IDs, W1)
    f_o, ne_o = oracle.fisher_obs(L, af.copy(), IDs, 1)
    assert same(np.asarray(f_obs), f_o) and same(np.asarray(ne_obs), ne_o)
    assert same(mean, np.mean(ne_o, axis=0))
    assert same(ne_ind, oracle.fisher_obs_ind(L, af.copy(), IDs, 1))


def test_misuse_is_refused_and_launches_nothing():
    from wgsassign_amd import device, fisher
    group_of = np.asarray([i % K for i in range(N)], dtype=np.int32)
    IDs = np.asarray([("Ind%d" % i, "pop%02d" % g) for i, g in enumerate(group_of)])
    b = device.DeviceBeagle(W1, N, group_of, K, site0=W1)
    b.synth(11, 2.0)
    A = frequencies(W1 + 100, IDs)
    afs = device.AFSet.from_host(np.ascontiguousarray(A[:W1]))
    st = device.FisherStream(N, K, W1 + 100)
    with pytest.raises(ValueError, match="starts at site 8192, but 0 sites were pushed so far"):       # a window out of order
        st.push(b, afs)
    b.set_window(100)
    with pytest.raises(ValueError, match="starts at site 100, which is not a multiple of 8192"):
        st.push(b, afs)
    with pytest.raises(ValueError, match="only 0 of the 8292 sites were pushed"):                      # finish before the last window
        st.finish()
    b.set_window(0)
    wrong_k = device.AFSet.from_host(np.ascontiguousarray(A[:W1, :2]))
    with pytest.raises(ValueError, match="12 individuals x 2 populations, the Fisher stream 12 x 3"):
        st.push(b, wrong_k)
    wrong_k.close()
    short_af = device.AFSet.from_host(np.ascontiguousarray(A[W1:]))
    with pytest.raises(ValueError, match="allele frequencies cover 100 SNPs, the window 8192"):
        st.push(b, short_af)
    one_group = device.DeviceBeagle(W1, N)
    with pytest.raises(ValueError, match="1 population slabs, the Fisher stream 3 populations"):
        st.push(one_group, afs)
    one_group.close()
    gap = device.DeviceBeagle(W1, N, np.where(group_of == 1, 0, group_of).astype(np.int32), K)
    with pytest.raises(ValueError, match="population 1 has no individuals"):
        st.push(gap, afs)
    gap.close()
    other_n = device.FisherStream(N + 1, K, W1)
    with pytest.raises(ValueError, match="12 individuals x 3 populations, the Fisher stream 13 x 3"):
        other_n.push(b, afs)
    other_n.close()
    small = device.FisherStream(N, K, 5000)
    with pytest.raises(ValueError, match="8192 sites after 0 pushed exceed the 5000 sites"):
        small.push(b, afs)
    small.close()
    assert st.windows == 0
    # the stream is still usable: a full window and a short one, against the resident functions on the two matrices
    f0, ne0 = st.push(b, afs)
    with pytest.raises(ValueError, match="only 8192 of the 8292 sites were pushed"):
        st.finish()
    short = device.DeviceBeagle(100, N, group_of, K, site0=W1)
    short.synth(12, 2.0)
    long = device.FisherStream(N, K, 3 * W1)
    long.push(b, afs)
    with pytest.raises(ValueError, match="a window of 100 sites that is not the last one"):
        long.push(short, short_af)
    long.close()
    f1, ne1 = st.push(short, short_af)
    want0 = fisher.fisher_obs(None, A[:W1], IDs, 1, beagle=b)
    want1 = fisher.fisher_obs(None, A[W1:], IDs, 1, beagle=short)
    assert same(f0, want0[0]) and same(ne0, want0[1]) and same(f1, want1[0]) and same(ne1, want1[1])
    ne_ind = st.finish()
    # one 8192-site chunk and a short one: np.mean's total is the first chunk's sum with the second added to it
    def chunk_sums(beagle, af_rows):
        """NumPy's float32 sum of every individual's terms over one matrix of at most 8192 sites (wgs_fisher_ind_sums, no carry)."""
        from wgsassign_amd import _lib
        a = device.AFSet.from_host(np.ascontiguousarray(af_rows))
        out = np.zeros(N, dtype=np.float32)
        for i in range(N):
            one = np.zeros(1, dtype=np.float32)
            _lib.check(_lib.load().wgs_fisher_ind_sums(beagle.handle, a.handle, i, 1, None, _lib.f32p(one)))
            out[i] = one[0]
        a.close()
        return out
    total = chunk_sums(b, A[:W1]) + chunk_sums(short, A[W1:])
    assert total.dtype == np.float32 and same(ne_ind, (total.astype(np.float64) / (W1 + 100)).astype(np.float32))
    assert np.isfinite(ne_ind).all() and (ne_ind > 0).all() and len(set(ne_ind.tolist())) == N
    with pytest.raises(ValueError, match="finished already"):                                          # a second finish
        st.finish()
    with pytest.raises(ValueError, match="takes no further window"):
        st.push(b, afs)
    st.close()
    st.close()
    for obj in (short_af, afs, short, b):
        obj.close()


def run_cli(argv):
    from wgsassign_amd import WGSassign
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        WGSassign.main(argv)
    return out.getvalue(), err.getvalue()


NE_FILES = (".pop_af.npy", ".pop_names.txt", ".fisher_obs.npy", ".ne_obs.npy", ".ne_obs.txt", ".ne_ind.txt")


@pytest.mark.parametrize("loo", [False, True])
def test_command_line(files, tmp_path, monkeypatch, loo):
    """--get_reference_af --ne_obs [--loo --partition_sites 3] as today and with WGSASSIGN_NE_WINDOW_SITES=8192: the same bytes in
    every output, the same stdout, the lines about windows on stderr; the two older variables alone send nothing to windows."""
    path, IDs, _ = files(20000)
    ids = str(tmp_path / "ids.txt")
    np.savetxt(ids, IDs, fmt="%s", delimiter="\t")
    argv = ["--beagle", path, "--pop_af_IDs", ids, "--get_reference_af", "--ne_obs", "--threads", "2"]
    names = NE_FILES
    if loo:
        argv += ["--loo", "--partition_sites", "3"]
        names += (".pop_like_LOO.tsv",)
    a, b, c = (str(tmp_path / x) for x in "abc")
    out1, err1 = run_cli(argv + ["--out", a])
    monkeypatch.setenv("WGSASSIGN_WINDOW_SITES", "8192")
    monkeypatch.setenv("WGSASSIGN_LOO_WINDOW_SITES", "8192")
    out3, err3 = run_cli(argv + ["--out", c])
    monkeypatch.delenv("WGSASSIGN_WINDOW_SITES")
    monkeypatch.delenv("WGSASSIGN_LOO_WINDOW_SITES")
    monkeypatch.setenv("WGSASSIGN_NE_WINDOW_SITES", "8192")
    out2, err2 = run_cli(argv + ["--out", b])
    for name in names:
        assert open(a + name, "rb").read() == open(b + name, "rb").read(), name
        assert open(a + name, "rb").read() == open(c + name, "rb").read(), name
    if loo:
        name = ".pop_like_LOO_partitions_3.tsv.gz"
        assert gzip.open(a + name, "rb").read() == gzip.open(b + name, "rb").read()
    assert out1.replace(a, "OUT") == out2.replace(b, "OUT")
    assert out1.replace(a, "OUT") == out3.replace(c, "OUT")
    assert "Estimating Fisher information." in out2 and out2.count("EM (MAF) converged at iteration") == K + (N if loo else 0)
    assert "window" not in err1 and "window" not in err3
    expected = ["wgsassign_amd: fitted in 2 rounds of 3 windows of 8192 sites", "wgsassign_amd: Fisher information in 3 windows of 8192 sites"]
    if loo:
        expected.append("wgsassign_amd: leave-one-out in 2 rounds of 3 windows of 8192 sites")
    assert [l for l in err2.splitlines() if "window" in l] == expected
