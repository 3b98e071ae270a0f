"""The leave-one-out run in site windows (glassy.loo_windowed, device.LooStream, wgs_loo_stream_*, wgs_em_stream_push_keep): a Beagle
file taken in consecutive windows, in rounds, gives the log-likelihoods, partition sums and iteration counts of its resident matrix
BIT FOR BIT -- every comparison here is of bytes, no tolerance.  The yardstick is glassy.loo_device on the matrix
reader_cy.stream_to_device makes of the same file, with the frequencies of the resident fit; it is held to the oracle elsewhere."""
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
# The first horizons of test_window_edges: glassy.LOO_MARGIN is measured on populations of 36 to 62 individuals, where leaving one out
# moves the stopping iteration by 0 or 1.  Here a population has FOUR, a re-fit loses a quarter of its data, and the oracle's re-fits on
# these very matrices stop up to 2 iterations after their population's fit (m = 5000: 26, 26, 28 against 27 to 28).  The window-edge
# cases are about the windows, so they take a margin that covers that; every other test runs with the margin in use.
EDGE_MARGIN = 4
UNEQUAL = [2, 1, 2, 0, 2, 1, 2, 1, 0, 2, 1, 2]           # populations of 2, 4 and 6: a re-fit from one individual, three clamps


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """case(m, odd_first=False, unequal=False) -> (gzipped Beagle file, IDs): populations interleaved in file order, so the sticky
    columns matter; odd_first: the first 8192 sites are of another depth than the rest; unequal: populations of 2, 4 and 6."""
    root = tmp_path_factory.mktemp("windowed_loo")
    made = {}

    def case(m, odd_first=False, unequal=False):
        key = (m, odd_first, unequal)
        if key not in made:
            if unequal:
                L, IDs = synth.make_beagle_for_labels(m, UNEQUAL, K, seed=4100 + N)
            else:
                L, IDs = synth.make_beagle(m, N, K, seed=4100 + N, interleave=True)
            if odd_first:
                L[:W1] = synth.make_beagle(W1, N, K, seed=77, depth=12.0, interleave=True)[0]
            path = str(root / ("m%d_%d_%d.beagle.gz" % (m, odd_first, unequal)))
            with gzip.open(path, "wb", compresslevel=1) as fh:
                fh.write(beagle_text(L))
            made[key] = (path, IDs)
        return made[key]
    case.root = root
    return case


@pytest.fixture(autouse=True)
def _private_index_cache(files, monkeypatch):
    monkeypatch.setenv("WGSASSIGN_INDEX_DIR", str(files.root))
    monkeypatch.delenv("WGSASSIGN_WINDOW_SITES", raising=False)
    monkeypatch.delenv("WGSASSIGN_LOO_WINDOW_SITES", raising=False)


_resident = {}


def resident_loo(path, IDs, P, maf_iter=200, tole=1e-4):
    """(af clamped, population iters, logl, parts, iters) of the resident fit and glassy.loo_device over the resident matrix of the
    file: computed once per file and setting, never changed."""
    from wgsassign_amd import device, glassy, reader_cy
    key = (path, P, maf_iter, tole, os.environ.get("WGSASSIGN_CODES"), os.environ.get("WGSASSIGN_CODES_TABLE"))
    if key not in _resident:
        pops = np.unique(IDs[:, 1])
        group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
        beagle, _, _, m = reader_cy.stream_to_device(path, group_of, len(pops), names="ends")
        em = device.EMBatch(beagle, np.arange(len(pops), dtype=np.int32))
        pop_iters = em.run(maf_iter, tole)
        af = np.empty((m, len(pops)), dtype=np.float32)
        for k in range(len(pops)):
            em.clamp(k, int(np.sum(group_of == k)))
            af[:, k] = em.get_f(k)
        em.close()
        tm = {}
        logl, parts = glassy.loo_device(beagle, beagle, af.copy(), group_of, maf_iter, tole, P, verbose=False, timings=tm)
        beagle.close()
        for a in (af, logl, parts):
            a.setflags(write=False)
        _resident[key] = (af, pop_iters, logl, parts, np.asarray(tm["iters"]).copy())
    return _resident[key]


def check(path, IDs, P=3, maf_iter=200, tole=1e-4, window=W1, first_iters="pop"):
    from wgsassign_amd import glassy
    af, pop_iters, logl_r, parts_r, iters_r = resident_loo(path, IDs, P, maf_iter, tole)
    if isinstance(first_iters, int):
        group_of = np.searchsorted(np.unique(IDs[:, 1]), IDs[:, 1])
        first_iters = glassy.loo_first_iters(group_of, pop_iters, maf_iter, margin=first_iters)
    kw = {"pop_iters": pop_iters} if isinstance(first_iters, str) else {"first_iters": first_iters}
    before = af.tobytes()
    logl, parts, iters = glassy.loo_windowed(path, af, IDs, maf_iter, tole, window, P, **kw)
    stats = glassy.loo_windowed.stats
    print("iterations: populations", list(pop_iters), "windowed", list(iters), "resident", list(iters_r),
          "stats", {k: v for k, v in stats.items() if k != "round_seconds"})
    assert list(iters) == list(iters_r)
    assert logl.dtype == np.float32 and logl.shape == (N, K) and logl.tobytes() == logl_r.tobytes()
    assert parts.dtype == np.float32 and parts.shape == (N * P, K) and parts.tobytes() == parts_r.tobytes()
    assert af.tobytes() == before                           # unlike loo(), the frequencies are left as they were
    assert stats["refit_bytes_to_host"] == 0
    return stats, iters_r


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("m, windows", [(20000, 3), (16384, 2), (5000, 1)])
def test_window_edges(files, monkeypatch, m, windows, P):
    """A short last window after two full ones, an exact multiple, one short window; with and without partitions.  The sums decide
    inside the first horizons: two rounds.  No re-fit frequencies reach the host: the fit stream's copying push is never called."""
    from wgsassign_amd import device
    from wgsassign_amd import windows as wplan

    def never(self, *a, **kw):
        raise AssertionError("EMStream.push copies final fits to the host")
    monkeypatch.setattr(device.EMStream, "push", never)
    path, IDs = files(m)
    stats, iters = check(path, IDs, P, first_iters=EDGE_MARGIN)
    assert stats["windows"] == windows and stats["window_sites"] == W1
    assert stats["rounds"] == 2 and stats["chain_iterations"] == 0 and stats["extension_rounds"] == 0
    assert stats["matrices"] == min(2, windows) and stats["seconds"] > 0 and len(stats["round_seconds"]) == 2
    counts = np.unique(IDs[:, 1], return_counts=True)[1]
    assert 0 < stats["largest_matrix_bytes"] <= W1 * wplan.loo_site_bytes(N, K, counts, P)
    assert stats["iterations_round1"] < 200 * N and stats["iterations_needed"] == int(sum(iters))
    assert all(i > 0 for i in iters)


def test_unequal_populations(files):
    """Populations of 2, 4 and 6: a re-fit from one individual, and three different clamps."""
    path, IDs = files(20000, unequal=True)
    assert sorted(np.unique(IDs[:, 1], return_counts=True)[1]) == [2, 4, 6]
    stats, iters = check(path, IDs)
    assert len(set(int(i) for i in iters)) > 1
    check(path, IDs, P=1)


def test_every_decision_through_the_chain(files, monkeypatch):
    from wgsassign_amd import device
    monkeypatch.setattr(device.EMBatch, "GUARD", 1e9)
    path, IDs = files(20000)
    stats, iters = check(path, IDs)
    assert stats["chain_iterations"] >= int(sum(iters)) and stats["rounds"] > 3
    path, IDs = files(5000)
    check(path, IDs, first_iters=None)


def test_exhausted(files):
    path, IDs = files(20000)
    stats, iters = check(path, IDs, maf_iter=3)
    assert list(iters) == [0] * N and stats["rounds"] == 2
    stats, iters = check(path, IDs, maf_iter=200, tole=0.0, first_iters=[50] * N)
    assert list(iters) == [0] * N and stats["extension_rounds"] == 2           # horizons 50, 100, 200


def test_horizons_of_one_force_extension_rounds(files):
    path, IDs = files(20000)
    stats, iters = check(path, IDs, first_iters=[1] * N)
    assert stats["extension_rounds"] == int(np.ceil(np.log2(max(iters)))) and stats["iterations_round1"] == N
    assert stats["rounds"] == 2 + stats["extension_rounds"]
    stats, _ = check(path, IDs, P=1, first_iters=None)
    assert stats["iterations_round1"] == 200 * N and stats["rounds"] == 2


@pytest.mark.parametrize("codes", [True, False])
def test_codes_on_and_off(files, monkeypatch, codes):
    """The windows' re-fits swept through the class codes and over the float32 slabs.  What the sweeps took is read off the batches."""
    from wgsassign_amd import device
    if codes:
        monkeypatch.setenv("WGSASSIGN_CODES_TABLE", "64")
        monkeypatch.setenv("WGSASSIGN_EM_CODES_MIN", "2")
    else:
        monkeypatch.setenv("WGSASSIGN_CODES", "0")
    paths = []
    push = device.EMStream.push_keep

    def recording(self, em, *a, **kw):
        push(self, em, *a, **kw)
        paths.append(em.sweep_paths())
    monkeypatch.setattr(device.EMStream, "push_keep", recording)
    path, IDs = files(20000)
    check(path, IDs)
    assert len(paths) == 6
    direct, coded = sum(p[0] + p[1] for p in paths[-2:]), sum(p[2] + p[3] for p in paths[-2:])
    print("sweeps over the float32 slabs", direct, "through the codes", coded)
    if codes:
        assert coded > 0
    else:
        assert coded == 0 and direct > 0


def test_a_first_window_unlike_the_rest(files):
    path, IDs = files(20000, odd_first=True)
    check(path, IDs)
    check(path, IDs, P=1, first_iters=[1] * N)


def test_bgzf(files, tmp_path):
    src, IDs = files(20000)
    path = str(tmp_path / "copy.beagle.gz")
    synth.write_bgzf(path, gzip.open(src, "rb").read(), block=50000)
    check(path, IDs)


def test_more_partitions_than_the_block_parallel_chains_take(files):
    from wgsassign_amd import device
    path, IDs = files(20000)
    check(path, IDs, P=device.MAX_BLOCK_PARALLEL_PARTS + 1)


def test_push_refusals_launch_nothing():
    from wgsassign_amd import device, glassy
    P = 3
    group_of = np.asarray([i % K for i in range(N)], dtype=np.int32)
    skips = np.arange(N, dtype=np.int32)
    b = device.DeviceBeagle(W1, N, group_of, K, site0=W1)
    b.synth(11, 2.0)
    em = b.window_em = device.EMBatch(b, group_of, skips)
    rng = np.random.default_rng(5)
    A = rng.uniform(0.05, 0.95, size=(W1, K)).astype(np.float32)
    afs = device.AFSet.from_host(A)
    st = device.LooStream(N, K, W1 + 100, P)
    with pytest.raises(ValueError, match="starts at site 8192, but 0 sites were pushed so far"):
        st.push(em, afs)
    b.set_window(100)
    with pytest.raises(ValueError, match="starts at site 100, which is not a multiple of 8192"):
        st.push(em, afs)
    with pytest.raises(ValueError, match="only 0 of the 8292 sites were pushed"):
        st.finish()
    b.set_window(0)
    pops_only = device.EMBatch(b, np.arange(K, dtype=np.int32))
    with pytest.raises(ValueError, match="the window's batch has 3 fits, the leave-one-out stream 12 individuals"):
        st.push(pops_only, afs)
    pops_only.close()
    whole = device.EMBatch(b, group_of)
    with pytest.raises(ValueError, match="fit 0 leaves nobody out"):
        st.push(whole, afs)
    whole.close()
    wrong_k = device.AFSet.from_host(np.ascontiguousarray(A[:, :2]))
    with pytest.raises(ValueError, match="12 individuals x 2 populations, the leave-one-out stream 12 x 3"):
        st.push(em, wrong_k)
    wrong_k.close()
    short_af = device.AFSet.from_host(np.ascontiguousarray(A[:100]))
    with pytest.raises(ValueError, match="allele frequencies cover 100 SNPs, the window 8192"):
        st.push(em, short_af)
    other_n = device.LooStream(N + 1, K, W1, P)
    with pytest.raises(ValueError, match="12 individuals x 3 populations, the leave-one-out stream 13 x 3"):
        other_n.push(em, afs)
    other_n.close()
    small = device.LooStream(N, K, 5000, P)
    with pytest.raises(ValueError, match="8192 sites after 0 pushed exceed the 5000 sites"):
        small.push(em, afs)
    small.close()
    fits = device.EMStream(N, 10, W1 + 100)
    with pytest.raises(ValueError, match="fit 1: sums above iteration 6, but it runs 5"):
        fits.push_keep(em, [5] * N, sums_from=[0, 6] + [0] * (N - 2))
    assert em.sweep_paths() == [0, 0, 0, 0] and st.windows == 0 and fits.windows == 0 and b.codes_state() == 0     # nothing was swept
    # the streams are still usable: two windows fitted, kept on the device and scored, against the step-wise resident scoring
    lo = np.float32(1 / (2 * (np.bincount(group_of)[group_of] - 1 + 1)))
    run = np.full(N, 5, dtype=np.int32)
    fits.push_keep(em, run, np.ones(N, dtype=np.int32), lo, np.float32(1) - lo, sums_from=np.zeros(N, dtype=np.int32))
    assert sum(em.sweep_paths()) == 5
    want, want_parts = glassy.score_loo_batch(b, afs, em, group_of, 0, N, P)
    st.push(em, afs)
    short = device.DeviceBeagle(100, N, group_of, K, site0=W1)
    short.synth(12, 2.0)
    em100 = device.EMBatch(short, group_of, skips)
    long = device.LooStream(N, K, 3 * W1, P)
    long.push(em, afs)
    with pytest.raises(ValueError, match="a window of 100 sites that is not the last one"):
        long.push(em100, short_af)
    long.close()
    fits.push_keep(em100, run, np.ones(N, dtype=np.int32), lo, np.float32(1) - lo, sums_from=np.zeros(N, dtype=np.int32))
    S, C = fits.read()
    assert (S[:5] > 0).all() and (S[5:] == 0).all() and (C == 0).all()
    tail, tail_parts = glassy.score_loo_batch(short, short_af, em100, group_of, 0, N, 1)
    st.push(em100, short_af)
    out, parts = st.finish()
    assert parts.shape == (N * P, K) and out.shape == (N, K)
    # one 8192-site chunk and a short one: the total is their float64 sum in this order
    assert out.tobytes() == (want + tail).tobytes() and np.isfinite(out).all() and (out < 0).all()
    assert want_parts.dtype == np.float32 and not (parts == want_parts).all()           # the second window went on from the first
    st.close()
    st.close()
    for obj in (fits, short_af, afs, em100, short, em, b):
        obj.close()


def run_cli(argv):
    from wgsassign_amd import WGSassign
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        WGSassign.main(argv)
    return out.getvalue(), err.getvalue()


def test_command_line(files, tmp_path, monkeypatch):
    """--get_reference_af --loo --partition_sites 3 as today and with WGSASSIGN_LOO_WINDOW_SITES=8192: the same bytes in the four
    outputs, the same stdout, two more lines on stderr; with --ne_obs beside them the resident path runs and says nothing of
    windows."""
    path, IDs = files(20000)
    ids = str(tmp_path / "ids.txt")
    np.savetxt(ids, IDs, fmt="%s", delimiter="\t")
    argv = ["--beagle", path, "--pop_af_IDs", ids, "--get_reference_af", "--loo", "--partition_sites", "3", "--threads", "2"]
    out1, err1 = run_cli(argv + ["--out", str(tmp_path / "a")])
    monkeypatch.setenv("WGSASSIGN_LOO_WINDOW_SITES", "8192")
    out2, err2 = run_cli(argv + ["--out", str(tmp_path / "b")])
    for name in (".pop_af.npy", ".pop_names.txt", ".pop_like_LOO.tsv"):
        assert open(str(tmp_path / "a") + name, "rb").read() == open(str(tmp_path / "b") + name, "rb").read(), name
    name = ".pop_like_LOO_partitions_3.tsv.gz"
    assert gzip.open(str(tmp_path / "a") + name, "rb").read() == gzip.open(str(tmp_path / "b") + name, "rb").read()
    assert out1.replace(str(tmp_path / "a"), "OUT") == out2.replace(str(tmp_path / "b"), "OUT")
    assert out2.count("EM (MAF) converged at iteration") == K + N
    assert "window" not in err1
    assert [l for l in err2.splitlines() if "window" in l] == ["wgsassign_amd: fitted in 2 rounds of 3 windows of 8192 sites",
                                                               "wgsassign_amd: leave-one-out in 2 rounds of 3 windows of 8192 sites"]
    out3, err3 = run_cli(argv + ["--ne_obs", "--out", str(tmp_path / "c")])
    assert "window" not in err3 and os.path.exists(str(tmp_path / "c.pop_like_LOO.tsv"))
    assert open(str(tmp_path / "a.pop_like_LOO.tsv"), "rb").read() == open(str(tmp_path / "c.pop_like_LOO.tsv"), "rb").read()
