"""The EM fit in site windows (emMAF.emMAF_windowed, device.EMStream, wgs_em_stream_*): a Beagle file fitted in consecutive windows,
in rounds, gives the frequencies and iteration counts of its resident matrix BIT FOR BIT -- every comparison here is of bytes, no
tolerance.  The yardstick is the resident EMBatch.run on the matrix reader_cy.stream_to_device makes of the same file; it is held to
the oracle elsewhere."""
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


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """case(m, odd_first=False) -> (gzipped Beagle file, IDs); odd_first: the first 8192 sites are of another depth than the rest, so
    that the first window's own sums would stop it at iteration 9 where the file stops at 26 to 28."""
    root = tmp_path_factory.mktemp("windowed_fit")
    made = {}

    def case(m, odd_first=False):
        if (m, odd_first) not in made:
            L, IDs = synth.make_beagle(m, N, K, seed=4100 + N)
            if odd_first:
                L[:W1] = synth.make_beagle(W1, N, K, seed=77, depth=12.0)[0]
            path = str(root / ("m%d_%d.beagle.gz" % (m, odd_first)))
            with gzip.open(path, "wb", compresslevel=1) as fh:
                fh.write(beagle_text(L))
            made[(m, odd_first)] = (path, IDs)
        return made[(m, odd_first)]
    case.root = root
    return case


@pytest.fixture(autouse=True)
def _private_index_cache(files, monkeypatch):
    monkeypatch.setenv("WGSASSIGN_INDEX_DIR", str(files.root))
    monkeypatch.delenv("WGSASSIGN_WINDOW_SITES", raising=False)


_resident = {}


def resident_fit(path, IDs, maf_iter=200, tole=1e-4):
    """(af clamped, iters) of EMBatch.run over the resident matrix of the file: computed once per file and setting, never changed."""
    from wgsassign_amd import device, reader_cy
    key = (path, maf_iter, tole, device.EMBatch.GUARD, os.environ.get("WGSASSIGN_CODES"))
    if key not in _resident:
        pops = np.unique(IDs[:, 1])
        group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
        beagle, _, _, m = reader_cy.stream_to_device(path, group_of, len(pops), names="ends")
        em = device.EMBatch(beagle, np.arange(len(pops), dtype=np.int32))
        iters = em.run(maf_iter, tole)
        af = np.empty((m, len(pops)), dtype=np.float32)
        for k in range(len(pops)):
            em.clamp(k, int(np.sum(group_of == k)))
            af[:, k] = em.get_f(k)
        em.close()
        beagle.close()
        af.setflags(write=False)
        _resident[key] = (af, iters)
    return _resident[key]


def check(path, IDs, maf_iter=200, tole=1e-4, window=W1):
    from wgsassign_amd import emMAF
    af, iters = emMAF.emMAF_windowed(path, IDs, maf_iter, tole, window)
    af_r, iters_r = resident_fit(path, IDs, maf_iter, tole)
    print("iterations: windowed", list(iters), "resident", list(iters_r), "stats", {k: v for k, v in emMAF.emMAF_windowed.stats.items() if k != "round_seconds"})
    assert list(iters) == list(iters_r)
    assert af.dtype == np.float32 and af.shape == af_r.shape and af.tobytes() == af_r.tobytes()
    return emMAF.emMAF_windowed.stats, iters_r


@pytest.mark.parametrize("m, windows", [(20000, 3), (16384, 2), (5000, 1)])
def test_window_edges_default_band(files, m, windows):
    """A short last window after two full ones, an exact multiple, one short window.  The sums decide: two rounds."""
    from wgsassign_amd import windows as wplan
    path, IDs = files(m)
    stats, iters = check(path, IDs)
    assert stats["windows"] == windows and stats["window_sites"] == W1 and stats["rounds"] == 2 and stats["chain_iterations"] == 0
    assert stats["matrices"] == min(2, windows) and stats["seconds"] > 0 and len(stats["round_seconds"]) == 2
    counts = np.unique(IDs[:, 1], return_counts=True)[1]
    assert 0 < stats["largest_matrix_bytes"] <= W1 * wplan.fit_site_bytes(N, K, counts)
    assert stats["iterations_round1"] == 200 * K and stats["iterations_needed"] == int(sum(iters))
    if m == 20000:
        assert len(set(int(i) for i in iters)) > 1          # the populations stop at different iterations


def test_bgzf_and_a_memmap(files, tmp_path):
    from wgsassign_amd import emMAF
    src, IDs = files(20000)
    path = str(tmp_path / "copy.beagle.gz")
    synth.write_bgzf(path, gzip.open(src, "rb").read(), block=50000)
    check(path, IDs)
    out = str(tmp_path / "af.npy")
    af, iters = emMAF.emMAF_windowed(path, IDs, 200, 1e-4, W1, out=out)
    assert isinstance(af, np.memmap)
    del af
    af_r, iters_r = resident_fit(src, IDs)
    assert np.load(out).tobytes() == af_r.tobytes() and list(iters) == list(iters_r)
    np.save(str(tmp_path / "saved.npy"), af_r)
    assert open(out, "rb").read() == open(str(tmp_path / "saved.npy"), "rb").read()      # the file np.save writes, header and all


def test_every_decision_through_the_chain(files, monkeypatch):
    """GUARD = 1e9: the chains decide everything, relayed over a short last window; eight candidate iterations per round."""
    from wgsassign_amd import device
    monkeypatch.setattr(device.EMBatch, "GUARD", 1e9)
    path, IDs = files(20000)
    stats, iters = check(path, IDs)
    assert stats["rounds"] == 1 + -(-int(max(iters)) // 8) + 1 and stats["chain_iterations"] >= int(sum(iters))
    path, IDs = files(5000)
    check(path, IDs)


def test_exhausted(files, monkeypatch):
    from wgsassign_amd import device
    path, IDs = files(20000)
    stats, iters = check(path, IDs, maf_iter=3)
    assert list(iters) == [0] * K and stats["rounds"] == 2
    check(path, IDs, maf_iter=200, tole=0.0)
    monkeypatch.setattr(device.EMBatch, "GUARD", 1e9)
    check(path, IDs, maf_iter=3)


@pytest.mark.parametrize("codes", [True, False])
def test_codes_on_and_off(files, monkeypatch, codes):
    """The windows swept through the class codes and over the float32 slabs (four individuals per population are coded only with the
    encoder's table fixed and the smallest coded population lowered).  What the sweeps took is read off the batches."""
    from wgsassign_amd import device
    if codes:
        monkeypatch.setenv("WGSASSIGN_CODES_TABLE", "64")
        monkeypatch.setenv("WGSASSIGN_EM_CODES_MIN", "2")
    else:
        monkeypatch.setenv("WGSASSIGN_CODES", "0")
    paths = []
    push = device.EMStream.push

    def recording(self, em, *a, **kw):
        push(self, em, *a, **kw)
        paths.append(em.sweep_paths())
    monkeypatch.setattr(device.EMStream, "push", recording)
    path, IDs = files(20000)
    check(path, IDs)
    assert len(paths) == 6
    direct, coded = sum(p[0] for p in paths[-2:]), sum(p[2] for p in paths[-2:])
    print("sweeps over the float32 slabs", direct, "through the codes", coded)
    if codes:
        assert coded > 0
    else:
        assert coded == 0 and direct > 0


def test_a_first_window_unlike_the_rest(files, monkeypatch):
    """The first window's own sums would stop it at iteration 9, the rest at 28 to 30, the file at 26 to 28: a decision taken per
    window, or a tail of the cut last window reaching S, C or the output, shows here."""
    from wgsassign_amd import device
    path, IDs = files(20000, odd_first=True)
    stats, iters = check(path, IDs)
    assert len(set(int(i) for i in iters)) > 1
    monkeypatch.setattr(device.EMBatch, "GUARD", 1e9)
    check(path, IDs)


def test_push_refusals_launch_nothing():
    from wgsassign_amd import device
    group_of = np.repeat(np.arange(K, dtype=np.int32), N // K)
    b = device.DeviceBeagle(W1, N, group_of, K, site0=W1)
    b.synth(11, 2.0)
    em = b.window_em = device.EMBatch(b, np.arange(K, dtype=np.int32))
    run = np.full(K, 5, dtype=np.int32)
    st = device.EMStream(K, 10, W1 + 100)
    with pytest.raises(ValueError, match="starts at site 8192, but 0 sites were pushed so far"):
        st.push(em, run, add_sums=True)
    b.set_window(100)            # (the batch stays: wgs_em_stream_move_window)
    with pytest.raises(ValueError, match="starts at site 100, which is not a multiple of 8192"):
        st.push(em, run, add_sums=True)
    with pytest.raises(ValueError, match="only 0 of the 8292 sites were pushed"):
        st.read()
    b.set_window(0)
    two = device.EMBatch(b, np.arange(2, dtype=np.int32))
    with pytest.raises(ValueError, match="the window's batch has 2 fits, the fit stream 3"):
        st.push(two, run, add_sums=True)
    with pytest.raises(ValueError, match="in use"):          # a second batch on the matrix: it cannot be moved any more
        b.set_window(W1)
    two.close()
    with pytest.raises(ValueError, match="fit 1: 11 iterations, the fit stream has 10"):
        st.push(em, [5, 11, 5])
    with pytest.raises(ValueError, match="chain 0: iteration 6 of fit 0, which runs 5"):
        st.push(em, run, chains=[(0, 6)])
    with pytest.raises(ValueError, match="not sorted by iteration"):
        st.push(em, run, chains=[(0, 3), (1, 2)])
    with pytest.raises(ValueError, match="final fits need their clamps"):
        st.push(em, run, final=[1, 0, 0])
    small = device.EMStream(K, 10, 5000)
    with pytest.raises(ValueError, match="8192 sites after 0 pushed exceed the 5000 sites"):
        small.push(em, run, add_sums=True)
    small.close()
    assert em.sweep_paths() == [0, 0, 0, 0] and st.windows == 0 and b.codes_state() == 0       # nothing was swept
    st.push(em, run, add_sums=True)
    assert sum(em.sweep_paths()) == 5 and st.windows == 1
    short = device.DeviceBeagle(100, N, group_of, K, site0=W1)
    short.synth(12, 2.0)
    em100 = device.EMBatch(short, np.arange(K, dtype=np.int32))
    long = device.EMStream(K, 10, 3 * W1)
    long.push(em, run, add_sums=True)
    with pytest.raises(ValueError, match="a window of 100 sites that is not the last one"):
        long.push(em100, run, add_sums=True)
    assert em100.sweep_paths() == [0, 0, 0, 0]
    long.close()
    # the stream is still usable: the short window ends the round, whose sums are those of both windows and of nothing else
    st.push(em100, run, add_sums=True)
    S, C = st.read()
    assert S.shape == (10, K) and (S[:5] > 0).all() and (S[5:] == 0).all() and (C == 0).all()
    st.close()
    st.close()
    for obj in (em100, short, em, b):
        obj.close()


def run_cli(argv):
    from wgsassign_amd import WGSassign
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        WGSassign.main(argv)
    return out.getvalue(), err.getvalue()


def test_command_line(files, tmp_path, monkeypatch):
    """--get_reference_af as today and with WGSASSIGN_WINDOW_SITES=8192: the same bytes in .pop_af.npy and .pop_names.txt, the same
    stdout, one more line on stderr; with --loo beside it the resident path runs and says nothing of windows."""
    path, IDs = files(20000)
    ids = str(tmp_path / "ids.txt")
    np.savetxt(ids, IDs, fmt="%s", delimiter="\t")
    argv = ["--beagle", path, "--pop_af_IDs", ids, "--get_reference_af", "--threads", "2"]
    out1, err1 = run_cli(argv + ["--out", str(tmp_path / "a")])
    monkeypatch.setenv("WGSASSIGN_WINDOW_SITES", "8192")
    out2, err2 = run_cli(argv + ["--out", str(tmp_path / "b")])
    for name in (".pop_af.npy", ".pop_names.txt"):
        assert open(str(tmp_path / "a") + name, "rb").read() == open(str(tmp_path / "b") + name, "rb").read(), name
    assert out1.replace(str(tmp_path / "a"), "OUT") == out2.replace(str(tmp_path / "b"), "OUT")
    assert "EM (MAF) converged at iteration" in out2
    assert "window" not in err1
    assert [l for l in err2.splitlines() if "window" in l] == ["wgsassign_amd: fitted in 2 rounds of 3 windows of 8192 sites"]
    out3, err3 = run_cli(argv + ["--loo", "--out", str(tmp_path / "c")])
    assert "window" not in err3 and os.path.exists(str(tmp_path / "c.pop_like_LOO.tsv"))
