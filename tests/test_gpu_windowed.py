"""Windowed scoring (glassy.assignLL_windowed, device.ScoreStream, reader_cy.stream_windows, wgs_score_stream_*): a Beagle file scored
in consecutive site windows gives the float64 totals of its resident matrix BIT FOR BIT -- every comparison here is np.array_equal,
no tolerance.  The resident path (device.assign on the matrix reader_cy.stream_to_device makes of the same file) is the yardstick;
it is held to the oracle elsewhere, and once more here."""
import contextlib
import ctypes
import gzip
import io
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
W1 = 8192


def beagle_text(L):
    """The matrix as Beagle text (d.dddddd, three likelihoods per individual): digits formed by whole-array integer arithmetic, a
    Python loop over the lines only."""
    m, n = L.shape[0], L.shape[1] // 2
    a = np.rint(L[:, 0::2].astype(np.float64) * 1e6).astype(np.int64)
    b = np.rint(L[:, 1::2].astype(np.float64) * 1e6).astype(np.int64)
    v = np.stack([a, b, np.maximum(0, 1_000_000 - a - b)], axis=2).reshape(m, 3 * n)
    txt = np.empty((m, 3 * n, 9), dtype=np.uint8)
    txt[:, :, 0] = 9
    txt[:, :, 1] = 48 + v // 1_000_000
    txt[:, :, 2] = 46
    r = v % 1_000_000
    for k in range(6):
        txt[:, :, 3 + k] = 48 + (r // 10 ** (5 - k)) % 10
    rows = txt.reshape(m, 27 * n)
    head = "marker\tallele1\tallele2" + "".join("\tInd%d\tInd%d\tInd%d" % (i, i, i) for i in range(n)) + "\n"
    return head.encode() + b"".join(b"chr1_%d\tA\tC" % (s + 1) + rows[s].tobytes() + b"\n" for s in range(m))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """case(m, n, K) -> (path of the gzipped Beagle file, A (m, K) float32); every file is written once per module."""
    root = tmp_path_factory.mktemp("windowed")
    made = {}

    def case(m, n, K):
        if (m, n, K) not in made:
            L, _ = synth.make_beagle(m, n, K, seed=4100 + n)
            path = str(root / ("m%d_n%d.beagle.gz" % (m, n)))
            with gzip.open(path, "wb", compresslevel=1) as fh:
                fh.write(beagle_text(L))
            A = np.random.default_rng(m + K).uniform(0.02, 0.98, size=(m, K)).astype(np.float32)
            made[(m, n, K)] = (path, A)
        return made[(m, n, K)]
    case.root = root
    return case


@pytest.fixture(autouse=True)
def _private_index_cache(files, monkeypatch):
    monkeypatch.setenv("WGSASSIGN_INDEX_DIR", str(files.root))
    monkeypatch.delenv("WGSASSIGN_WINDOW_SITES", raising=False)


_resident = {}


def resident_totals(path, A):
    """device.assign over the resident matrix of the file: computed once per file (and per setting of the class codes), never changed."""
    from wgsassign_amd import device, reader_cy
    key = (path, os.environ.get("WGSASSIGN_SCORE_CODES_ALWAYS"), os.environ.get("WGSASSIGN_CODES_TABLE"))
    if key not in _resident:
        beagle, _, _, m = reader_cy.stream_to_device(path, names="ends")
        afs = device.AFSet.from_host(A)
        out, _ = device.assign(beagle, afs)
        afs.close()
        beagle.close()
        out.setflags(write=False)
        _resident[key] = out
    return _resident[key]


@pytest.mark.parametrize("m, windows", [(5000, 1), (8192, 1), (12000, 2), (16384, 2), (25810, 4)])
def test_window_edges(files, oracle, m, windows):
    """One short window, exactly one, one and a short second (the second matrix is then made short), exactly two, three and a rest
    that is no multiple of 64."""
    from wgsassign_amd import glassy, reader_cy
    path, A = files(m, 7, 3)
    out = glassy.assignLL_windowed(path, A, W1)
    st = glassy.assignLL_windowed.stats
    assert out.dtype == np.float64 and out.shape == (7, 3)
    assert st["windows"] == windows and st["window_sites"] == W1 and len(st["sweep_ms"]) == windows
    assert np.array_equal(out, resident_totals(path, A))
    if m == 25810:
        L, _, _ = reader_cy.readBeagle(path)
        ll_o = oracle.assignLL(np.ascontiguousarray(L), A.copy(), 2)
        ll = out.astype(np.float32)
        assert ll.dtype == ll_o.dtype and ll.tobytes() == ll_o.tobytes()
        # the frequencies as a memory-mapped file, as the command line hands them over
        np.save(os.path.join(os.path.dirname(path), "A25810.npy"), A)
        view = np.load(os.path.join(os.path.dirname(path), "A25810.npy"), mmap_mode="r")
        assert np.array_equal(glassy.assignLL_windowed(path, view, W1), out)


def test_the_carry_does_work(files, oracle, tmp_path):
    """Five windows of 8192 sites and three of 16384: a window that restarted NumPy's running total instead of continuing it would
    differ from the resident totals in the last bits -- on the order case, that is, which comes first here.  The generated matrix
    behind it cannot show the order: every partial float64 sum of its cells is exact (window total plus window total, math.fsum and
    np.sum agree in all 350 cells), so what it holds is that the windows lose and repeat nothing.  The case of tests/order_cases.py
    (7 blocks, the last one ragged: a window of 16384 sites and a short one of two chunks) is built so that its block sums are exact
    and its totals are not: there the restarting twin differs from np.sum in at least eight cells, and the windows must not."""
    import order_cases as oc
    from wgsassign_amd import glassy
    shape = (7, "ragged")
    vals = oc.reference(oracle, shape)
    want, S = oc.expected(vals), oc.block_sums(vals)
    assert oc.different_cells(oc.restart_order(S, 16384), want) >= oc.MIN_DIFFERENT
    assert oc.different_cells(oc.restart_order(S, 8192), want) == 0                  # (total + chunk either way: 8192 can never show)
    L, A_order = oc.matrix_of(shape)
    order_path = str(tmp_path / "order.beagle.gz")
    with gzip.open(order_path, "wb", compresslevel=1) as fh:
        fh.write(oc.beagle_text(L))
    got = glassy.assignLL_windowed(order_path, np.ascontiguousarray(A_order), 16384)
    assert glassy.assignLL_windowed.stats["windows"] == 2
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    path, A = files(40000, 70, 5)
    a = glassy.assignLL_windowed(path, A, 8192)
    assert glassy.assignLL_windowed.stats["windows"] == 5
    b = glassy.assignLL_windowed(path, A, 16384)
    assert glassy.assignLL_windowed.stats["windows"] == 3
    res = resident_totals(path, A)
    assert np.array_equal(a, res) and np.array_equal(b, res) and np.array_equal(a, b)
    # (what a restart would give is not what is asserted above by accident: the plain sum of per-window totals differs)
    from wgsassign_amd import device, reader_cy
    parts = []
    for beagle in reader_cy.stream_windows(path, 8192):
        afs = device.AFSet.from_host(np.ascontiguousarray(A[beagle.site0:beagle.site0 + beagle.m]))
        parts.append(device.assign(beagle, afs)[0])
        afs.close()
    assert len(parts) == 5 and np.allclose(sum(parts), res, rtol=1e-12, atol=0)


@pytest.mark.parametrize("forced", [True, False])
def test_both_modes(files, monkeypatch, forced):
    """Windows swept through the class codes and over the float32 slabs.  The suite's setting makes the cost model say yes, but the
    sample pass still finds seven individuals not worth coding (hardly fewer classes than individuals: csrc/codes.hip,
    wgs_beagle_codes_plan), so the coded case also fixes the encoder's table (WGSASSIGN_CODES_TABLE, the switch that overrides that
    finding); left to itself the library builds no codes for 8192 sites x 7.  What each window's sweep took is read off the matrix."""
    from wgsassign_amd import device, glassy
    if forced:
        monkeypatch.setenv("WGSASSIGN_CODES_TABLE", "64")
    else:
        monkeypatch.delenv("WGSASSIGN_SCORE_CODES_ALWAYS")
    states = []
    push = device.ScoreStream.push

    def recording(self, beagle, afset, mode=None):
        push(self, beagle, afset, mode)
        states.append(beagle.codes_state())
    monkeypatch.setattr(device.ScoreStream, "push", recording)
    path, A = files(25810, 7, 3)
    out = glassy.assignLL_windowed(path, A, W1)
    assert len(states) == 4 and all((s == 1) == forced for s in states), states
    assert np.array_equal(out, resident_totals(path, A))


def test_c_abi_misuse_is_refused_without_a_launch(files, monkeypatch):
    from wgsassign_amd import _lib, device, glassy, windows
    monkeypatch.setenv("WGSASSIGN_CODES_TABLE", "64")         # (seven individuals are coded only with the table fixed: test_both_modes)
    n, K = 7, 3
    b = device.DeviceBeagle(8192, n, site0=8192)
    b.synth(11, 2.0)
    afs = device.AFSet.from_host(np.full((8192, K), 0.25, dtype=np.float32))
    st = device.ScoreStream(n, K, 16384)
    with pytest.raises(ValueError, match="starts at site 8192, but 0 sites were pushed so far"):
        st.push(b, afs)
    b.set_window(100)
    with pytest.raises(ValueError, match="starts at site 100, which is not a multiple of 8192"):
        st.push(b, afs)
    with pytest.raises(ValueError, match="only 0 of the 16384 sites were pushed"):
        st.finish()
    assert b.codes_state() == 0 and st.windows == 0          # nothing was swept: a sweep would have built the class codes (the suite forces them)
    b.set_window(0)
    st.push(b, afs)
    assert b.codes_state() == 1
    with pytest.raises(ValueError, match="only 8192 of the 16384 sites were pushed"):
        st.finish()
    short = device.DeviceBeagle(100, n, site0=8192)
    short.synth(12, 2.0)
    with pytest.raises(ValueError, match="allele frequencies cover 8192 SNPs, the window 100"):
        st.push(short, afs)
    afs100 = device.AFSet.from_host(np.full((100, K), 0.25, dtype=np.float32))
    with pytest.raises(ValueError, match="a window of 100 sites that is not the last one"):      # 8192 + 100 < 16384
        st.push(short, afs100)
    small = device.ScoreStream(n, K, 5000)
    with pytest.raises(ValueError, match="8192 sites after 0 pushed exceed the 5000 sites"):
        small.push(b, afs)
    assert short.codes_state() == 0 and small.windows == 0 and st.windows == 1
    small.close()
    afs100.close()
    # the stream is still destroyable, and destroying it twice is a no-op -- through the wrapper and at the C ABI itself
    h = ctypes.c_void_p(st.handle.value)
    st.close()
    st.close()
    _lib.load().wgs_score_stream_destroy(h)
    st2 = device.ScoreStream(n, K, 8192)
    h2 = ctypes.c_void_p(st2.handle.value)
    _lib.load().wgs_score_stream_destroy(h2)
    _lib.load().wgs_score_stream_destroy(h2)
    st2._h = None
    for obj in (short, afs, b):
        obj.close()
    path, A = files(5000, n, K)
    monkeypatch.setenv(windows.ENV, "100")
    with pytest.raises(ValueError, match="WGSASSIGN_WINDOW_SITES=100 is below 8192"):
        glassy.assignLL_windowed(path, A)
    with pytest.raises(ValueError, match="at least 8192 sites"):
        glassy.assignLL_windowed(path, A, 100)


def test_memory_really_is_bounded(files, monkeypatch):
    from wgsassign_amd import device, glassy
    n, K = 7, 3
    path, A = files(25810, n, K)
    probe = device.DeviceBeagle(8192, n)
    one_window = probe.nbytes()
    probe.close()
    made, alive, most = [], set(), [0]
    init, close = device.DeviceBeagle.__init__, device.DeviceBeagle.close

    def counting_init(self, m, n_, *a, **kw):
        init(self, m, n_, *a, **kw)
        made.append((int(m), int(n_)))
        alive.add(id(self))
        most[0] = max(most[0], len(alive))

    def counting_close(self):
        alive.discard(id(self))
        close(self)
    monkeypatch.setattr(device.DeviceBeagle, "__init__", counting_init)
    monkeypatch.setattr(device.DeviceBeagle, "close", counting_close)
    out = glassy.assignLL_windowed(path, A, W1)
    st = glassy.assignLL_windowed.stats
    assert st["windows"] == 4 and st["largest_matrix_bytes"] == one_window and st["seconds"] > 0
    assert made == [(8192, n), (8192, n)] and st["matrices"] == 2 and most[0] == 2 and not alive
    assert np.array_equal(out, resident_totals(path, A))


def run_cli(argv):
    from wgsassign_amd import WGSassign
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        WGSassign.main(argv)
    return out.getvalue(), err.getvalue()


@pytest.mark.parametrize("bgzf", [False, True])
def test_command_line(files, tmp_path, monkeypatch, bgzf):
    """--get_pop_like as today and with WGSASSIGN_WINDOW_SITES=8192: the same bytes in .pop_like.txt, the same stdout, one more line on
    stderr; with --get_reference_af beside it the resident path runs and says nothing of windows."""
    m, n, K = 20000, 6, 3
    path, A = files(m, n, K)
    if bgzf:
        src, path = path, str(tmp_path / "copy.beagle.gz")
        synth.write_bgzf(path, gzip.open(src, "rb").read(), block=50000)
    af = str(tmp_path / "ref.pop_af.npy")
    np.save(af, A)
    argv = ["--beagle", path, "--pop_af_file", af, "--get_pop_like", "--threads", "2"]
    out1, err1 = run_cli(argv + ["--out", str(tmp_path / "a")])
    monkeypatch.setenv("WGSASSIGN_WINDOW_SITES", "8192")
    out2, err2 = run_cli(argv + ["--out", str(tmp_path / "b")])
    assert open(str(tmp_path / "a.pop_like.txt"), "rb").read() == open(str(tmp_path / "b.pop_like.txt"), "rb").read()
    assert out1.replace(str(tmp_path / "a"), "OUT") == out2.replace(str(tmp_path / "b"), "OUT")
    assert "window" not in err1
    assert [l for l in err2.splitlines() if "window" in l] == ["wgsassign_amd: scored in 3 windows of 8192 sites"]
    ids = str(tmp_path / "ids.txt")
    np.savetxt(ids, synth.pop_labels(n, K), fmt="%s", delimiter="\t")
    out3, err3 = run_cli(argv + ["--get_reference_af", "--pop_af_IDs", ids, "--out", str(tmp_path / "c")])
    assert "window" not in err3 and os.path.exists(str(tmp_path / "c.pop_like.txt"))
