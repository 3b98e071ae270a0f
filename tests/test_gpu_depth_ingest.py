"""GPU: allele-depth and ANGSD-counts files tokenised on the device into the depth table (csrc/ingest.hip: depth_tokenise_kernel,
wgs_depth_ingest_*; zscore.DepthTable.from_file) -- read back with wgs_depth_download_rows and compared with np.loadtxt, exactly:
shapes around the 64-site tiles and the 256-individual strips, plain / gzip / BGZF, default and small chunks, every refusal with
its line number, the z-scores of the recorded cases through a streamed table, and the host memory the ingest held."""
import ast
import contextlib
import gzip
import hashlib
import io
import os

import numpy as np
import pytest

import synth
import synth_counts
import synth_depth
import test_gpu_zscore
from conftest import GOLDEN
from test_zscore_cpu import case_inputs, compare_individual, runs

pytestmark = pytest.mark.gpu

FORMATS = ("text", "gzip", "bgzf")
EDGE_VALUES = (0, 9, 10, 99, 100, 255)


def write_as(path, data, fmt, block=20000):
    if fmt == "text":
        with open(path, "wb") as fh:
            fh.write(data)
    elif fmt == "gzip":
        with gzip.open(path, "wb", compresslevel=1) as fh:
            fh.write(data)
    else:
        synth.write_bgzf(path, data, block=block)
    return str(path)


def table_text(AD):
    buf = io.BytesIO()
    np.savetxt(buf, AD, fmt="%d")
    return buf.getvalue()


def edge_table(m, n, seed):
    AD = synth_depth.make_depth(m, n, min(2, n), seed=seed)[1].copy()
    flat = AD.reshape(-1)
    for k, v in enumerate(EDGE_VALUES * 3):
        flat[(k * 7919 + k) % flat.size] = v
    flat[0], flat[-1] = 255, 100                       # first and last cell of the file
    return AD


class Shape:
    """A matrix of m x n that only gives the table its shape."""

    def __init__(self, m, n):
        from wgsassign_amd.device import DeviceBeagle
        self.b = DeviceBeagle(m, n)

    def __enter__(self):
        return self.b

    def __exit__(self, *exc):
        self.b.close()


def streamed(b, path, **kw):
    from wgsassign_amd import zscore
    t = zscore.DepthTable.from_file(b, path, **kw)
    try:
        return t.download_rows(), t.ingest_stats
    finally:
        t.close()


@pytest.mark.parametrize("n", [1, 13, 200])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 5003])
def test_equals_loadtxt_over_shapes_formats_and_chunks(tmp_path, m, n):
    AD = edge_table(m, n, seed=m + n)
    data = table_text(AD)
    want = np.atleast_2d(np.loadtxt(io.StringIO(data.decode()), dtype=np.int32))
    assert np.array_equal(want, AD)
    with Shape(m, n) as b:
        for fmt in FORMATS:
            path = write_as(tmp_path / ("ad." + fmt), data, fmt)      # (the container is told by the file's bytes, not its name)
            got, st = streamed(b, path)
            assert np.array_equal(got, want), (fmt, "default chunks")
            assert st["host_lines"] == 0 and st["lines"] == m
            # small chunks: 16 KiB of text through the host's inflater, one BGZF member's worth (64 KiB) on the device
            got, st = streamed(b, path, chunk_bytes=1)
            assert np.array_equal(got, want), (fmt, "small chunks")
            if len(data) >= 6 * 65536:
                assert st["chunks"] >= 5, (fmt, st)
            if fmt == "bgzf" and len(data) > 2 << 20:           # (opening the reader inflates up to 1 MiB on the host: the first line)
                assert st["members_on_device"] > 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_more_individuals_than_a_strip_and_extra_columns(tmp_path, fmt):
    """300 and 700 individuals: the strips of 256 follow one another inside a workgroup; columns behind 2n are ignored.
    20000 individuals: a line of 80 KB and more is longer than a small device chunk (64 KiB), so every chunk is carried whole
    into the next and the text buffer grows while it holds the carry."""
    for m, n, extra in ((130, 300, 0), (77, 700, 0), (200, 257, 3), (40, 20000, 0)):
        AD = edge_table(m, n, seed=n)
        full = np.hstack([AD, np.full((m, extra), 7, dtype=np.int32)]) if extra else AD
        path = write_as(tmp_path / ("w%d.%s" % (n, fmt)), table_text(full), fmt)
        with Shape(m, n) as b:
            for chunk in (None, 1):
                got, st = streamed(b, path, chunk_bytes=chunk)
                assert np.array_equal(got, AD), (n, chunk)
                assert st["host_lines"] == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_text_variants_and_flagged_lines(tmp_path, fmt):
    """What np.loadtxt accepts comes out the same: the kernel takes the plain lines, the host the flagged ones."""
    text = (" 1\t2   3 4 \r\n"            # blanks around, repeated spaces, CRLF
            "\n"
            "# a comment line\n"
            "5 6 7 8\t\n"
            "+9 010 0011 12\n"            # a sign, leading zeros beyond three characters: the host's lines
            "13 14 15 16 # trailing comment\n"
            " \t \n"
            "17 18 1.9e1 20.7\n"          # NumPy still reads integers via floats (deprecated): truncated
            "255 0 100 99")               # no newline at the end
    path = write_as(tmp_path / ("v." + fmt), text.encode(), fmt, block=9)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        want = np.loadtxt(io.StringIO(text), dtype=np.int32)
    with Shape(want.shape[0], 2) as b:
        got, st = streamed(b, path)
        assert np.array_equal(got, want)
        assert st["host_lines"] == 2 and st["lines"] == 6       # (the trailing comment lies behind the 2n columns: not looked at)
        with Shape(want.shape[0], 1) as b1:
            got, _ = streamed(b1, path)
            assert np.array_equal(got, want[:, :2])


def test_a_million_sites(tmp_path):
    m, n = 1000003, 6
    rng = np.random.default_rng(12)
    AD = rng.poisson(0.75, size=(m, 2 * n)).astype(np.int32)
    AD[::100003, 3] = 255
    AD[5::77777, 0] = 100
    data = table_text(AD)
    with Shape(m, n) as b:
        for fmt in FORMATS:
            path = write_as(tmp_path / ("big." + fmt), data, fmt, block=60000)
            got, st = streamed(b, path)
            assert np.array_equal(got, AD), fmt
            assert st["host_lines"] == 0
            assert (st["members_on_device"] > 0) == (fmt == "bgzf")


# ---------------------------------------------------------------- counts mode
@pytest.fixture(scope="module")
def counts_gold():
    g = np.load(os.path.join(GOLDEN, "allele_counts.npz"), allow_pickle=False)
    counts, majmin = synth_counts.make_counts(**ast.literal_eval(str(g["gen"])))
    assert hashlib.sha256(counts.tobytes()).hexdigest() == str(g["counts_digest"]), "the generator no longer reproduces the recorded input"
    assert np.array_equal(majmin, g["majmin"])
    return g, counts, majmin


def test_counts_mode_against_the_recorded_reference(tmp_path, counts_gold):
    from wgsassign_amd import allele_counts
    g, counts, majmin = counts_gold
    cpath, mpath = str(tmp_path / "g.counts.gz"), str(tmp_path / "g.majmin.txt")
    synth_counts.write_counts(cpath, counts)
    synth_counts.write_majmin(mpath, majmin)
    m, n = g["out"].shape[0], g["out"].shape[1] // 2
    with Shape(m, n) as b:
        for chunk in (None, 1):
            got, st = streamed(b, cpath, counts=True, majmin=g["majmin"], chunk_bytes=chunk)
            assert np.array_equal(got, g["out"])
            assert st["host_lines"] == 0                          # ANGSD output flags no line
    # the module entry point: its file, gunzipped, byte for byte what the reference's script wrote
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        allele_counts.main([cpath, mpath])
    text = gzip.open(cpath + ".majmin.counts.txt.gz", "rb").read()
    assert hashlib.sha256(text).hexdigest() == str(g["text_digest"])
    out = str(tmp_path / "plain.txt")
    with contextlib.redirect_stdout(buf):
        allele_counts.main([cpath, mpath, "--out", out])
    assert open(out, "rb").read() == text


@pytest.mark.parametrize("fmt", FORMATS)
def test_counts_mode_wide_and_bgzf(tmp_path, fmt):
    """Four tokens per individual over more than one strip, all containers, against the restated np.take_along_axis."""
    counts, majmin = synth_counts.make_counts(333, 300, seed=3)
    head = b"h\t" * (4 * 300) + b"\n"
    body = b"".join(b"".join(b"%d\t" % v for v in row) + b"\n" for row in counts)
    path = write_as(tmp_path / ("c." + fmt), head + body, fmt)
    with Shape(333, 300) as b:
        for chunk in (None, 1):
            got, _ = streamed(b, path, counts=True, majmin=majmin.astype(np.uint8), chunk_bytes=chunk)
            assert np.array_equal(got, synth_counts.pick(counts, majmin))


# ---------------------------------------------------------------- every refusal, with its line, and no table left behind
def refused(b, path, match, **kw):
    from wgsassign_amd import zscore
    made = []

    class Watched(zscore.DepthTable):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    with pytest.raises(ValueError, match=match):
        Watched.from_file(b, path, **kw)
    assert len(made) == 1 and made[0]._h is None, "the table's handle outlived the refusal"


@pytest.mark.parametrize("fmt", FORMATS)
def test_refusals_name_the_line_and_leave_no_table(tmp_path, fmt):
    m, n = 200, 3
    AD = edge_table(m, n, seed=1)
    rows = [" ".join(str(v) for v in r) for r in AD]

    def file_of(lines, name):
        return write_as(tmp_path / (name + "." + fmt), ("\n".join(lines) + "\n").encode(), fmt, block=700)

    with Shape(m, n) as b:
        bad = list(rows)
        bad[149] = bad[149].replace(" ", " 256 ", 1).rsplit(" ", 1)[0]          # (still 2n columns)
        refused(b, file_of(bad, "big"), r"line 150: allele depths outside 0\.\.255 do not fit the device table")
        bad = list(rows)
        bad[10] = "-1 " + bad[10].split(" ", 1)[1]
        refused(b, file_of(bad, "neg"), r"line 11: allele depths outside 0\.\.255 do not fit")
        bad = ["", "# c"] + rows
        bad[2 + 77] = bad[2 + 77].rsplit(" ", 1)[0]                              # one column short, behind a blank and a comment line
        refused(b, file_of(bad, "short"), r"line 80 has fewer than 6 columns")
        bad = list(rows)
        bad[199] = bad[199].replace(" ", " 1x ", 1)
        refused(b, file_of(bad, "junk"), r"line 200, column 2: not an integer")
        refused(b, file_of(rows[:-1], "fewer"), r"has 199 data lines, 200 sites were expected")
        refused(b, file_of(rows + rows[:5], "more"), r"has 205 data lines, 200 sites were expected")
        refused(b, file_of(["1 2 3 4"] + rows[1:], "narrow"), r"line 1 has 4 columns, 3 individuals need 6")
        # counts mode: 4n columns wanted
        sel = np.zeros((m, 2), dtype=np.uint8)
        sel[:, 1] = 1
        refused(b, file_of(["h"] + rows, "c"), r"line 2 has 6 columns, 3 individuals need 12", counts=True, majmin=sel)
        # ... and the same matrix still takes a good file afterwards
        got, _ = streamed(b, file_of(rows, "good"))
        assert np.array_equal(got, AD)


# ---------------------------------------------------------------- z-scores through the streamed table
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "zscore.npz"), allow_pickle=False)


@pytest.mark.parametrize("fmt", FORMATS)
def test_recorded_z_scores_through_a_streamed_table(tmp_path, monkeypatch, gold, fmt):
    """Cases a, b, c of tests/golden/zscore.npz with the table built by DepthTable.from_file instead of the upload: the per-individual
    arrays and z of every recorded run, bit for bit."""
    from wgsassign_amd import zscore
    real = zscore.DepthTable
    count = [0]

    def from_a_file(b, AD, chunk_rows=None):
        count[0] += 1
        return real.from_file(b, write_as(tmp_path / ("ad%d.%s" % (count[0], fmt)), table_text(AD), fmt, block=3000), chunk_bytes=1)

    monkeypatch.setattr(zscore, "DepthTable", from_a_file)
    seen = set()
    for r, spec in runs(gold):
        L, AD, IDs, A = case_inputs(gold, spec["case"])
        z, details, lines = test_gpu_zscore.device_run(L, AD, IDs, A, spec["flavour"], spec["thr"], spec["srt"], spec["ind_start"], spec["ind_end"])
        lo = spec["ind_start"] or 0
        for j, d in enumerate(details):
            compare_individual(gold, r, lo + j, dict(d, sums=None), d.get("it"))
        assert lines == str(gold["run%d_stdout" % r]).splitlines()[:-1]
        seen.add((spec["case"], spec["flavour"]))
    assert count[0] == len(list(runs(gold)))
    assert {c for c, _ in seen} >= {"a", "b", "c"} and {f for _, f in seen} == {"assignment", "reference"}


def test_cli_with_a_bgzf_depth_file_and_with_angsd_counts(tmp_path, gold):
    from wgsassign_amd import WGSassign
    r, spec = next((r, s) for r, s in runs(gold) if s["flavour"] == "assignment" and not s["srt"] and s["ind_start"] is None)
    L, AD, IDs, A = case_inputs(gold, spec["case"])
    paths = synth_depth.write_inputs(str(tmp_path / "in"), L, AD, IDs, A)
    bgzf = write_as(tmp_path / "in.ad.txt.gz", open(paths["ad"], "rb").read(), "bgzf", block=5000)
    # ANGSD counts that hold the same depths: the reads of the reference allele on the major base, of the alternative on the minor
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
    for tag, depth_args in (("bgzf", ["--ind_ad_file", bgzf]), ("counts", ["--ind_counts_file", cpath, "--ind_majmin_file", mpath])):
        out = str(tmp_path / tag)
        argv = ["--beagle", paths["beagle"], "--pop_af_IDs", paths["ids"], "--pop_names", paths["names"], "--out", out,
                "--get_assignment_z_score", "--pop_af_file", paths["af"]] + depth_args
        if spec["thr"]:
            argv += ["--allele_count_threshold", str(spec["thr"])]
        with contextlib.redirect_stdout(io.StringIO()):
            WGSassign.main(argv)
        assert open(out + ".z_ind.txt").read() == str(gold["run%d_file" % r]), tag


# ---------------------------------------------------------------- host memory
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_memory_stays_at_chunks(tmp_path, fmt):
    """200 000 sites x 50 individuals: the (m, 2n) int32 array the parent path held is 80 MB; the largest host buffer of the streamed
    path -- reader buffers, page-locked staging, a flagged line's row -- stays below a tenth of that, with the default chunks."""
    m, n = 200000, 50
    rng = np.random.default_rng(2)
    AD = np.minimum(rng.poisson(1.5, size=(m, 2 * n)), 9).astype(np.uint8)
    txt = np.empty((m, 2 * n, 2), dtype=np.uint8)                # single digits: the text without formatting 2 * 10^7 numbers
    txt[:, :, 0] = AD + 48
    txt[:, :, 1] = 9
    txt[:, -1, 1] = 10
    path = write_as(tmp_path / ("mem." + fmt), txt.tobytes(), fmt, block=60000)
    with Shape(m, n) as b:
        got, st = streamed(b, path)
        assert np.array_equal(got, AD)
        print("largest host buffer: %d bytes, chunks: %d" % (st["host_peak_bytes"], st["chunks"]))
        assert 0 < st["host_peak_bytes"] < m * 2 * n * 4 / 10
