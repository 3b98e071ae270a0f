"""CPU-only: the integer-table mode of the streamed reader (wgs_reader_open_table: allele depths, ANGSD counts) -- line listing,
column count, line numbers and the host parser of the lines the device flags, against np.loadtxt on plain, gzip and BGZF files --
and the command line's checks of --ind_counts_file / --ind_majmin_file."""
import ctypes
import gzip
import io
import warnings

import numpy as np
import pytest

import synth

VARIANTS = {
    "tabs": "1\t2\t3\t4\n5\t6\t7\t8\n",
    "spaces": "1 2  3   4\n5 6 7 8\n",
    "blanks_around": " \t1\t2\t3\t4\t\n5\t6\t7\t8 \t \n",            # ANGSD ends every counts line with a tab
    "crlf": "1\t2\t3\t4\r\n5\t6\t7\t8\r\n",
    "blank_lines": "\n1 2 3 4\n\n \t\n5 6 7 8\n\n",
    "no_last_newline": "1 2 3 4\n5 6 7 8",
    "comments": "# a comment first\n1 2 3 4 # trailing\n#another\n5 6 7 8\n",
    "signs_and_zeros": "+1 002 3 4\n5 6 0007 255\n",
    "extra_columns": "1 2 3 4 9 9\n5 6 7 8 9 9\n",
}


def write(path, text, fmt):
    data = text.encode()
    if fmt == "text":
        open(path, "wb").write(data)
    elif fmt == "gzip":
        with gzip.open(path, "wb") as fh:
            fh.write(data)
    else:
        synth.write_bgzf(path, data, block=7)            # members end inside lines and inside tokens


def table_rows(path, need, skip=0, chunk_bytes=1 << 20, max_rows=100000):
    from wgsassign_amd import _lib
    lib = _lib.load()
    r = ctypes.c_void_p()
    _lib.check(lib.wgs_reader_open_table(str(path).encode(), 2, skip, ctypes.byref(r)))
    try:
        cols = lib.wgs_reader_table_columns(r)
        rows = np.zeros((max_rows, need), dtype=np.int32)
        lines = np.zeros(max_rows, dtype=np.int64)
        n = ctypes.c_int64()
        _lib.check(lib.wgs_debug_reader_table_rows(r, chunk_bytes, need, _lib.i32p(rows), max_rows, ctypes.byref(n),
                                                   lines.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return cols, rows[:n.value], lines[:n.value]
    finally:
        lib.wgs_reader_close(r)


@pytest.mark.parametrize("fmt", ["text", "gzip", "bgzf"])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_text_variants_as_loadtxt_reads_them(tmp_path, name, fmt):
    text = VARIANTS[name]
    path = tmp_path / ("t." + fmt)
    write(path, text, fmt)
    want = np.loadtxt(io.StringIO(text), dtype=np.int32)
    cols, rows, lines = table_rows(path, 4)
    assert cols == want.shape[1]
    assert np.array_equal(rows, want[:, :4])
    # the 1-based file line of every row: data lines are those np.loadtxt keeps
    keep = [i + 1 for i, ln in enumerate(text.split("\n")) if ln.split("#")[0].strip()]
    assert lines.tolist() == keep


@pytest.mark.parametrize("fmt", ["text", "gzip", "bgzf"])
def test_header_line_and_many_chunks(tmp_path, fmt):
    """One header line (ANGSD counts), 3000 lines of uneven length in 16 KiB chunks: nothing lost or doubled at chunk ends."""
    rng = np.random.default_rng(4)
    tab = rng.integers(0, 300, size=(3000, 24))
    body = "".join("\t".join(str(v) for v in row) + "\t\n" for row in tab)
    path = tmp_path / ("c." + fmt)
    data = ("ind0TotDepthA\tind0TotDepthC\n" + body).encode()
    if fmt == "bgzf":
        synth.write_bgzf(path, data, block=5000)
    else:
        write(path, data.decode(), fmt)
    cols, rows, lines = table_rows(path, 24, skip=1, chunk_bytes=16 << 10)
    assert cols == 24
    assert np.array_equal(rows, tab)
    assert lines.tolist() == list(range(2, 3002))


def test_empty_and_header_only(tmp_path):
    for text, skip in (("", 0), ("head\n", 1), ("\n\n# only a comment\n", 0)):
        path = tmp_path / "e.txt"
        path.write_text(text)
        cols, rows, _ = table_rows(path, 2, skip=skip)
        assert cols == 0 and rows.shape[0] == 0


LINES = ["1 2 3", "1\t2\t3\t", "+1 -2 3", "1 2", "1 2 # 3", "1 2 3 # c", "1.0 2 3", "1e2 2 3", "2.9 -2.9 .5", "0x1 2 3", "1_0 2 3",
         "1 2 2147483647", "1 2 -2147483648", "01 002 0003", "1 2 3x", "- 2 3", "1 2 3 4 5", "1,2,3", "１ 2 3", "1 2 1e", "1 2 1.2.3"]


@pytest.mark.parametrize("line", LINES)
def test_host_parse_of_a_flagged_line_agrees_with_loadtxt(line):
    """The parser the ingest falls back to for lines the kernel flags: accepted exactly when np.loadtxt(dtype=int32) accepts the
    line with at least three columns, and then with the same values."""
    from wgsassign_amd import _lib
    raw = line.encode()
    out = np.zeros(3, dtype=np.int32)
    rc = _lib.load().wgs_debug_table_parse_line(raw, len(raw), 3, _lib.i32p(out))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)     # "parsing an integer via a float": NumPy still does, so do we
            want = np.atleast_1d(np.loadtxt(io.StringIO(line), dtype=np.int32))
        ok = want.shape[0] >= 3
    except ValueError:
        ok = False
    assert (rc == 0) == ok, (line, rc)
    if ok:
        assert out.tolist() == want[:3].tolist()


@pytest.mark.parametrize("line", ["1 2 2147483648", "1 2 99999999999", "1 2 1e10", "1 2 inf", "1 2 nan"])
def test_host_parse_refuses_what_no_int32_holds(line):
    """Beyond int32 NumPy's cast of the float is undefined; such a value fits no table, the parser refuses it."""
    from wgsassign_amd import _lib
    raw = line.encode()
    out = np.zeros(3, dtype=np.int32)
    assert _lib.load().wgs_debug_table_parse_line(raw, len(raw), 3, _lib.i32p(out)) == 3


def test_a_bad_line_is_named_by_its_number_in_the_file(tmp_path):
    path = tmp_path / "bad.txt"
    path.write_text("1 2\n\n# c\n3 x\n5 6\n")
    with pytest.raises(ValueError, match="line 4, column 2"):
        table_rows(path, 2)
    path.write_text("h\n1 2\n3\n")
    with pytest.raises(ValueError, match="line 3 has fewer than 2 columns"):
        table_rows(path, 2, skip=1)


def test_table_readers_and_beagle_readers_do_not_mix(tmp_path):
    from wgsassign_amd import _lib
    lib = _lib.load()
    path = tmp_path / "t.txt"
    path.write_text("1 2\n")
    r = ctypes.c_void_p()
    _lib.check(lib.wgs_reader_open_table(str(path).encode(), 1, 0, ctypes.byref(r)))
    rows = np.zeros(4, dtype=np.float32)
    n = ctypes.c_int64()
    assert lib.wgs_reader_next(r, _lib.f32p(rows), 1, ctypes.byref(n)) == 2
    assert "integer table" in _lib.last_error()
    lib.wgs_reader_close(r)
    with pytest.raises(ValueError):
        _lib.check(lib.wgs_reader_open_table(str(tmp_path / "missing").encode(), 1, 0, ctypes.byref(r)))


# ---------------------------------------------------------------- the command line's option checks
def cli(tmp_path, *extra):
    from wgsassign_amd import WGSassign
    # the Beagle file does not exist: every check below has to fire before it is looked at
    WGSassign.main(["--beagle", str(tmp_path / "no.beagle.gz"), "--out", str(tmp_path / "o"), "--get_assignment_z_score"] + list(extra))


def test_cli_counts_options(tmp_path):
    counts, majmin, ad = tmp_path / "x.counts.gz", tmp_path / "x.majmin.txt", tmp_path / "x.ad.txt"
    with gzip.open(counts, "wt") as fh:
        fh.write("h\n1\t0\t0\t2\t\n")
    majmin.write_text("site major minor\ns1 0 3\n")
    ad.write_text("1 2\n")
    with pytest.raises(SystemExit, match="in place of --ind_ad_file"):
        cli(tmp_path, "--ind_counts_file", str(counts), "--ind_majmin_file", str(majmin), "--ind_ad_file", str(ad))
    with pytest.raises(SystemExit, match="--ind_majmin_file is missing"):
        cli(tmp_path, "--ind_counts_file", str(counts))
    with pytest.raises(SystemExit, match="--ind_counts_file is missing"):
        cli(tmp_path, "--ind_majmin_file", str(majmin))
    majmin.write_text("site major minor\ns1 0 3\ns2 4 1\n")
    with pytest.raises(SystemExit, match="line 3: allele selector outside 0..3"):
        cli(tmp_path, "--ind_counts_file", str(counts), "--ind_majmin_file", str(majmin))
    with pytest.raises(SystemExit, match="does not exist"):
        cli(tmp_path, "--ind_counts_file", str(tmp_path / "none.gz"), "--ind_majmin_file", str(majmin))
    # a valid pair passes the checks and gets as far as the device (none here: RuntimeError) or the missing Beagle file
    majmin.write_text("site major minor\ns1 0 3\n")
    with pytest.raises((AssertionError, RuntimeError)):
        cli(tmp_path, "--ind_counts_file", str(counts), "--ind_majmin_file", str(majmin))


def test_read_majmin_takes_columns_one_and_two(tmp_path):
    from wgsassign_amd import zscore
    p = tmp_path / "m.txt"
    p.write_text("chr_pos major minor extra\n7 2 0 9\n8 1 3 9\n")
    want = np.loadtxt(p, dtype="int", skiprows=1, usecols=(1, 2))
    got = zscore.read_majmin(p)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
