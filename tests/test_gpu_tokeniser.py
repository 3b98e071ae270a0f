"""GPU: the two device tokenisers (csrc/ingest.hip: tokenise_kernel with parse_token, depth_tokenise_kernel) held to the
specification of tests/token_cases.py -- atof, then (float), for every token; np.loadtxt for the integer tables -- on
enumerated tokens and enumerated alignments.  Every assertion is equality: of the downloaded slabs or table with the
expectation, bit for bit, and of ingest_stats["host_lines"] with the number of lines that hold a token outside the grammar
the device documents -- so neither a line the host quietly re-parsed nor a line the device should have left to it passes.
tests/test_token_cases_cpu.py holds the specification itself to the host parser, to exact arithmetic and to np.loadtxt, and
counts the coverage of the alignment files for every offset at which a line can begin in its chunk."""
import functools
import gzip
import io

import numpy as np
import pytest

import synth
import token_cases as tc
from test_gpu_depth_ingest import FORMATS, Shape, streamed, write_as
from test_gpu_ingest import device_rows

pytestmark = pytest.mark.gpu
CONTAINERS = ("gzip", "bgzf")              # gzip: the host inflates and lists the lines; BGZF: the device does both


def write(tmp_path, text, container):
    p = str(tmp_path / ("f_%s.beagle.gz" % container))
    if container == "bgzf":
        synth.write_bgzf(p, text, block=60000 if len(text) > (8 << 20) else 9973)
    else:
        with gzip.open(p, "wb", compresslevel=1) as fh:
            fh.write(text)
    return p


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def hold(tmp_path, monkeypatch, text, want, flagged, container, names=None, group_of=None, n_groups=1):
    monkeypatch.setenv("WGSASSIGN_INDEX_DIR", str(tmp_path))
    rows, _, sites, stats = device_rows(write(tmp_path, text, container), group_of=group_of, n_groups=n_groups)
    assert rows.shape == want.shape and rows.dtype == want.dtype
    bad = np.argwhere(bits(rows) != bits(want))
    assert bad.size == 0, "%d values differ, first (row, column, device, atof32): %s" % (
        len(bad), [(int(r), int(c), float(rows[r, c]), float(want[r, c])) for r, c in bad[:6]])
    assert names is None or sites == names
    assert stats["host_lines"] == flagged, "the host parsed %d lines, %d hold a token outside the device's grammar" % (stats["host_lines"], flagged)


@pytest.mark.parametrize("lead", range(10))
def test_every_f6_token(tmp_path, monkeypatch, lead):
    """All 10^7 "d.dddddd", a decade per case: the SWAR path."""
    text, want = tc.f6_decade(lead)
    hold(tmp_path, monkeypatch, text, want, 0, "gzip")


@pytest.fixture(scope="module")
def contract():
    return tc.contract_case()


@pytest.mark.parametrize("container", CONTAINERS)
def test_random_tokens_of_the_accepted_grammar(tmp_path, monkeypatch, contract, container):
    assert contract.flagged == 0 and contract.want.size == tc.CONTRACT_COUNT
    hold(tmp_path, monkeypatch, contract.text, contract.want, 0, container, contract.names)


@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("name", ["ties", "grammar", "substituted", "beyond_contract"])
def test_enumerated_tokens(tmp_path, monkeypatch, name, container):
    """Float32 ties with their neighbours; the whole grammar over 0 1 7 . - + e E up to five characters; every byte at every place
    of two SWAR tokens; what lies just beyond the contract.  Lines of accepted tokens are the device's, the others the host's."""
    case = tc.BEAGLE_CASES[name]()
    assert (case.flagged > 0) and case.flagged < len(case.names)
    hold(tmp_path, monkeypatch, case.text, case.want, case.flagged, container, case.names)


@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("length", tc.ALIGN_LENGTHS)
def test_every_alignment_of_every_token_length(tmp_path, monkeypatch, length, container):
    """Tokens of one length in lines that pass two steps of a wavefront, the site name lengthened by 0..1039 bytes: whatever offset
    the lines begin at, a token of this length begins at every byte of a word, and begins and ends at every byte from 16 before
    to 1 behind the first step boundary.  Lengths above 16 are the host's, line by line."""
    case = tc.alignment_case(length)
    a, b = tc.file_spans(case.lines, case.n)
    for offset in range(16):
        assert tc.Coverage(offset, a, b).missing([length]) == [], offset
    assert case.flagged == (len(case.lines) if length > 16 else 0)
    hold(tmp_path, monkeypatch, case.text, case.want, case.flagged, container, case.names)


@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("k", range(16))
def test_separators_line_ends_and_header_lengths(tmp_path, monkeypatch, k, container):
    case = tc.separator_case(k)
    hold(tmp_path, monkeypatch, case.text, case.want, case.flagged, container, case.names)


@pytest.mark.parametrize("container", CONTAINERS)
def test_columns_the_kernel_must_not_look_at(tmp_path, monkeypatch, container):
    case = tc.ignored_columns_case()
    hold(tmp_path, monkeypatch, case.text, case.want, 0, container, case.names)


@pytest.mark.parametrize("container", CONTAINERS)
def test_placement_over_interleaved_populations_and_tiles(tmp_path, monkeypatch, container):
    case = tc.placement_case()
    hold(tmp_path, monkeypatch, case.text, case.want, case.flagged, container, case.names, case.group_of, case.n_groups)


# ---------------------------------------------------------------- the depth tokeniser
@functools.lru_cache(maxsize=None)
def depth_case(name):
    """The case and what np.loadtxt reads from its text (counts: from which the selected pairs are taken)."""
    case = tc.DEPTH_CASES[name]()
    table = np.atleast_2d(np.loadtxt(io.StringIO(case.text.decode()), dtype=np.int32, skiprows=1 if case.counts else 0))
    if case.counts:
        c = table.reshape(len(case.lines), case.n, 4)
        sel = case.majmin.astype(np.int64)
        table = np.empty((len(case.lines), 2 * case.n), dtype=np.int32)
        for w in range(2):
            table[:, w::2] = np.take_along_axis(c, np.broadcast_to(sel[:, None, w:w + 1], c.shape[:2] + (1,)), 2)[:, :, 0]
    if case.want is not None:
        assert np.array_equal(table, case.want)                     # ... which are the integers the text was written from
    return case, table


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", sorted(tc.DEPTH_CASES))
def test_depth_tokeniser(tmp_path, name, fmt):
    """forms: every value 0..255 as %d, %02d and %03d at every byte of a word and across the first step boundary, behind 0..1039
    blanks.  strip_*: 257 and 513 individuals, the first token of individuals 256 and 512 on every byte of a step.  tile_*: 63..129
    such lines.  counts: four tokens per individual, every pair of selectors.  flagged: +7, 0007, 00255 at the first, a middle
    and the last column and as individuals 255 and 256 -- the host's lines, and only they."""
    case, want = depth_case(name)
    path = write_as(tmp_path / ("d." + fmt), case.text, fmt, block=9973)
    with Shape(want.shape[0], case.n) as b:
        got, st = streamed(b, path, counts=case.counts, majmin=case.majmin)
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and bad.size == 0, "%d cells differ, first (row, column, device, loadtxt): %s" % (
        len(bad), [(int(r), int(c), int(got[r, c]), int(want[r, c])) for r, c in bad[:6]])
    assert st["host_lines"] == case.flagged
