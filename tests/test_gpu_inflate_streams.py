"""The device inflate (csrc/inflate.hip) on hand-built deflate streams: the format, not one encoder's choices.  CRC32 is not
checked anywhere, so a copy piece taken one period too far back, a deferred store that lands behind the literal that should
overwrite it or a long code walked against the wrong counts would be silent corruption of every BGZF file's text.  The streams
(tests/deflate_cases.py, written by tests/deflate_build.py; zlib agrees with every expectation: tests/test_deflate_build_cpu.py)
reach the branches zlib's own output reaches by chance or never: every distance 1..80 with every length at every output phase,
every member tail for all three ways of copying, long codes in wavefronts of chosen composition, matches of 48 bits at every
bit phase, every order of block types, the corners of the dynamic header, and the streams that must be refused.

Every family runs at each input alignment in_off = 0..7 (mod 8), its output slots between 64 guard bytes that must stay zero
(the hook zeroes the buffer and no data byte is zero).  A valid stream must come out with status 0 and exactly the expected
bytes: refusing it would be hidden by the host's fallback, at a cost."""
import numpy as np
import pytest

import deflate_cases as dc
from inflate_dev import check_launch

pytestmark = pytest.mark.gpu

ALIGNMENTS = range(8)


def run(cases, in_align):
    wrong = check_launch(cases, in_align)
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("in_align", ALIGNMENTS)
def test_a_match_geometry(in_align):
    """Fixed-code streams, one per distance (1..80 and 255 .. 32768) and output phase 0..15: every length 3..258 between one
    to three literals, matches back to back, matches whose source is the tail of the match before them."""
    run(dc.family_a()[0], in_align)


@pytest.mark.parametrize("in_align", ALIGNMENTS)
def test_b_member_tails(in_align):
    """A match, S = 0..80 literals, the end of the member: `pos + 16 <= want` and `pos + 64 <= want` from both sides for the far,
    the near and the bytewise copy, the last piece ending exactly at ISIZE among them."""
    run(dc.family_b()[0], in_align)


@pytest.mark.parametrize("in_align", ALIGNMENTS)
def test_c_long_codes_and_the_collective_walk(in_align):
    """Used literal, length and distance symbols at every code length beyond the tables, the end-of-block at 15 bits; k streams
    of long codes among 64 - k of short codes for k = 1, 3, 11, 12, 16, 63, 64 (the walk's thresholds), launches of 1, 65 and 127
    streams, and a wavefront whose members' ISIZE runs from 0 (the BGZF EOF member) to 65536."""
    for name, cases in dc.family_c()[0].items():
        run(cases, in_align)


@pytest.mark.parametrize("in_align", ALIGNMENTS)
def test_d_matches_of_48_bits(in_align):
    """15 + 5 + 15 + 13 bits per match, back to back behind a stored block of 32768 bytes, extra bits all zeros, all ones and
    random: a trip refills only below 48 bits."""
    run(dc.family_d()[0], in_align)


@pytest.mark.parametrize("in_align", ALIGNMENTS)
def test_e_block_structure_and_headers(in_align):
    """Members of 2..40 blocks in every order of types, stored blocks at every bit phase and LEN at every byte of an input word,
    empty blocks, the extremes of HLIT / HDIST / HCLEN, the longest code-length repeats, zlib's flushes."""
    run(dc.family_e()[0], in_align)


@pytest.mark.parametrize("in_align", ALIGNMENTS)
def test_n_refused_streams_between_valid_ones(in_align):
    """Each a valid stream with one defect: status != 0, guards untouched, the valid members on both sides intact."""
    run(dc.family_n()[0], in_align)
    run(dc.family_n_unusable_header() + dc.family_n()[0][:1], in_align)


@pytest.mark.parametrize("in_align", ALIGNMENTS)
def test_incomplete_code_sets_are_refused_or_decoded(in_align):
    """zlib refuses an incomplete literal/length set and an incomplete distance set of several codes at the header; the kernel
    checks for over-subscription only.  Either is right here: refused (the host's inflater then reports the member), or decoded
    to what the tokens stand for -- every code the streams use exists.
    On the MI355X both are decoded (status 0, the expected bytes), at every input alignment."""
    from inflate_dev import Launch
    cases = dc.family_incomplete()
    good = dc.family_n()[0][0]
    r = Launch([good[0]] + [c[0] for c in cases] + [good[0]], [good[1]] + [c[1] for c in cases] + [good[1]], in_align, 64)
    slots = r.slots()
    print("incomplete sets: status", r.status[1:-1].tolist())
    assert r.status[0] == 0 and slots[0] == good[2] and r.status[-1] == 0 and slots[-1] == good[2]
    for i, (_, isize, expected, label) in enumerate(cases, 1):
        assert r.status[i] != 0 or slots[i] == expected, label
    used = np.zeros(r.out.size, dtype=bool)
    for o, n in zip(r.out_off, r.isize):
        used[int(o):int(o) + int(n)] = True
    assert not r.out[~used].any()


def test_f_hand_built_members_through_the_ingest(tmp_path, monkeypatch):
    """A Beagle file whose last 300 sites lie in hand-built BGZF members (cut mid-line and mid-number, 2..4 blocks of mixed type
    around an empty stored block and a stored block) through stream_to_device: the bits of the same file inflated by zlib on the
    host, every hand-built member inflated by the kernel and none left to the host's inflater."""
    from wgsassign_amd import reader_cy
    monkeypatch.setenv("WGSASSIGN_INDEX_DIR", str(tmp_path))
    blob, cases, body = dc.family_f()
    path = str(tmp_path / "built.beagle.gz")
    with open(path, "wb") as fh:
        fh.write(blob)

    def read():
        b, samples, sites, _ = reader_cy.stream_to_device(path)
        try:
            return b.download_rows(0, b.m), samples, sites, b.ingest_stats
        finally:
            b.close()

    rows, samples, sites, stats = read()
    monkeypatch.setenv("WGSASSIGN_INFLATE", "zlib")
    rows_z, samples_z, sites_z, _ = read()
    assert rows.shape == (dc.F_SITES, 2 * dc.F_INDIVIDUALS) and rows.shape == rows_z.shape and rows.tobytes() == rows_z.tobytes()
    assert samples == samples_z and sites == sites_z and len(sites) == dc.F_SITES
    assert stats["blocks_left_to_host_inflater"] == 0 and stats["blocks_inflated_on_device"] >= len(cases) > 20
