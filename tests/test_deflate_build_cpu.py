"""The hand-built deflate streams (tests/deflate_build.py, tests/deflate_cases.py) against zlib, without a GPU: zlib inflates every
valid stream to exactly the expected bytes and refuses every stream that must be refused -- so what the device inflate is held
to in tests/test_gpu_inflate_streams.py is RFC 1951 as an independent decoder reads it, not the writer's opinion.  And every
family's covered set is counted from its inputs, so that an edit of the generators cannot thin it out unnoticed."""
import itertools
import zlib

import numpy as np
import pytest

import deflate_build as db
import deflate_cases as dc


def check_against_zlib(cases):
    wrong = []
    for stream, isize, expected, label in cases:
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress(stream)
        except zlib.error as e:
            if expected is not None:
                wrong.append("%s: zlib says %s" % (label, e))
            continue
        if expected is None:
            # refused by zlib itself, not finished (a truncation), or a stream that does not make the member's ISIZE
            if d.eof and len(out) == isize:
                wrong.append("%s: zlib accepts it" % label)
        elif out != expected or not d.eof or d.unused_data or len(out) != isize or 0 in out:
            wrong.append("%s: %d bytes of %d, eof %s, %d unused" % (label, len(out), isize, d.eof, len(d.unused_data)))
    assert not wrong, wrong[:10]


def test_writer_pieces():
    assert [db.length_code(n) for n in (3, 10, 11, 12, 257, 258)] == [(257, 0, 0), (264, 0, 0), (265, 1, 0), (265, 1, 1), (284, 5, 30), (285, 0, 0)]
    assert db.length_code(258, long258=True) == (284, 5, 31)
    assert [db.dist_code(n) for n in (1, 4, 5, 6, 7, 24577, 32768)] == [(0, 0, 0), (3, 0, 0), (4, 1, 0), (4, 1, 1), (5, 1, 0), (29, 13, 0), (29, 13, 8191)]
    assert db.expand([97, 98, 99, (7, 3), (3, 10), (4, 1)]) == b"abcabcabcaabcc" + b"ccc"
    assert db.expand([(3, 2)], b"xy") == b"xyx"
    with pytest.raises(ValueError):
        db.expand([97, (3, 2)])
    # the canonical code of RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) give F = 00, A = 010 ... H = 1111
    codes = db.canonical([3, 3, 3, 3, 3, 2, 4, 4])
    assert codes[5] == (0, 2) and codes[0] == (0b010, 3) and codes[1] == (0b110, 3) and codes[7] == (0b1111, 4) and codes[6] == (0b0111, 4)
    rng = np.random.default_rng(1)
    for limit, n in ((15, 286), (7, 19), (15, 30)):
        for _ in range(20):
            f = [int(x) for x in (rng.random(n) ** 12 * 1e6)]
            lens = db.huffman_lengths(f, limit)
            assert max(lens) <= limit and db.kraft(lens, limit) == 1 << limit and all(bool(a) == bool(b) for a, b in zip(f, lens) if a)
    lens = db.complete([0, 3, 0, 15, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], 15, pad_symbols=range(17))
    assert lens[1] == 3 and lens[3] == 15 and lens[4] == 9 and db.kraft(lens) == 1 << 15
    assert [(s, n) for _, s, _, _, n in db.rle_code_lengths([0] * 139 + [5] * 8 + [0] * 10 + [3])] == [(18, 138), (0, 1), (5, 1), (16, 6), (5, 1), (17, 10), (3, 1)]
    text = dc.beagle_text(20000, seed=3)
    for max_dist, min_len in ((32768, 3), (100, 3), (32768, 8)):
        tokens = db.tokenize(text, max_dist, min_len)
        assert db.expand(tokens) == text and all(t[0] >= min_len and t[1] <= max_dist for t in tokens if isinstance(t, tuple))
        assert zlib.decompress(db.Deflate().dynamic(tokens, True).getvalue(), -15) == text
    w = db.Deflate().fixed([65], False).raw_bits(0b101, 3).stored(b"xyz", True)
    assert w.blocks[1]["bit"] == 3 + 8 + 7 + 3 and w.getvalue()[-3:] == b"xyz"


def test_family_a_match_geometry():
    cases, cover = dc.family_a()
    check_against_zlib(cases)
    far = set(itertools.product(dc.A_FAR_LENGTHS, dc.A_FAR))
    assert cover["pairs"] >= set(itertools.product(range(3, 259), range(1, 81))) | far
    assert set(dc.A_FAR) == {255, 256, 257, 4095, 4096, 4097, 32767, 32768}
    assert cover["phases"] == set(itertools.product(dc.A_NEAR + dc.A_FAR, range(16)))
    assert cover["back_to_back"] == set(dc.A_NEAR + dc.A_FAR)
    # a match whose source is the tail of the match before it, through every way of copying (short period, 16 bytes, 64 bytes)
    assert {(d,) + (l2, d2) for d in dc.A_NEAR + dc.A_FAR for _, l2, d2 in dc.A_PENDING} <= cover["pending"]
    assert {d2 for _, _, d2 in dc.A_PENDING} >= {1, 3, 5, 15, 16, 20, 64, 65}
    assert max(c[1] for c in cases) <= 65536 and len(cases) == 88 * 16


def test_family_b_member_tails():
    cases, cover = dc.family_b()
    check_against_zlib(cases)
    assert cover == set(itertools.product((1, 2, 7, 9, 15, 16, 17, 63, 64, 65, 300), (3, 15, 16, 17, 32, 33, 48, 49, 64, 65, 258), range(81)))
    assert len(cases) == len(cover)


def test_family_c_long_codes():
    launches, cover = dc.family_c()
    for cases in launches.values():
        check_against_zlib(cases)
    lits, lens, dists, eob = cover["used"]
    assert lits >= set(range(9, 16)) and lens >= set(range(9, 16)) and dists >= set(range(8, 16)) and eob == 15
    assert cover["mixes"] == {k: k for k in (1, 3, 11, 12, 16, 63, 64)} and len(launches["mixes"]) == 7 * 64
    assert len({c[1] for c in launches["mixes"]}) == 1                        # equal ISIZE
    assert cover["launch_sizes"] >= {1, 65, 127, 64}
    sizes = cover["retire_sizes"]
    assert len(sizes) == 64 and sizes[0] == 0 and sizes[-1] == 65536 and launches["retire"][0][0] == bytes([3, 0]) and len(set(sizes)) >= 60
    for seed in range(8):
        tokens = dc.heavy_pair(seed)[3]
        lit, dist = dc.heavy_codes()
        # a 15-bit length code directly followed by a 15-bit distance code; the last symbols of the input are long codes
        assert any(isinstance(t, tuple) and lit[db.length_code(t[0])[0]] == 15 and dist[db.dist_code(t[1])[0]] == 15 for t in tokens)
        assert isinstance(tokens[-1], tuple) and dist[db.dist_code(tokens[-1][1])[0]] == 15 and lit[db.EOB] == 15


def test_family_d_the_48_bit_trip():
    cases, cover = dc.family_d()
    check_against_zlib(cases)
    assert cover["phases_48"] == set(range(8))
    assert cover["syms"] == {281, 282, 283, 284, 26, 27, 28, 29}
    assert {("zeros", False, False), ("ones", True, True)} <= cover["extras"] and any(m == "random" for m, _, _ in cover["extras"])
    lit, dist = dc.d_codes()
    assert all(lit[s] == 15 for s in (281, 282, 283, 284)) and all(dist[s] == 15 for s in (26, 27, 28, 29))


def test_family_e_block_structure():
    cases, cover = dc.family_e()
    check_against_zlib(cases)
    assert cover["orders"] >= set(itertools.product((0, 1, 2), repeat=2)) | set(itertools.product((0, 1, 2), repeat=3))
    assert {len(k) for k in cover["orders"]} == set(range(2, 41))
    assert cover["stored_phase"] == set(range(8)) and cover["len_at"] == set(range(8))
    assert cover["empties"] == set(itertools.product((0, 1, 2), (0, 1, 2)))
    assert {257, 286} <= cover["hlit"] and {1, 30} <= cover["hdist"] and {5, 19} <= cover["hclen"] and cover["clen_max"] == 7
    assert cover["dist_single"] == {0, 1}
    assert {(16, 6), (17, 10), (18, 138)} <= cover["repeats"] and cover["across"]
    assert cover["flushes"] == {"sync", "full", "partial"}
    assert max(c[1] for c in cases) == 65536


def test_family_n_refused_streams():
    cases, cover = dc.family_n()
    check_against_zlib(cases)
    check_against_zlib(dc.family_n_unusable_header())
    assert cover["defects"] == [
        "distance = pos + 1", "match overruns ISIZE by one byte", "literal overruns ISIZE by one byte", "stored block overruns ISIZE by one byte",
        "stream one byte short of ISIZE", "stored stream one byte short of ISIZE", "symbol 286 in a fixed block", "symbol 287 in a fixed block",
        "distance symbol 30 in a fixed block", "distance symbol 31 in a fixed block", "over-subscribed literal/length set",
        "over-subscribed distance set", "over-subscribed code-length set", "no end-of-block code", "symbol 16 first", "repeat past HLIT + HDIST",
        "HLIT 287", "NLEN wrong", "block type 3", "cut inside the header", "cut inside a code", "cut inside the extra bits"]
    assert cases[0][2] is not None and cases[-1][2] is not None
    assert all((c[2] is None) == (i % 2 == 1) for i, c in enumerate(cases))            # valid members on both sides of every one
    for stream, isize, expected, label in dc.family_incomplete():
        with pytest.raises(zlib.error):
            zlib.decompress(stream, -15)
        assert len(expected) == isize


def test_family_f_members():
    blob, cases, body = dc.family_f()
    check_against_zlib(cases)
    import gzip
    assert gzip.decompress(blob) == body and len(cases) >= 20
