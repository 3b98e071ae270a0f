#!/usr/bin/env python3
"""Writes the inputs of tests/c_abi/reader_trace.cpp into this directory:  python3 make_fixtures.py

Everything is derived from fixed formulas (no random numbers), with periodic values and a distinct site name per line, so
that 3 MiB of text deflate to tens of kilobytes.  The compressed bytes are committed: the trace then does not depend on the
zlib that happens to be installed where the test runs.  Re-running this script with another zlib may change the files
(same text, other deflate streams); tests/golden/reader_trace.txt then has to be recorded again."""
import os
import struct
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
N_IND = 12
LINES = 9800
TRIPLES = ["0.333333\t0.333333\t0.333334", "0.000000\t0.999999\t0.000001", "0.250000\t0.500000\t0.250000",
           "1.000000\t0.000000\t0.000000", "0.000133\t0.011402\t0.988465"]
ODD = ["1e-3\t.5\t0.4990", "0.1234567890123456789\t+0.25\t0.5", "nan\t0x1p-2\t0", "0.75\t1E-2\t0.24"]   # the strtod path


def header(names):
    return "marker\tallele1\tallele2\t" + "\t".join("%s\t%s\t%s" % (x, x, x) for x in names)


def line(s):
    vals = [TRIPLES[(s + (i >> 2)) % len(TRIPLES)] for i in range(N_IND)]
    if s % 997 == 5:
        vals[s % N_IND] = ODD[(s // 997) % len(ODD)]
    return "chr%d_%d\t%d\t%d\t" % (1 + s // 4000, 100 + 37 * s, s % 4, (s + 1) % 4) + "\t".join(vals)


def beagle_text(line_end="\n", final_newline=True, blanks=False, partial=False):
    names = ["Ind%d" % i for i in range(N_IND)]
    head = header(names) + ("\tIndP\tIndP" if partial else "")
    out = [head]
    for s in range(LINES):
        out.append(line(s) + ("\t0.5\t0.5" if partial else ""))
        if blanks and s % 1500 == 7:
            out.append("" if s % 3000 == 7 else " \t ")
    return (line_end.join(out) + (line_end if final_newline else "")).encode()


def gzip_member(data, flush_every=0):
    """One gzip member (header time 0).  flush_every: end a deflate block about every so many bytes of text, which is where an
    index pass can place its access points -- level 9 on text like this would otherwise emit blocks of megabytes."""
    c = zlib.compressobj(9, zlib.DEFLATED, 31)
    out = []
    step = flush_every or len(data) or 1
    for at in range(0, len(data), step):
        out.append(c.compress(data[at:at + step]))
        if flush_every and at + step < len(data):
            out.append(c.flush(zlib.Z_SYNC_FLUSH))
    out.append(c.flush())
    return b"".join(out)


def bgzf_member(data, extra=b""):
    """One BGZF member: the 'BC' subfield first, then `extra` (further subfields, already encoded)."""
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    xlen = 6 + len(extra)
    size = 12 + xlen + len(body) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + b"BC\x02\0" + struct.pack("<H", size - 1) + extra + body +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bgzf_members(data, member_bytes):
    return [bgzf_member(data[at:at + member_bytes]) for at in range(0, len(data), member_bytes)] + [bgzf_member(b"")]


def planted(data, member_bytes):
    """A BGZF file in which the byte range of part 1 of 2 starts inside the header of a member M whose extra field holds, in a
    second subfield, the 16-byte BGZF signature and a member size that leads to the true member after M: a pass in two parts
    takes the planted bytes for a block boundary, and the parts do not chain."""
    texts = [data[at:at + member_bytes] for at in range(0, len(data), member_bytes)]
    plain = [bgzf_member(t) for t in texts] + [bgzf_member(b"")]
    sig = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"
    k = len(texts) // 2
    for empties in range(0, 400):                            # empty members (legal BGZF) move the middle of the file in steps of 14 bytes
        def build(fake):
            extra = b"PL" + struct.pack("<H", 18) + sig + struct.pack("<H", fake)
            return plain[:k] + [bgzf_member(texts[k], extra)] + plain[k + 1:] + [bgzf_member(b"")] * empties
        ms = build(0)
        start = sum(len(m) for m in ms[:k])
        at = start + 12 + 6 + 4                              # file offset of the planted signature
        half = sum(len(m) for m in ms) // 2
        if start < half <= at:
            return b"".join(build(start + len(ms[k]) - at - 1))
    raise SystemExit("no member header straddles the middle of the file")


def table_text():
    out = ["# allele depths", "ind0 ind1 ind2 ind3 ind4 ind5"]           # two header lines, skipped by number
    for s in range(4000):
        if s % 400 == 3:
            out.append("# block %d" % (s // 400))
        if s % 700 == 11:
            out.append("" if s % 1400 == 11 else "  \t")
        row = " ".join(str((s * (c + 3) + c) % 23) for c in range(6))
        out.append(row + ("   # deep" if s % 900 == 13 else ""))
    return ("\n".join(out) + "\n").encode()


def main():
    text = beagle_text()
    assert len(text) >= 3 << 20
    files = {
        "beagle.gz": gzip_member(text, 200000),
        "beagle_b60000.gz": b"".join(bgzf_members(text, 60000)),
        "beagle_b700.gz": b"".join(bgzf_members(text, 700)),
        "beagle_cat.gz": b"".join(gzip_member(text[a:b]) for a, b in [(0, 100), (100, 900001), (900001, 900002), (900002, 2500000), (2500000, len(text))]),
        "beagle_crlf.gz": gzip_member(beagle_text(line_end="\r\n"), 200000),
        "beagle_blanks.gz": b"".join(bgzf_members(beagle_text(final_newline=False, blanks=True), 60000)),
        "beagle_partial.gz": gzip_member(beagle_text(partial=True), 200000),
    }
    table = table_text()
    assert len(table) >= 3 * (16 << 10)
    files["table.txt"] = table
    files["table.gz"] = gzip_member(table)
    files["table_bgzf.gz"] = b"".join(bgzf_members(table, 5000))
    whole = files["beagle_b60000.gz"]
    files["bad_cut.gz"] = whole[:len(whole) // 2 + 777]
    flipped = bytearray(whole)
    flipped[len(whole) // 3] ^= 0x55
    files["bad_flip.gz"] = bytes(flipped)
    files["bad_planted.gz"] = planted(text, 60000)
    rows = [header(["Ind%d" % i for i in range(N_IND)])] + [line(s) for s in range(40)]
    rows[18] = rows[18].rsplit("\t", 4)[0]                   # data line 19 of the file: one value of its last individual
    files["bad_short.gz"] = gzip_member(("\n".join(rows) + "\n").encode())
    for name, data in sorted(files.items()):
        with open(os.path.join(HERE, name), "wb") as fh:
            fh.write(data)
        print("%-20s %8d bytes" % (name, len(data)))


if __name__ == "__main__":
    main()
