"""The hand-built deflate streams the device inflate is held to, shared by tests/test_deflate_build_cpu.py (zlib agrees with
every expectation; what each family covers, counted from its inputs) and tests/test_gpu_inflate_streams.py (the kernel).

Every family returns (cases, cover): cases = [(stream, isize, expected bytes | None, label)] -- None: a stream that must be
refused -- and cover = what the family's inputs contain.  No data byte is 0: the output buffer starts as zeros, so a byte
that was never written, or written where it does not belong, shows.  64 consecutive cases of a launch are one wavefront."""
import functools
import itertools
import struct
import zlib

import numpy as np

import deflate_build as db
from deflate_build import Deflate

A_NEAR = tuple(range(1, 81))
A_FAR = (255, 256, 257, 4095, 4096, 4097, 32767, 32768)
A_FAR_LENGTHS = tuple(range(3, 21)) + (31, 32, 33, 34, 47, 48, 49, 50, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258)
A_BACK_TO_BACK = (3, 4, 5, 15, 16, 17, 33, 64, 65, 258, 3)
# (L1, L2, d2): a match of L1 bytes directly followed by one of L2 bytes from d2 <= L1 back -- its source is the tail of the first,
# whose last piece has been requested and not yet stored when the second is requested
A_PENDING = ((20, 18, 5), (9, 30, 1), (3, 17, 3), (40, 30, 20), (17, 40, 16), (100, 70, 64), (258, 258, 65), (33, 100, 15), (16, 16, 16), (64, 64, 64))
B_DISTANCES = (1, 2, 7, 9, 15, 16, 17, 63, 64, 65, 300)
B_LENGTHS = (3, 15, 16, 17, 32, 33, 48, 49, 64, 65, 258)
B_TAILS = tuple(range(81))
C_MIXES = (1, 3, 11, 12, 16, 63, 64)
C_ISIZE = 6000


def _bytes(rng, n, lo=1, hi=256):
    return bytes(rng.integers(lo, hi, size=n, dtype=np.uint8))


@functools.lru_cache(None)
def beagle_text(n=65536, seed=11):
    rng = np.random.default_rng(seed)
    v = rng.random(n // 8)
    v[rng.random(v.size) < 0.35] = 1 / 3
    return ("\t".join("%.6f" % x for x in v) + "\n").encode()[:n]


# ---- A: match geometry -- every distance 1..80 and the far ones, every length, every output phase
def a_body(d, rng):
    tokens = []
    for length in (range(3, 259) if d <= 80 else A_FAR_LENGTHS):
        tokens += list(_bytes(rng, 1 + length % 3))
        tokens.append((length, d))
    tokens += [(length, d) for length in A_BACK_TO_BACK] + list(_bytes(rng, 2))
    for l1, l2, d2 in A_PENDING:
        tokens += [(l1, d), (l2, d2), int(rng.integers(1, 256))]
    return tokens


@functools.lru_cache(None)
def family_a():
    cases, cover = [], {"pairs": set(), "phases": set(), "back_to_back": set(), "pending": set()}
    extra = _bytes(np.random.default_rng(100), 15)
    for d in A_NEAR + A_FAR:
        rng = np.random.default_rng(1000 + d)
        prefix, body = _bytes(rng, d), a_body(d, rng)
        cover["pairs"] |= {t for t in body if isinstance(t, tuple) and t[1] == d}
        for t, u in zip(body, body[1:]):
            if isinstance(t, tuple) and isinstance(u, tuple):
                cover["back_to_back"].add(d)
                if u[1] <= t[0]:
                    cover["pending"].add((d,) + u)
        for phase in range(16):
            w = Deflate()
            if d <= 80:
                base = db.expand(list(prefix) + body)
                w.raw_bits(3, 3).raw_bits(*db.encode_fixed(list(extra[:phase])))
                if phase == 0:
                    bits = db.encode_fixed(list(prefix) + body)
                w.raw_bits(*bits).raw_bits(*db.encode_fixed([db.EOB]))
            else:
                # the far distances become legal behind a stored block of filler
                base = prefix + db.expand(body, prefix)
                if phase == 0:
                    bits = db.encode_fixed(body)
                w.stored(extra[:phase] + prefix, False).raw_bits(3, 3).raw_bits(*bits).raw_bits(*db.encode_fixed([db.EOB]))
            expected = extra[:phase] + base
            cover["phases"].add((d, len(expected) % 16))
            cases.append((w.getvalue(), len(expected), expected, "A dist=%d phase=%d" % (d, phase)))
    return cases, cover


# ---- B: member tails -- a match, S literals, the end of the member
@functools.lru_cache(None)
def family_b():
    cases, cover = [], set()
    tail = _bytes(np.random.default_rng(200), 80)
    tails = [db.encode_fixed(list(tail[:s])) for s in B_TAILS]
    eob = db.encode_fixed([db.EOB])
    for d in B_DISTANCES:
        for length in B_LENGTHS:
            rng = np.random.default_rng(2000 + 300 * d + length)
            head = list(_bytes(rng, d + (3 * d + length) % 16)) + [(length, d)]
            bits, text = db.encode_fixed(head), db.expand(head)
            for s in B_TAILS:
                w = Deflate().raw_bits(3, 3).raw_bits(*bits).raw_bits(*tails[s]).raw_bits(*eob)
                cover.add((d, length, s))
                cases.append((w.getvalue(), len(text) + s, text + tail[:s], "B dist=%d len=%d tail=%d" % (d, length, s)))
    return cases, cover


# ---- C: codes beyond the 8- and 7-bit tables, and who else is in the wavefront
HEAVY_SHORT_LITS = (0x41, 0x42, 0x43, 0x44)                            # 3 bits each
HEAVY_LONG_LITS = {n: (0x61 + 2 * (n - 9), 0x62 + 2 * (n - 9)) for n in range(9, 16)}
HEAVY_LEN_SYMS = {4: 258, 5: 270, 9: 257, 10: 262, 11: 266, 12: 271, 13: 276, 14: 281, 15: 285}
HEAVY_DIST_SYMS = {2: 3, 3: 12, 8: 0, 9: 2, 10: 5, 11: 8, 12: 10, 13: 13, 14: 17, 15: 20}


@functools.lru_cache(None)
def heavy_codes():
    """Forced code lengths: used literals and length symbols at every length 9..15, distance symbols at 8..15, end-of-block
    at 15 bits; the space left over goes to symbols no token uses."""
    lit, dist = [0] * 286, [0] * 30
    for s in HEAVY_SHORT_LITS:
        lit[s] = 3
    for n, pair in HEAVY_LONG_LITS.items():
        lit[pair[0]] = lit[pair[1]] = n
    for n, s in HEAVY_LEN_SYMS.items():
        lit[s] = n
    lit[db.EOB] = 15
    for n, s in HEAVY_DIST_SYMS.items():
        dist[s] = n
    dist[6] = 2
    return (tuple(db.complete(lit, 15, pad_symbols=range(1, 0x41))),
            tuple(db.complete(dist, 15, pad_symbols=[s for s in range(30) if not dist[s]])))


def heavy_tokens(seed, isize, prefix=1600):
    """Tokens over the symbols heavy_codes() forces, most of them with long codes, expanding to exactly isize bytes; among them a
    15-bit length code directly followed by a 15-bit distance code, and a long code as the last symbol before the end-of-block."""
    rng = np.random.default_rng(seed)
    lits = list(HEAVY_SHORT_LITS) + [b for pair in HEAVY_LONG_LITS.values() for b in pair] * 3
    len_syms = [s for s in HEAVY_LEN_SYMS.values()]
    dist_syms = [3, 6] + list(HEAVY_DIST_SYMS.values())
    tokens = [lits[i] for i in rng.integers(0, len(lits), size=min(prefix, isize))]
    pos = len(tokens)
    while pos + 600 < isize:
        if rng.random() < 0.5:
            tokens.append(lits[int(rng.integers(0, len(lits)))])
            pos += 1
            continue
        i = len_syms[int(rng.integers(0, len(len_syms)))] - 257
        length = db.LEN_BASE[i] + int(rng.integers(0, 1 << db.LEN_EXTRA[i]))
        j = dist_syms[int(rng.integers(0, len(dist_syms)))]
        dist = db.DIST_BASE[j] + int(rng.integers(0, 1 << db.DIST_EXTRA[j]))
        if dist <= pos:
            tokens.append((length, dist))
            pos += length
    if isize - pos >= 264 and pos >= 1536:
        tokens.append((258, 1025 + int(rng.integers(0, 512))))         # symbol 285 and distance symbol 20: 15 bits each
        pos += 258
    last = isize - pos >= 3 and pos >= 1536
    while pos < isize - (3 if last else 0):
        tokens.append(lits[int(rng.integers(4, len(lits)))])
        pos += 1
    if last:
        tokens.append((3, 1536))
    return tokens


@functools.lru_cache(None)
def heavy_pair(seed, isize=C_ISIZE):
    """(long-code stream, short-code stream, expected bytes, tokens) of one token list: forced lengths / the fixed code."""
    tokens = heavy_tokens(seed, isize)
    lit, dist = heavy_codes()
    text = db.expand(tokens)
    assert len(text) == isize
    return (Deflate().dynamic(tokens, True, lit_lens=lit, dist_lens=dist).getvalue(), Deflate().fixed(tokens, True).getvalue(), text, tokens)


def c_heavy_lanes(k):
    return {(j * 64) // k for j in range(k)}


@functools.lru_cache(None)
def family_c():
    """cases: a dict of launches."""
    launches, cover = {}, {"mixes": {}, "launch_sizes": set()}

    def member(i, heavy, tag):
        h, s, text, _ = heavy_pair(i % 8)
        return (h if heavy else s, len(text), text, "C %s lane=%d %s seed=%d" % (tag, i, "long" if heavy else "short", i % 8))

    mixes = []
    for k in C_MIXES:
        lanes = c_heavy_lanes(k)
        cover["mixes"][k] = len(lanes)
        mixes += [member(i, i in lanes, "mix=%d" % k) for i in range(64)]
    launches["mixes"] = mixes
    launches["one"] = [member(0, True, "alone")]
    launches["65"] = [member(i, i % 2 == 0, "of65") for i in range(65)]
    launches["127"] = [member(i, i % 3 != 0, "of127") for i in range(127)]
    # one wavefront whose members' ISIZE runs from 0 to 65536: lanes retire throughout
    text = beagle_text()
    tokens = db.tokenize(text)
    ends = np.cumsum([t[0] if isinstance(t, tuple) else 1 for t in tokens])
    retire = [(bytes([3, 0]), 0, b"", "C retire isize=0 (the BGZF EOF member)"), (bytes([1, 0, 0, 0xFF, 0xFF]), 0, b"", "C retire isize=0 stored"),
              (Deflate().dynamic([], True).getvalue(), 0, b"", "C retire isize=0 dynamic")]
    sizes = sorted({int(65536 * (i / 60) ** 2.5) for i in range(1, 61)} | {1, 2, 3})
    sizes = sizes[:1] + sizes[-60:]
    lit, dist = heavy_codes()
    for i, n in enumerate(sizes):
        if i % 3 == 2 and n >= 2000:
            toks = heavy_tokens(50 + i, n)
            stream, want = Deflate().dynamic(toks, True, lit_lens=lit, dist_lens=dist).getvalue(), db.expand(toks)
        else:
            k = int(np.searchsorted(ends, n, side="right"))
            toks = tokens[:k] + list(text[(int(ends[k - 1]) if k else 0):n])
            want = text[:n]
            stream = (Deflate().dynamic(toks, True) if i % 3 == 0 else Deflate().fixed(toks, True)).getvalue()
        retire.append((stream, n, want, "C retire isize=%d" % n))
    assert len(retire) == 64 and retire[-1][1] == 65536
    launches["retire"] = retire
    cover["retire_sizes"] = [c[1] for c in retire]
    cover["launch_sizes"] = {len(v) for v in launches.values()}
    cover["used"] = db.used_code_lengths([t for s in range(8) for t in heavy_pair(s)[3]], lit, dist)
    return launches, cover


# ---- D: matches of 48 bits, back to back
@functools.lru_cache(None)
def d_codes():
    lit, dist = [0] * 286, [0] * 30
    for s in HEAVY_SHORT_LITS:
        lit[s] = 3
    lit[db.EOB] = 4
    for s in (281, 282, 283, 284):
        lit[s] = 15
    for s in (26, 27, 28, 29):
        dist[s] = 15
    return tuple(db.complete(lit, 15, pad_symbols=range(1, 0x41))), tuple(db.complete(dist, 15, pad_symbols=range(26)))


@functools.lru_cache(None)
def filler(n=32768):
    return _bytes(np.random.default_rng(400), n)


@functools.lru_cache(None)
def family_d():
    cases, cover = [], {"phases_48": set(), "extras": set(), "syms": set()}
    lit, dist = d_codes()
    for mode in ("zeros", "ones", "random"):
        for lead in range(8):
            rng = np.random.default_rng(4000 + lead)
            tokens = [HEAVY_SHORT_LITS[i % 4] for i in range(lead)]
            pos, k = 32768 + lead, 0
            while pos + 258 <= 65536 - 8:
                ls = 281 + int(rng.integers(0, 4))
                ds = (28 + int(rng.integers(0, 2))) if k % 4 != 3 else (26 + int(rng.integers(0, 2)))       # 13 / 12 extra bits
                lx = {"zeros": 0, "ones": 31, "random": int(rng.integers(0, 32))}[mode]
                dx = {"zeros": 0, "ones": (1 << db.DIST_EXTRA[ds]) - 1, "random": int(rng.integers(0, 1 << db.DIST_EXTRA[ds]))}[mode]
                tokens.append((db.LEN_BASE[ls - 257] + lx, db.DIST_BASE[ds] + dx))
                cover["syms"] |= {ls, ds}
                cover["extras"].add((mode, lx == 31, dx == 8191))
                pos += tokens[-1][0]
                k += 1
            trace = []
            w = Deflate().stored(filler(), False).dynamic(tokens, True, lit_lens=lit, dist_lens=dist, long258=True, trace=trace)
            cover["phases_48"] |= {b % 8 for b, n in trace if n == 48}
            text = filler() + db.expand(tokens, filler())
            cases.append((w.getvalue(), len(text), text, "D extras=%s lead=%d" % (mode, lead)))
    return cases, cover


# ---- E: block structure and headers
def _split(tokens, n):
    cut = [len(tokens) * i // n for i in range(n + 1)]
    return [tokens[a:b] for a, b in zip(cut, cut[1:])]


def member_of_blocks(tokens, kinds, empties=()):
    """One stream of len(kinds) blocks (0 stored, 1 fixed, 2 dynamic) that share the tokens; empties: (index, kind) of empty
    blocks put in front of block `index`."""
    w, done = Deflate(), b""
    parts = _split(tokens, len(kinds))
    for i, (kind, part) in enumerate(zip(kinds, parts)):
        for at, ek in empties:
            if at == i:
                (w.stored(b"", False) if ek == 0 else w.fixed([], False) if ek == 1 else w.dynamic([], False))
        final = i == len(kinds) - 1
        text = db.expand(part, done)
        if kind == 0:
            w.stored(text, final)
        elif kind == 1:
            w.fixed(part, final)
        else:
            w.dynamic(part, final)
        done += text
    return w, done


MAXIMAL_LIT_LENS = [0] * 10 + [4] * 7 + [0] * 138 + [2, 3, 3] + [0] * 98 + [6] + [0] * 20 + [6, 6, 6]        # 280 symbols
MAXIMAL_DIST_LENS = [6, 6, 6, 6, 1, 2, 3, 4]


def maximal_tokens(seed=5):
    rng = np.random.default_rng(seed)
    lits = list(range(10, 17)) + [155, 156, 157]
    tokens = [lits[i] for i in rng.integers(0, len(lits), size=40)]
    for _ in range(60):
        tokens.append((int(rng.integers(67, 115)), int(rng.integers(1, 17))))
        tokens.append(lits[int(rng.integers(0, len(lits)))])
    return tokens


@functools.lru_cache(None)
def family_e():
    cases, cover = [], {"orders": set(), "stored_phase": set(), "len_at": set(), "empties": set(), "hlit": set(), "hdist": set(), "hclen": set(),
                        "clen_max": 0, "repeats": set(), "across": False, "flushes": set(), "dist_single": set()}
    text = beagle_text(3000, seed=12)
    tokens = db.tokenize(text)

    def add(w, want, label):
        cases.append((w.getvalue(), len(want), want, "E " + label))
        for b in w.blocks:
            if b["type"] == 2:
                cover["hlit"].add(b["hlit"]), cover["hdist"].add(b["hdist"]), cover["hclen"].add(b["hclen"])
                cover["clen_max"] = max(cover["clen_max"], max(b["clen_lens"]))
        return w

    # members of 2..40 blocks in every order of the three types (every order of two and three, then longer ones)
    rng = np.random.default_rng(500)
    orders = [k for n in (2, 3) for k in itertools.product((0, 1, 2), repeat=n)] + [tuple(int(x) for x in rng.integers(0, 3, size=n)) for n in range(4, 41)]
    for kinds in orders:
        w, want = member_of_blocks(tokens, kinds)
        assert want == text
        cover["orders"].add(kinds)
        add(w, want, "blocks=" + "".join("SFD"[k] for k in kinds))
    # a stored block behind a compressed one at each of the eight bit phases (j literals of nine bits move it)
    for j in range(8):
        lits = [200 + i for i in range(j)] + [65, 66]
        for kind in (1, 2):
            w = Deflate()
            (w.fixed(lits, False) if kind == 1 else w.dynamic(lits, False))
            w.stored(text[:100], True)
            if kind == 1:
                cover["stored_phase"].add(w.blocks[1]["bit"] % 8)
            add(w, bytes(lits) + text[:100], "stored behind %s at bit %d" % ("FD"[kind - 1], w.blocks[1]["bit"] % 8))
    # empty blocks of every type in the middle of a member, in front and at the end
    for ek in (0, 1, 2):
        for at in (0, 1, 2):
            w, want = member_of_blocks(tokens, (2, 1, 0, 2), empties=((at, ek), (at + 1, ek)))
            cover["empties"].add((ek, at))
            add(w, want, "empty %s before block %d and %d" % ("SFD"[ek], at, at + 1))
        w = Deflate().dynamic(tokens, False)
        (w.stored(b"", True) if ek == 0 else w.fixed([], True) if ek == 1 else w.dynamic([], True))
        add(w, text, "empty final %s" % "SFD"[ek])
    # LEN / NLEN at every byte of an eight-byte input word
    for n in range(8):
        w = Deflate().stored(text[:n], False).stored(text[n:40], False).fixed(tokens, True)
        cover["len_at"].add(w.blocks[1]["len_at_byte"] % 8)
        add(w, text[:40] + text, "LEN at byte %d" % w.blocks[1]["len_at_byte"])
    # the largest stored block, in a member of 65536 bytes
    big = beagle_text()
    add(Deflate().stored(big[:65535], False).stored(big[65535:], True), big, "stored 65535+1")
    add(Deflate().stored(big[:1], False).stored(big[1:], True), big, "stored 1+65535")
    add(Deflate().fixed([big[0]], False).stored(big[1:], True), big, "fixed 1 + stored 65535")
    # header shapes
    lits = [t for t in tokens if not isinstance(t, tuple)]
    w = add(Deflate().dynamic(lits, True), bytes(lits), "HLIT 257, HDIST 1 without a distance code")
    assert w.blocks[0]["hlit"] == 257 and w.blocks[0]["dist_lens"] == [0]
    cover["dist_single"].add(0)
    t286 = lits[:20] + [(258, 5), (258, 7)] + lits[20:40]
    w = add(Deflate().dynamic(t286, True), db.expand(t286), "HLIT 286")
    assert w.blocks[0]["hlit"] == 286
    t1 = lits[:5] + [(30, 1), 66, (3, 1), (258, 1)]
    w = add(Deflate().dynamic(t1, True), db.expand(t1), "HDIST 1 with the single one-bit distance code")
    assert w.blocks[0]["dist_lens"] == [1]
    cover["dist_single"].add(1)
    t30 = lits[:30] + [(40, 32768), (100, 24577), (5, 3)]
    w = add(Deflate().stored(filler(), False).dynamic(t30, True), filler() + db.expand(t30, filler()), "HDIST 30")
    assert w.blocks[1]["hdist"] == 30
    hl, hd = heavy_codes()
    ht = heavy_tokens(77, 4000)
    w = add(Deflate().dynamic(ht, True, lit_lens=hl, dist_lens=hd), db.expand(ht), "HCLEN 19")
    assert w.blocks[0]["hclen"] == 19
    l5 = list(range(1, 256)) * 2
    w = add(Deflate().dynamic(l5, True, lit_lens=[0] + [8] * 256, dist_lens=[0]), bytes(l5), "HCLEN 5 (the fewest a valid block can have)")
    assert w.blocks[0]["hclen"] == 5
    # a code-length code of seven bits: frequencies that make the code a chain
    probe = Deflate().dynamic(ht, True, lit_lens=hl, dist_lens=hd)
    used = sorted({s for _, s, _, _, _ in probe.blocks[0]["runs"]})
    chain = [0] * 19
    for rank, s in enumerate(used):
        chain[s] = 1 << rank
    cl7 = db.huffman_lengths(chain, 7)
    w = add(Deflate().dynamic(ht, True, lit_lens=hl, dist_lens=hd, clen_lens=cl7), db.expand(ht), "code-length code of 7 bits")
    assert max(cl7) == 7 and all(cl7[s] for s in used)
    # the longest repeats (16: 6, 17: 10, 18: 138), and a 16-run that goes on from the literal lengths into the distance lengths
    mt = maximal_tokens()
    w = add(Deflate().dynamic(mt, True, lit_lens=MAXIMAL_LIT_LENS, dist_lens=MAXIMAL_DIST_LENS), db.expand(mt), "maximal repeats, run across HLIT")
    for i, s, xb, xv, n in w.blocks[0]["runs"]:
        if s >= 16:
            cover["repeats"].add((s, n))
            cover["across"] |= s == 16 and i < len(MAXIMAL_LIT_LENS) < i + n
    add(Deflate().dynamic(mt, True, lit_lens=MAXIMAL_LIT_LENS, dist_lens=MAXIMAL_DIST_LENS, across=False), db.expand(mt), "same lengths, no run across HLIT")
    add(Deflate().dynamic(mt, True, lit_lens=MAXIMAL_LIT_LENS, dist_lens=MAXIMAL_DIST_LENS, maximal=False), db.expand(mt), "same lengths, no repeats")
    # one token list in the fixed code and in three dynamic code sets: the same bytes
    want = db.expand(ht)
    add(Deflate().fixed(ht, True), want, "one token list: fixed")
    add(Deflate().dynamic(ht, True), want, "one token list: dynamic, lengths from the frequencies")
    add(Deflate().dynamic(ht, True, lit_lens=hl, dist_lens=hd), want, "one token list: dynamic, long codes")
    ht_lits = {t for t in ht if not isinstance(t, tuple)}
    flat = db.complete([7 if s in ht_lits or s >= 256 else 0 for s in range(286)], 15, pad_symbols=range(1, 0x41))
    add(Deflate().dynamic(ht, True, lit_lens=flat, dist_lens=[5] * 24 + [4] * 4), want, "one token list: dynamic, flat lengths")
    # zlib's own flushes: an empty stored block (sync, full) or an empty fixed block (partial) mid-member
    for name, mode in (("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH), ("partial", zlib.Z_PARTIAL_FLUSH)):
        for level in (1, 6):
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            s = b"".join(co.compress(text[i:i + 700]) + co.flush(mode) for i in range(0, 2800, 700)) + co.compress(text[2800:]) + co.flush()
            cover["flushes"].add(name)
            cases.append((s, len(text), text, "E zlib level %d with %s flushes" % (level, name)))
    return cases, cover


# ---- N: streams the device must refuse (each a valid stream with ONE defect), between valid neighbours
@functools.lru_cache(None)
def family_n():
    text = beagle_text(1200, seed=13)
    tokens = db.tokenize(text)
    good = (Deflate().dynamic(tokens, True).getvalue(), len(text), text, "N valid neighbour")
    bad = []

    def refuse(stream, isize, label):
        bad.append((stream if isinstance(stream, bytes) else stream.getvalue(), isize, None, "N " + label))

    lits = list(text[:10])
    refuse(Deflate().fixed(lits + [(5, 11)] + list(text[:20]), True), 35, "distance = pos + 1")
    refuse(Deflate().fixed(lits + [(20, 3)], True), 29, "match overruns ISIZE by one byte")
    refuse(Deflate().dynamic(tokens + [65], True), len(text), "literal overruns ISIZE by one byte")
    refuse(Deflate().fixed(tokens[:50], False).stored(text[:31], True), len(db.expand(tokens[:50])) + 30, "stored block overruns ISIZE by one byte")
    refuse(Deflate().dynamic(tokens, True), len(text) + 1, "stream one byte short of ISIZE")
    refuse(Deflate().stored(text[:30], True), 31, "stored stream one byte short of ISIZE")
    fixed_lit, fixed_dist = db.canonical(db.FIXED_LIT_LENS), db.canonical(db.FIXED_DIST_LENS)
    for sym in (286, 287):
        w = Deflate().raw_bits(3, 3).raw_bits(*db.encode_fixed(lits)).raw_bits(*fixed_lit[sym]).raw_bits(*db.encode_fixed(lits + [db.EOB]))
        refuse(w, 20, "symbol %d in a fixed block" % sym)
    for sym in (30, 31):
        w = Deflate().raw_bits(3, 3).raw_bits(*db.encode_fixed(lits)).raw_bits(*fixed_lit[257]).raw_bits(*fixed_dist[sym]).raw_bits(0, 13)
        w.raw_bits(*db.encode_fixed(lits + [db.EOB]))
        refuse(w, 23, "distance symbol %d in a fixed block" % sym)
    base = Deflate().dynamic(tokens, True).blocks[0]
    lit_lens, dist_lens = base["lit_lens"], base["dist_lens"]
    over = list(lit_lens)
    over[max(range(len(over)), key=lambda s: over[s])] -= 1
    refuse(Deflate().dynamic(tokens, True, lit_lens=over, dist_lens=dist_lens), len(text), "over-subscribed literal/length set")
    over = list(dist_lens)
    over[max(range(len(over)), key=lambda s: over[s])] -= 1
    refuse(Deflate().dynamic(tokens, True, lit_lens=lit_lens, dist_lens=over), len(text), "over-subscribed distance set")
    over = list(base["clen_lens"])
    over[max(range(19), key=lambda s: over[s])] -= 1
    refuse(Deflate().dynamic(tokens, True, lit_lens=lit_lens, dist_lens=dist_lens, clen_lens=over), len(text), "over-subscribed code-length set")
    noeob = list(lit_lens)
    spare = next(s for s in range(1, 256) if not noeob[s])
    noeob[spare], noeob[db.EOB] = noeob[db.EOB], 0
    refuse(Deflate().dynamic(tokens, True, lit_lens=noeob, dist_lens=dist_lens, eob=False), len(text), "no end-of-block code")
    runs = [(s, xb, xv) for _, s, xb, xv, _ in base["runs"]]
    refuse(Deflate().dynamic(tokens, True, lit_lens=lit_lens, dist_lens=dist_lens, clen_tokens=[(16, 2, 0)] + runs[1:]), len(text), "symbol 16 first")
    refuse(Deflate().dynamic(tokens, True, lit_lens=lit_lens, dist_lens=dist_lens, clen_tokens=runs[:-1] + [(18, 7, 127)]), len(text),
           "repeat past HLIT + HDIST")
    l287 = list(lit_lens) + [0] * (287 - len(lit_lens))
    refuse(Deflate().dynamic(tokens, True, lit_lens=l287, dist_lens=dist_lens), len(text), "HLIT 287")
    refuse(Deflate().stored(text[:50], True, nlen=(50 ^ 0xFFFF) ^ 0x100), 50, "NLEN wrong")
    refuse(Deflate().raw_bits(1, 1).raw_bits(3, 2).raw_bits(*db.encode_fixed(lits + [db.EOB])), 10, "block type 3")
    w = Deflate().dynamic(tokens, True)
    s = w.getvalue()
    refuse(s[:w.blocks[0]["header_bits"] // 16], len(text), "cut inside the header")
    # nine-bit literals from bit 3 on: byte 5 ends inside the code that covers bits 39..47
    nine = [200 + i for i in range(40)]
    refuse(Deflate().fixed(nine, True).getvalue()[:5], 40, "cut inside a code")
    # ten literals of 8 bits, the length code (7 bits) and the distance code (5 bits) end at bit 3 + 80 + 12 = 95 of the block: the
    # 13 extra bits of the distance are cut at bit 96
    w = Deflate().stored(filler(), False)
    at = w.bit_position()
    w.fixed(lits + [(3, 32768)], True)
    refuse(w.getvalue()[:(at + 3 + 80 + 7 + 5 + 6) // 8], 32768 + 13, "cut inside the extra bits")
    cases = [good]
    for b in bad:
        cases += [b, good]
    return cases, {"defects": [b[3][2:] for b in bad]}


@functools.lru_cache(None)
def family_n_unusable_header():
    """HCLEN 4 gives lengths to the code-length symbols 16, 17, 18 and 0 only, so every code length of the block is 0 and there
    is no end-of-block code: no valid block has HCLEN 4 (the fewest is 5, family E)."""
    clen = [0] * 19
    clen[18], clen[0] = 1, 1
    w = Deflate().dynamic([], True, lit_lens=[0] * 257, dist_lens=[0], clen_lens=clen, eob=False)
    assert w.blocks[0]["hclen"] == 4
    return [(w.getvalue() + bytes(8), 0, None, "N HCLEN 4")]


@functools.lru_cache(None)
def family_incomplete():
    """Incomplete code sets (zlib refuses them at the header; the device may refuse them, or decode -- every code the tokens use
    exists): [(stream, isize, expand(tokens), label)]."""
    text = beagle_text(1200, seed=13)
    tokens = db.tokenize(text)
    base = Deflate().dynamic(tokens, True).blocks[0]
    lit = list(base["lit_lens"])
    s = min((s for s in range(len(lit)) if lit[s]), key=lambda s: lit[s])
    lit[s] += 1
    t3 = list(text[:40]) + [(10, 1), 66, (12, 2), 67, (9, 3), 68]
    return [(Deflate().dynamic(tokens, True, lit_lens=lit, dist_lens=base["dist_lens"]).getvalue(), len(text), text, "incomplete literal/length set"),
            (Deflate().dynamic(t3, True, dist_lens=[2, 2, 2]).getvalue(), len(db.expand(t3)), db.expand(t3), "incomplete distance set of three codes")]


# ---- F: a Beagle file whose members are hand-built streams
def beagle_body(sites=300, individuals=20, seed=14):
    rng = np.random.default_rng(seed)
    head = "marker\tallele1\tallele2\t" + "\t".join("I%d\tI%d\tI%d" % (i, i, i) for i in range(individuals)) + "\n"
    lines = [head]
    for s in range(sites):
        a = rng.random(individuals)
        b = rng.random(individuals) * (1 - a)
        miss = rng.random(individuals) < 0.35
        vals = np.stack([np.where(miss, 1 / 3, a), np.where(miss, 1 / 3, b), np.where(miss, 1 / 3, 1 - a - b)], axis=1).reshape(-1)
        lines.append("chr2_%d\tA\tG\t" % (1000 + 37 * s) + "\t".join("%.6f" % v for v in vals) + "\n")
    return "".join(lines).encode()


def bgzf_member(stream, chunk):
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(stream) + 8 - 1) +
            stream + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))


F_SITES, F_INDIVIDUALS, F_BUILT_BYTES = 2600, 20, 165_000


def family_f(member_bytes=7919):
    """(file bytes, the hand-built members' streams as cases, the text).  The reader inflates the first MiB of text on the host
    while it reads the header, so the file begins with 1.2 MiB in zlib's members; the last F_BUILT_BYTES (300 sites) are cut every
    member_bytes bytes (mid-line, mid-number), each member 2..4 blocks of mixed type around an empty stored block and a stored block."""
    body = beagle_body(F_SITES, F_INDIVIDUALS)
    first = len(body) - F_BUILT_BYTES
    out, cases = [], []
    for at in range(0, first, 60000):
        chunk = body[at:min(at + 60000, first)]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        out.append(bgzf_member(co.compress(chunk) + co.flush(), chunk))
    for k, at in enumerate(range(first, len(body), member_bytes)):
        chunk = body[at:at + member_bytes]
        tokens = db.tokenize(chunk)
        parts = _split(tokens, 2 + k % 3)
        w, done = Deflate(), b""
        for i, part in enumerate(parts):
            text = db.expand(part, done)
            final = i == len(parts) - 1
            if i == 1:
                w.stored(b"", False).stored(text, final)
            elif (i + k) % 2:
                w.fixed(part, final)
            else:
                w.dynamic(part, final)
            done += text
        assert done == chunk
        cases.append((w.getvalue(), len(chunk), chunk, "F member %d" % k))
        out.append(bgzf_member(w.getvalue(), chunk))
    out.append(bgzf_member(bytes([3, 0]), b""))
    return b"".join(out), cases, body
