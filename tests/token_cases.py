"""What the device tokenisers (csrc/ingest.hip: tokenise_kernel / parse_token, depth_tokenise_kernel) must compute, stated
without a GPU and without the library: the value of a token (`atof32`), the grammar the device converts itself
(`device_takes`, `depth_takes`), the tokens that probe both (ties, the whole grammar, byte substitutions, ...), the files
that carry them, and what a file covers of the wave-level machinery, counted from its text.

`device_takes` restates the comment at the head of ingest.hip, not the kernel's code path: the two must change together.

Test infrastructure (NumPy and the standard library only)."""
import itertools
import random
import re

import numpy as np

DELIMS = b"\t \n\r"                                   # reader.cpp: is_delim
STEP = 1024                                           # bytes a wavefront takes per step: 64 lanes x 16-byte words
STRIP = 256                                           # individuals per strip of depth_tokenise_kernel

# ---------------------------------------------------------------- the value of a token: atof, then (float)
_DEC = re.compile(rb"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?")
_HEX = re.compile(rb"([+-]?)0[xX]((?:[0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)(?:[pP][+-]?[0-9]+)?)")
_WORD = re.compile(rb"([+-]?)(infinity|inf|nan)", re.IGNORECASE)


def atof(token):
    """C's atof in the C locale on a token that holds no Beagle delimiter: the longest prefix that is a number, 0.0 where there
    is none.  Bytes, not str: str.isdigit and float() know digits and separators that C does not."""
    t = bytes(token).lstrip(b"\v\f")                  # white space to atof, no delimiter to the readers
    m = _HEX.match(t)
    if m:
        try:
            v = float.fromhex("0x" + m.group(2).decode("ascii"))
        except OverflowError:
            v = float("inf")
        return -v if m.group(1) == b"-" else v
    m = _WORD.match(t)
    if m:
        v = float("nan") if m.group(2).lower() == b"nan" else float("inf")
        return -v if m.group(1) == b"-" else v
    m = _DEC.match(t)
    return float(m.group().decode("ascii")) if m else 0.0


def atof32(token):
    with np.errstate(over="ignore"):
        return np.float32(atof(token))


def atof32_many(tokens):
    with np.errstate(over="ignore"):
        return np.array([atof(t) for t in tokens], dtype=np.float64).astype(np.float32)


# ---------------------------------------------------------------- the grammar the device converts itself
_TAKEN = re.compile(rb"[+-]?([0-9]*)\.?([0-9]*)(?:[eE]([+-]?[0-9]{1,3}))?")


def device_takes(token):
    """At most 16 bytes: an optional sign, digits with at most one point and at least one digit, at most 15 significant digits
    (from the first non-zero digit on, trailing zeros included), an optional e/E exponent of an optional sign and 1..3 digits,
    exponent minus digits behind the point within +-22, and nothing behind."""
    token = bytes(token)
    if not 1 <= len(token) <= 16:
        return False
    m = _TAKEN.fullmatch(token)
    if not m:
        return False
    whole, frac, ex = m.groups()
    if not whole and not frac:
        return False
    if len((whole + frac).lstrip(b"0")) > 15:
        return False
    return -22 <= int(ex or 0) - len(frac) <= 22


def depth_takes(token):
    """depth_tokenise_kernel: runs of one to three digits with a value of at most 255."""
    token = bytes(token)
    return 1 <= len(token) <= 3 and token.isdigit() and int(token) <= 255


# ---------------------------------------------------------------- tokens
_M = 1 << 23
TIE_MANTISSAS = (_M, _M + 1, _M + 2, 2 * _M - 2, 2 * _M - 1, _M + _M // 2, 0xAAAAAA, 0xD55555, 0x9E3779)


def _decimal(digits, f):
    """The integer `digits` with its last f digits behind the point."""
    s = str(digits)
    if f == 0:
        return s
    s = s.rjust(f + 1, "0")
    return s[:-f] + "." + s[-f:]


def _fits(text):
    return len(text) <= 16 and len(text.replace(".", "").lstrip("0")) <= 15


def tie_triples():
    """(below, tie, above, lower mantissa, binary exponent k) with tie = (2 mantissa + 1) 2^k exactly, the midpoint of the float32
    values mantissa 2^(k+1) and (mantissa + 1) 2^(k+1): every k at which the midpoint's decimal expansion has at most 15
    significant digits and fits 16 bytes.  below and above differ from it by one unit of the last decimal place that still fits."""
    out = []
    for k in range(-60, 61):
        for mant in TIE_MANTISSAS:
            odd = 2 * mant + 1
            digits, f = (odd << k, 0) if k >= 0 else (odd * 5 ** -k, -k)
            if not _fits(_decimal(digits, f)):
                continue
            z = 0
            while _fits(_decimal(digits * 10 ** (z + 1), f + z + 1)) and _fits(_decimal(digits * 10 ** (z + 1) + 1, f + z + 1)):
                z += 1
            scaled = digits * 10 ** z
            out.append((_decimal(scaled - 1, f + z).encode(), _decimal(digits, f).encode(), _decimal(scaled + 1, f + z).encode(), mant, k))
    return out


def ties():
    """Every tie of tie_triples with its two neighbours, with both signs (a sign may take a token past 16 bytes: those are the
    host's)."""
    out = []
    for below, tie, above, _, _ in tie_triples():
        for t in (below, tie, above):
            out += [t, b"-" + t]
    return out


CONTRACT_EXTREMES = [b"9999999999999e22", b"9.99999999999e34", b"1e-22", b".000000001e-13", b"1e22", b"1E+022", b"1e-022", b"0", b"-0", b"+0",
                     b"000000000000000", b"0000000000000000", b"999999999999999", b"-99999999999999.", b".999999999999999", b"0.00000000000001",
                     b"0.99999999999999", b"-.5", b"5.", b"+5.e+1", b"1.e0", b"00000000001e-22", b"0.0000000000e-12"]


def contract_tokens(count, seed):
    """Random tokens of the accepted grammar: 1..15 digits with the point at every position (none, first .. last), signs, e and E,
    exponent digits zero-padded to 1..3, the net power of ten over the whole of +-22.  (16 bytes hold 13 digits in front of
    "e22": the values reach 10^35 upwards and 10^-22 downwards.)"""
    rnd = random.Random(seed)
    out = [t for t in CONTRACT_EXTREMES if device_takes(t)][:count]
    while len(out) < count:
        r = rnd.getrandbits(48)                       # one draw per token, taken apart
        r, nd = divmod(r, 15)
        nd += 1
        r, point = divmod(r, nd + 2)
        r, sign = divmod(r, 4)
        r, form = divmod(r, 3)
        r, net = divmod(r, 45)
        r, width = divmod(r, 3)
        r, big = divmod(r, 2)
        digits = "%0*d" % (nd, rnd.randrange(10 ** nd))
        frac = 0 if point == 0 else nd - point + 1    # point: 0 = none, 1 .. nd + 1 = in front of digit point - 1 .. behind the last
        tok = ("", "", "-", "+")[sign] + (digits if point == 0 else digits[:point - 1] + "." + digits[point - 1:])
        if form:
            ex = net - 22 + frac
            tok += "eE"[big] + ("-" if ex < 0 else ("", "+")[r % 2]) + "%0*d" % (width + 1, abs(ex))
        if len(tok) <= 16:
            out.append(tok.encode())
    return out


def grammar_tokens():
    """Every string of length 1..5 over 0 1 7 . - + e, and the same with E."""
    out = []
    for n in range(1, 6):
        for t in itertools.product(b"017.-+e", repeat=n):
            t = bytes(t)
            out.append(t)
            if b"e" in t:
                out.append(t.replace(b"e", b"E"))
    return out


SUBSTITUTION_BASES = (b"1.234567", b"9.000000")


def substituted():
    """Every byte 1..255 except the four delimiters at every position of two tokens of the SWAR path."""
    out = []
    for base in SUBSTITUTION_BASES:
        for pos in range(len(base)):
            for c in range(1, 256):
                if c not in DELIMS:
                    out.append(base[:pos] + bytes([c]) + base[pos + 1:])
    return out


def beyond_contract():
    """Tokens the device must leave to the host."""
    out = [b"1234567890123456", b"0.1234567890123456", b"1.234567890123456", b"-123456789.1234567",           # 16 significant digits
           b"1e23", b"1e-23", b"0.1e-22", b"10e23", b"1.5E+24", b".000001e-17",                                # net power +-23
           b"1e0001", b"1e+0022", b"1E-0001", b"1e", b"1e+", b"1e-", b"1E", b"1.5e+",                          # exponents
           b"nan", b"NaN", b"-nan", b"inf", b"-inf", b"+Inf", b"INFINITY", b"-infinity", b"infin",
           b"0x1p-2", b"0X1P-2", b"-0x1.8p1", b"0x.8", b"0x1p", b"0x", b"0x1p99999",
           b"1e400", b"-1e400", b"1e-46", b"1e-45", b"7e-46", b"1e39", b"3.5e38", b"1e-400",
           b"-0.0000000000000000", b"-0.000000000000000000000", b"-00000000000000000",                        # -0 written long
           b"0.00123456789012345", b"0000123456789012345", b"00000000.123456789012345",                        # 15 digits past 16 bytes
           b"0.5abc", b"1.2.3", b"--1", b"+-1", b"1,5", b"1_0", b".", b"-.", b"+", b"e5", b".e5", b"1e5.0", b"1\xb2", b"\xef\xbc\x91"]
    for n in range(17, 41):                                                                                    # 17..40 byte tokens
        out.append((b"0." + b"1234567890" * 4)[:n])
        out.append((b"1" + b"0" * 40)[:n])
    assert not any(device_takes(t) for t in out), [t for t in out if device_takes(t)]
    return out


def tokens_of_length(length, count, seed):
    """Random tokens of exactly `length` bytes: of the accepted grammar up to 16 bytes, plain decimals beyond."""
    rnd = random.Random(seed * 1000 + length)
    out = []
    while len(out) < count:
        sign = rnd.choice(("", "-")) if length >= 2 and rnd.randrange(3) == 0 else ""
        room = length - len(sign)
        if room >= 2 and (room > 15 or rnd.randrange(4)):
            point = rnd.randint(0, room - 1)
            digits = "".join(rnd.choices("0123456789", k=room - 1))
            tok = sign + digits[:point] + "." + digits[point:]
        else:
            tok = sign + "".join(rnd.choices("0123456789", k=room))
        tok = tok.encode()
        if device_takes(tok) == (length <= 16):
            out.append(tok)
    return out


# ---------------------------------------------------------------- files
def beagle_header(n, sep=b"\t", pad=0):
    """The header line of n individuals, its first name lengthened by `pad` bytes."""
    return sep.join([b"marker" + b"_" * pad, b"allele1", b"allele2"] + [b"I%d" % i for i in range(n) for _ in range(3)])


def beagle_line(name, kept, filler=b"0.333333", sep=b"\t", alleles=(b"A", b"C"), behind=()):
    """One data line: the 2n kept tokens of a row, the dropped third column filled from `filler` (one token, or a list taken in
    turns), `behind` = columns behind 3 + 3n."""
    fill = [filler] if isinstance(filler, bytes) else list(filler)
    cols = [name, alleles[0], alleles[1]]
    for i in range(len(kept) // 2):
        cols += [kept[2 * i], kept[2 * i + 1], fill[i % len(fill)]]
    return sep.join(cols + list(behind))


def expected_rows(rows):
    """The (m, 2n) float32 matrix of the rows' kept tokens, and the number of rows that hold a token the device does not take."""
    width = len(rows[0])
    flat = [t for r in rows for t in r]
    cache = {}
    for t in flat:
        if t not in cache:
            cache[t] = atof(t)
    with np.errstate(over="ignore"):
        want = np.array([cache[t] for t in flat], dtype=np.float64).astype(np.float32).reshape(len(rows), width)
    takes = {t: device_takes(t) for t in cache}
    return want, sum(1 for r in rows if not all(takes[t] for t in r))


def rows_of(tokens, n, pad=b"0"):
    """The tokens as rows of 2n.  Those the device takes fill rows of their own.  Every other token gets a row to itself, at a
    column that moves on from row to row, among tokens the device takes: the number of rows the host must parse is then the number
    of such tokens, and moves with every single token the device wrongly takes or wrongly leaves."""
    own = [t for t in tokens if device_takes(t)]
    other = [t for t in tokens if not device_takes(t)]
    fill = own or [pad]
    group = own + [pad] * (-len(own) % (2 * n))
    rows = [group[i:i + 2 * n] for i in range(0, len(group), 2 * n)]
    for j, t in enumerate(other):
        row = [fill[(j * 2 * n + c) % len(fill)] for c in range(2 * n)]
        row[j % (2 * n)] = t
        rows.append(row)
    return rows


def beagle_file(tokens, n, filler=b"0.333333", sep=b"\t", eol=b"\n", final_eol=True, header_pad=0):
    """(text, expected matrix, lines with a kept token outside the accepted grammar, site names) of a Beagle file that holds the
    tokens in its kept columns (rows_of)."""
    rows = rows_of(tokens, n)
    names = [b"s%d" % i for i in range(len(rows))]
    lines = [beagle_header(n, sep.strip() or sep, header_pad)] + [beagle_line(nm, r, filler, sep) for nm, r in zip(names, rows)]
    want, flagged = expected_rows(rows)
    return eol.join(lines) + (eol if final_eol else b""), want, flagged, [x.decode() for x in names]


# ---------------------------------------------------------------- every d.dddddd
def f6_decade(lead, n=500):
    """All 10^6 tokens "lead.dddddd" as the kept values of a Beagle file of n individuals (10^6 / 2n lines), built from byte arrays:
    (text, expected (m, 2n) float32).  The expectation is k / 1e6 in float64, rounded to float32 -- atof32 of the token, one
    correctly rounded division of two exact numbers (held against atof32 by the CPU tests)."""
    m = 1_000_000 // (2 * n)
    k = np.random.default_rng(lead).permutation(1_000_000).astype(np.int64) + lead * 1_000_000
    want = (k / 1e6).astype(np.float32).reshape(m, 2 * n)
    txt = np.empty((m, n, 3, 9), dtype=np.uint8)
    txt[:, :, :, 0] = 9
    txt[:, :, 2, 1:] = np.frombuffer(b"0.333333", dtype=np.uint8)
    v = k.reshape(m, n, 2)
    txt[:, :, :2, 1] = 48 + v // 1_000_000
    txt[:, :, :2, 2] = 46
    r = v % 1_000_000
    for d in range(6):
        txt[:, :, :2, 3 + d] = 48 + (r // 10 ** (5 - d)) % 10
    body = txt.reshape(m, -1)
    lines = [b"c%d_%d\tA\tC" % (lead, s) + body[s].tobytes() for s in range(m)]
    return beagle_header(n) + b"\n" + b"\n".join(lines) + b"\n", want


def f6_token(k):
    return b"%d.%06d" % (k // 1_000_000, k % 1_000_000)


# ---------------------------------------------------------------- what a text covers of the wave-level machinery
_IS_DELIM = np.zeros(256, dtype=bool)
_IS_DELIM[list(DELIMS)] = True


def spans(line):
    """(starts, ends) of the tokens of a line, as arrays: token i is line[starts[i]:ends[i]]."""
    nd = np.concatenate(([False], ~_IS_DELIM[np.frombuffer(line, dtype=np.uint8)], [False]))
    edge = np.flatnonzero(nd[1:] != nd[:-1])
    return edge[0::2], edge[1::2]


def kept_spans(line, n):
    """... of the tokens in the kept columns of a Beagle line of n individuals."""
    a, b = spans(line)
    keep = np.arange(3, 3 + 3 * n)
    keep = keep[(keep - 3) % 3 < 2]
    return a[keep], b[keep]


AROUND = range(-16, 2)                                 # positions around a step boundary: -16 .. +1


class Coverage:
    """What tokens cover when their line begins `offset` bytes into a 16-byte word of its chunk (a wavefront's steps count from
    that word, so a byte p of the line is byte offset + p of the first step): (byte within the word, length) of every token --
    lengths above 16 counted as 17 -- and, per length, where tokens begin and where their last byte lies around the first step
    boundary (0 = the first byte of the second step)."""

    def __init__(self, offset, starts, ends):
        n = np.minimum(ends - starts, 17)
        a, z = starts + offset, ends - 1 + offset
        self.word = set(np.unique((a % 16) * 32 + n).tolist())
        self.first = self._around(n, a - STEP)
        self.last = self._around(n, z - STEP)

    @staticmethod
    def _around(n, d):
        near = (d >= AROUND[0]) & (d <= AROUND[-1])
        return set(np.unique(n[near] * 64 + (d[near] - AROUND[0])).tolist())

    def missing(self, lengths):
        """What is not covered for tokens of the given lengths (17 = every longer one)."""
        out = []
        for n in sorted({min(x, 17) for x in lengths}):
            out += [("word", w, n) for w in range(16) if w * 32 + n not in self.word]
            out += [("first", n, d) for d in AROUND if n * 64 + d - AROUND[0] not in self.first]
            out += [("last", n, d) for d in AROUND if n * 64 + d - AROUND[0] not in self.last]
        return out


def file_spans(lines, n=None):
    """The spans of all lines in one pair of arrays (n: only the kept columns of Beagle lines of n individuals)."""
    parts = [kept_spans(x, n) if n else spans(x) for x in lines]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def strip_starts(lines, tpi=2):
    """Where, in its line, the first token of every strip after the first begins.  (A line that begins `offset` bytes into a word has
    it at byte (offset + start) % STEP of a step; at byte 0 the strip before it ends exactly with the step before.)"""
    out = []
    for x in lines:
        a, _ = spans(x)
        out += a[STRIP * tpi::STRIP * tpi].tolist()
    return np.array(out)


# ---------------------------------------------------------------- Beagle files of the GPU cases, each with what it must give
class BeagleCase:
    def __init__(self, text, want, flagged, names, group_of=None, n_groups=1, lines=None, n=None):
        self.text, self.want, self.flagged, self.names = text, want, flagged, names
        self.group_of, self.n_groups = group_of, n_groups
        self.lines, self.n = lines, n                  # the data lines and their individuals, where coverage is counted


def tokens_case(tokens, n=24, **kw):
    return BeagleCase(*beagle_file(tokens, n, **kw))


ALIGN_LENGTHS = tuple(range(1, 17)) + (17, 18, 31, 32, 33, 40)
ALIGN_SHIFTS = range(1040)


def alignment_case(length, shifts=ALIGN_SHIFTS, seed=5, bodies=7):
    """Lines whose kept (and dropped) tokens all have `length` bytes, long enough to pass two steps, one per shift: the site name of
    line i is lengthened by shifts[i] bytes.  Lengths above 16 flag every line."""
    n = -(-(2 * STEP + 64) // (3 * (length + 1)))
    toks = tokens_of_length(length, bodies * 3 * n, seed)
    kept, fill = [], []
    for b in range(bodies):
        t = toks[b * 3 * n:(b + 1) * 3 * n]
        kept.append([t[3 * i + w] for i in range(n) for w in range(2)])
        fill.append([t[3 * i + 2] for i in range(n)])
    body_want, body_flagged = expected_rows(kept)
    assert body_flagged == (bodies if length > 16 else 0)
    lines, names = [], []
    for i, s in enumerate(shifts):
        names.append(b"L%d_" % length + (b"%d" % i).rjust(5, b"x") + b"n" * s)
        lines.append(beagle_line(names[-1], kept[i % bodies], fill[i % bodies]))
    want = body_want[np.arange(len(lines)) % bodies]
    text = beagle_header(n) + b"\n" + b"\n".join(lines) + b"\n"
    return BeagleCase(text, want, len(lines) if length > 16 else 0, [x.decode() for x in names], lines=lines, n=n)


def _mixed_tokens():
    """Ties with their neighbours and a sample of every other generator: what the small files of separators, ignored columns and
    placement carry."""
    return ties()[::5] + contract_tokens(400, 3) + grammar_tokens()[::97] + substituted()[::61] + beyond_contract()[::3]


SEPARATORS = (b"\t", b" ", b"  ", b" \t")


def separator_case(k):
    """k = 0..15: the header lengthened by k bytes (the first data line begins at every offset of a word), the separators in turn,
    CRLF in every other group of four, every third file without a newline at its end."""
    return tokens_case(_mixed_tokens(), n=7, sep=SEPARATORS[k % 4], eol=b"\r\n" if (k // 4) % 2 else b"\n", final_eol=k % 3 != 0, header_pad=k)


JUNK = [b"junk", b"\xff\xfe\x80", b"0.5abc", b"nan", b"1e", b"x" * 40, b"0." + b"123456789" * 4 + b"12", b"-", b"\x7f", b"1e400", b"0x1p-2"]


def ignored_columns_case():
    """Junk, bytes >= 0x80 and 40-byte tokens in the dropped third column, the site name, the allele columns and behind column 3 + 3n;
    the kept columns hold accepted tokens only: no line is flagged."""
    n = 7
    tokens = [t for t in _mixed_tokens() if device_takes(t)]
    rows = rows_of(tokens, n)
    names, lines = [], []
    for i, r in enumerate(rows):
        name = [b"s%d" % i, "s%d_é中".encode() % i, b"s%d_" % i + b"x" * 40, b"nan%d" % i, b"0.5abc%d" % i][i % 5]
        alleles = [(b"A", b"C"), (b"\xff\x80", b"1e"), (b"y" * 40, b"nan"), (b"0.5abc", b"-")][i % 4]
        behind = [(), (b"junk",), (b"\xfe" * 3, b"z" * 40, b"1e"), (b"0.1",) * 5][i % 4]
        names.append(name)
        lines.append(beagle_line(name, r, JUNK[i % len(JUNK):] + JUNK[:i % len(JUNK)], b"\t", alleles, behind))
    want, flagged = expected_rows(rows)
    assert flagged == 0
    return BeagleCase(beagle_header(n) + b"\n" + b"\n".join(lines) + b"\n", want, 0, [x.decode() for x in names])


def placement_case():
    """The ties file with three populations interleaved over the slabs -- 3, 2 and 2 of the 7 individuals: an odd column count -- and
    more than two 64-row tiles: neighbours of a tie differ from it, so no misplaced value equals what belongs there."""
    case = tokens_case(ties(), n=7)
    assert case.want.shape[0] > 130
    case.group_of, case.n_groups = np.array([0, 1, 2, 0, 1, 2, 0], dtype=np.int32), 3
    return case


BEAGLE_CASES = {"ties": lambda: tokens_case(ties()), "grammar": lambda: tokens_case(grammar_tokens(), n=3),
                "substituted": lambda: tokens_case(substituted(), n=3), "beyond_contract": lambda: tokens_case(beyond_contract() + CONTRACT_EXTREMES, n=5),
                "ignored_columns": ignored_columns_case, "placement": placement_case}
BEAGLE_CASES.update(("separators_%d" % k, lambda k=k: separator_case(k)) for k in range(16))
BEAGLE_CASES.update(("align_%d" % n, lambda n=n: alignment_case(n)) for n in ALIGN_LENGTHS)
CONTRACT_COUNT, CONTRACT_SEED = 1_000_000, 20


def contract_case(count=CONTRACT_COUNT):
    return tokens_case(contract_tokens(count, CONTRACT_SEED), n=100)


# ---------------------------------------------------------------- integer tables of the GPU cases
DEPTH_FORMS = [b"%d" % v for v in range(256)] + [b"%02d" % v for v in range(10)] + [b"%03d" % v for v in range(100)]
DEPTH_SHIFTS = range(1040)


class DepthCase:
    def __init__(self, lines, want, n, flagged=0, counts=False, majmin=None, head=b""):
        self.lines, self.want, self.n, self.flagged, self.counts, self.majmin = lines, want, n, flagged, counts, majmin
        self.text = head + b"\n".join(lines) + b"\n"
        self.head = head                               # counts: the header line, which np.loadtxt must skip


def depth_forms_case(shifts=DEPTH_SHIFTS, seed=9):
    """Every value 0..255 in every form of at most three characters (%d, %02d, %03d: 366 tokens = 183 individuals) in another order
    per line, behind shifts[i] blanks."""
    rnd = random.Random(seed)
    lines, values = [], []
    for s in shifts:
        forms = DEPTH_FORMS[:]
        rnd.shuffle(forms)
        lines.append(b" " * s + b" ".join(forms))
        values.append([int(t) for t in forms])
    return DepthCase(lines, np.array(values, dtype=np.int32), len(DEPTH_FORMS) // 2)


def depth_strip_case(n, shifts=DEPTH_SHIFTS, seed=11):
    """n individuals behind shifts[i] blanks.  The token widths (1..3) are dealt per line -- so what lies on either side of a strip
    boundary differs from line to line -- but every strip's 512 tokens take the same number of bytes in every line: over 1024
    consecutive shifts the first token of every later strip falls on every byte of a step."""
    rnd = random.Random(seed + n + len(shifts))
    ranges = {1: (0, 9), 2: (10, 99), 3: (100, 255)}
    lines, values = [], []
    for s in shifts:
        row = []
        for i0 in range(0, 2 * n, 2 * STRIP):
            widths = ([1] * 171 + [2] * 171 + [3] * 170)[:min(2 * STRIP, 2 * n - i0)]
            if len(widths) == 2 * STRIP:
                rnd.shuffle(widths)
            row += [rnd.randint(*ranges[w]) for w in widths]
        lines.append(b" " * s + b" ".join(b"%d" % v for v in row))
        values.append(row)
    return DepthCase(lines, np.array(values, dtype=np.int32), n)


def depth_counts_case(n=300, m=130):
    """Counts mode: the four counts of an individual pairwise different and 1, 2, 3 and 1 characters wide; every ordered (major,
    minor) pair of selectors, equal ones included, on consecutive sites.  The expectation restates np.take_along_axis."""
    rnd = random.Random(4)
    counts = np.empty((m, n, 4), dtype=np.int64)
    for s in range(m):
        for i in range(n):
            a = rnd.randint(0, 9)
            counts[s, i] = (a, rnd.randint(10, 99), rnd.randint(100, 255), (a + rnd.randint(1, 9)) % 10)
    majmin = np.array([(s % 16 // 4, s % 4) for s in range(m)], dtype=np.uint8)
    lines = [b"\t".join(b"%d" % v for v in row) + b"\t" for row in counts.reshape(m, 4 * n)]
    want = np.empty((m, 2 * n), dtype=np.int32)
    sel = majmin.astype(np.int64)
    want[:, 0::2] = np.take_along_axis(counts, np.broadcast_to(sel[:, None, :1], (m, n, 1)), 2)[:, :, 0]
    want[:, 1::2] = np.take_along_axis(counts, np.broadcast_to(sel[:, None, 1:], (m, n, 1)), 2)[:, :, 0]
    head = b"".join(b"ind%dTotDepth%s\t" % (i, b) for i in range(n) for b in (b"A", b"C", b"G", b"T")) + b"\n"
    return DepthCase(lines, want, n, counts=True, majmin=majmin, head=head)


DEPTH_FLAGGED_TOKENS = (b"+7", b"0007", b"00255")      # np.loadtxt reads them as 0..255; the kernel takes 1..3 digits only


def depth_flagged_case(n=300, tokens=DEPTH_FLAGGED_TOKENS):
    """Each token the kernel must flag at the first, a middle and the last column and as individuals 255 and 256 (either token of
    the pair), one per line, between lines the kernel takes."""
    rnd = random.Random(6)
    cols = (0, 1, n, 2 * n - 2, 2 * n - 1, 2 * 255, 2 * 255 + 1, 2 * 256, 2 * 256 + 1)
    lines, flagged = [], 0
    for t in tokens:
        for c in cols:
            for bad in (None, c):
                row = [b"%d" % rnd.choice((rnd.randint(0, 9), rnd.randint(10, 255))) for _ in range(2 * n)]
                if bad is not None:
                    row[bad] = t
                    flagged += 1
                lines.append(b" ".join(row))
    return DepthCase(lines, None, n, flagged=flagged)


DEPTH_CASES = {"forms": depth_forms_case, "strip_257": lambda: depth_strip_case(257), "strip_513": lambda: depth_strip_case(513),
               "counts": depth_counts_case, "flagged": depth_flagged_case}
DEPTH_CASES.update(("tile_%d" % m, lambda m=m: depth_strip_case(257, range(500, 500 + m))) for m in (63, 64, 65, 127, 129))
