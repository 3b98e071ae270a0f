"""A deflate WRITER for the tests (RFC 1951, from the specification): it emits exactly the tokens, code lengths and block structure
a case calls for, so that the device inflate (csrc/inflate.hip) is held to the format and not to what one encoder happens to
choose.  Nothing here knows the kernel; `zlib.decompress(stream, -15)` is the independent reference for every stream it writes
(tests/test_deflate_build_cpu.py).

A token is a literal `0..255` or a match `(length 3..258, distance 1..32768)`.  Blocks are appended to one LSB-first bit writer
(`Deflate`), so several blocks form one stream at any bit phase; `raw_bits` writes anything else (malformed streams)."""
import bisect
import heapq

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [b for b in range(1, 14) for _ in (0, 1)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32                  # (30 and 31 have codes and no meaning: the streams that must be refused use them)
EOB = 256


def length_code(length, long258=False):
    """(symbol, extra bits, extra value) of a match length; long258 writes 258 as symbol 284 with all five extra bits set."""
    if length == 258 and not long258:
        return 285, 0, 0
    i = bisect.bisect_right(LEN_BASE, length, 0, 28) - 1
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_code(dist):
    i = bisect.bisect_right(DIST_BASE, dist) - 1
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def expand(tokens, prefix=b""):
    """What a token list stands for, behind `prefix` (which matches may reach into)."""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            if not (3 <= length <= 258 and 1 <= dist <= len(out)):
                raise ValueError("match %r at %d" % (t, len(out)))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:                               # the source runs into the bytes the match itself writes: period `dist`
                seg = bytes(out[-dist:])
                out += (seg * (length // dist + 1))[:length]
        else:
            out.append(t)
    return bytes(out[len(prefix):])


def _reverse(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical(lens):
    """Per symbol (code as it goes into an LSB-first stream, length), None for a symbol without a code (RFC 1951 3.2.2).  An
    over-subscribed set still gets codes (cut to their length): only the streams that must be refused carry one."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = []
    for n in lens:
        if n:
            out.append((_reverse(nxt[n] & ((1 << n) - 1), n), n))
            nxt[n] += 1
        else:
            out.append(None)
    return out


def kraft(lens, limit=15):
    """The code space a set of lengths takes, in units of 2**-limit (complete at 2**limit)."""
    return sum(1 << (limit - n) for n in lens if n)


def huffman_lengths(freqs, limit=15):
    """Code lengths of at most `limit` bits for the symbols with freq > 0, a complete set (two symbols at least get a code)."""
    lens = [0] * len(freqs)
    used = [s for s, f in enumerate(freqs) if f > 0]
    for s in range(len(freqs)):                 # a code of one symbol has no length: give it company
        if len(used) >= 2:
            break
        if s not in used:
            used.append(s)
    heap = [(max(freqs[s], 0), s, (s,)) for s in used]
    heapq.heapify(heap)
    while len(heap) > 1:
        fa, ka, a = heapq.heappop(heap)
        fb, kb, b = heapq.heappop(heap)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
    if max(lens) > limit:
        for s in used:
            lens[s] = min(lens[s], limit)
        over = kraft(lens, limit) - (1 << limit)
        while over > 0:                         # lengthen the longest codes still below the limit
            s = max((s for s in used if lens[s] < limit), key=lambda s: (lens[s], -freqs[s]))
            over -= 1 << (limit - lens[s] - 1)
            lens[s] += 1
        slack = -over
        while slack > 0:                        # and hand back what that took too much
            s = max((s for s in used if lens[s] > 1 and (1 << (limit - lens[s])) <= slack), key=lambda s: lens[s])
            slack -= 1 << (limit - lens[s])
            lens[s] -= 1
    assert kraft(lens, limit) == 1 << limit, "not a complete code"
    return lens


def complete(lens, limit=15, pad_symbols=()):
    """`lens` with the code space its non-zero entries leave free handed to `pad_symbols` (symbols without a length that the
    case does not use), one power of two each: a case can force chosen symbols to chosen lengths and still have a complete set."""
    lens = list(lens)
    free = (1 << limit) - kraft(lens, limit)
    if free < 0:
        raise ValueError("over-subscribed")
    pads = [s for s in pad_symbols if not lens[s]]
    if free == 1 << limit:
        need = [1, 1]
    else:
        need = [limit - b for b in range(limit - 1, -1, -1) if free >> b & 1]
    if len(need) > len(pads):
        raise ValueError("%d symbols needed to complete the set, %d offered" % (len(need), len(pads)))
    for s, n in zip(pads, need):
        lens[s] = n
    assert kraft(lens, limit) == 1 << limit
    return lens


def encode_tokens(tokens, lit_codes, dist_codes, long258=False, trace=None):
    """The tokens' bits as (value, number of bits), LSB first.  trace (a list) receives (first bit, bits) of every match."""
    value, total, acc, n = 0, 0, 0, 0
    for t in tokens:
        if isinstance(t, tuple):
            ls, lxb, lxv = length_code(t[0], long258)
            ds, dxb, dxv = dist_code(t[1])
            lc, ln = lit_codes[ls]
            dc, dn = dist_codes[ds]
            if trace is not None:
                trace.append((total + n, ln + lxb + dn + dxb))
            acc |= (lc | lxv << ln | dc << (ln + lxb) | dxv << (ln + lxb + dn)) << n
            n += ln + lxb + dn + dxb
        else:
            c, k = lit_codes[t]
            acc |= c << n
            n += k
        if n >= 2048:
            value |= acc << total
            total += n
            acc, n = 0, 0
    return value | acc << total, total + n


_FIXED_LIT = canonical(FIXED_LIT_LENS)
_FIXED_DIST = canonical(FIXED_DIST_LENS)


def encode_fixed(tokens, long258=False):
    """(value, bits) of tokens in the fixed code, without block header and end-of-block: a family that needs thousands of
    streams with a common body encodes the body once and appends it with `Deflate.raw_bits`."""
    return encode_tokens(tokens, _FIXED_LIT, _FIXED_DIST, long258)


def rle_code_lengths(lens, maximal=True):
    """Code lengths as code-length symbols [(first index, symbol, extra bits, extra value, lengths covered)]: runs become the
    longest repeats 16/17/18 allow (maximal=False: no repeat symbols at all)."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if not maximal:
            out += [(i + k, v, 0, 0, 1) for k in range(run)]
            i = j
            continue
        if v:
            out.append((i, v, 0, 0, 1))
            i, run = i + 1, run - 1
        while run >= 3:
            if v:
                k = min(run, 6)
                out.append((i, 16, 2, k - 3, k))
            elif run >= 11:
                k = min(run, 138)
                out.append((i, 18, 7, k - 11, k))
            else:
                k = min(run, 10)
                out.append((i, 17, 3, k - 3, k))
            i, run = i + k, run - k
        out += [(i + k, v, 0, 0, 1) for k in range(run)]
        i = j
    return out


def token_frequencies(tokens, long258=False):
    lit, dist = [0] * 286, [0] * 30
    lit[EOB] = 1
    for t in tokens:
        if isinstance(t, tuple):
            lit[length_code(t[0], long258)[0]] += 1
            dist[dist_code(t[1])[0]] += 1
        else:
            lit[t] += 1
    return lit, dist


def used_code_lengths(tokens, lit_lens, dist_lens, long258=False):
    """The code lengths of the symbols the tokens actually use: (literals, length symbols, distance symbols, end-of-block)."""
    lit, dist = token_frequencies(tokens, long258)
    return ({lit_lens[s] for s in range(256) if lit[s]}, {lit_lens[s] for s in range(257, 286) if lit[s]},
            {dist_lens[s] for s in range(30) if dist[s]}, lit_lens[EOB])


class Deflate:
    """One raw deflate stream under construction.  `blocks` records what was written: per block a dict with its type, the bit
    it starts at, and for a dynamic block the header's fields and code-length symbols."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.blocks = []

    def bit_position(self):
        return len(self.out) * 8 + self.n

    def raw_bits(self, value, n):
        self.acc |= value << self.n
        self.n += n
        if self.n >= 4096:
            self._flush()
        return self

    def _flush(self):
        k = self.n >> 3
        self.out += (self.acc & ((1 << (k * 8)) - 1)).to_bytes(k, "little")
        self.acc >>= k * 8
        self.n &= 7

    def getvalue(self):
        """The stream so far, the last byte filled up with zero bits."""
        self._flush()
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")

    def stored(self, data, final, nlen=None):
        self.blocks.append({"type": 0, "bit": self.bit_position(), "bytes": len(data)})
        self.raw_bits(1 if final else 0, 1).raw_bits(0, 2)
        self.raw_bits(0, -self.n & 7)
        self.blocks[-1]["len_at_byte"] = self.bit_position() >> 3
        self.raw_bits(len(data), 16).raw_bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self._flush()
        self.out += data
        return self

    def fixed(self, tokens, final, long258=False, eob=True, trace=None):
        self.blocks.append({"type": 1, "bit": self.bit_position(), "tokens": len(tokens)})
        self.raw_bits(1 if final else 0, 1).raw_bits(1, 2)
        t0 = self.bit_position()
        sub = None if trace is None else []
        self.raw_bits(*encode_tokens(tokens, _FIXED_LIT, _FIXED_DIST, long258, sub))
        if trace is not None:
            trace += [(t0 + b, k) for b, k in sub]
        if eob:
            self.raw_bits(*_FIXED_LIT[EOB])
        return self

    def dynamic(self, tokens, final, lit_lens=None, dist_lens=None, clen_lens=None, hclen=None, maximal=True, across=True,
                long258=False, eob=True, trace=None, clen_tokens=None, header_only=False):
        """A dynamic block.  Code lengths given are used as given (lit_lens: 257..288 entries, dist_lens: 1..32, clen_lens: 19 by
        symbol); otherwise they follow from the token frequencies, at most 15 (7) bits.  maximal / across: code lengths are written
        with the longest repeats possible, runs continuing from the literal/length lengths into the distance lengths.  clen_tokens
        replaces the code-length symbols altogether [(symbol, extra bits, extra value)] (malformed headers)."""
        flit, fdist = token_frequencies(tokens, long258)
        if lit_lens is None:
            lit_lens = huffman_lengths(flit, 15)
            while len(lit_lens) > 257 and not lit_lens[-1]:
                lit_lens.pop()
        if dist_lens is None:
            used = [s for s in range(30) if fdist[s]]
            if not used:
                dist_lens = [0]
            elif len(used) == 1:
                dist_lens = [0] * used[0] + [1]          # the one incomplete set inflate accepts: a single code of one bit
            else:
                dist_lens = huffman_lengths(fdist, 15)
                while not dist_lens[-1]:
                    dist_lens.pop()
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        hlit, hdist = len(lit_lens), len(dist_lens)
        if clen_tokens is None:
            if across:
                runs = rle_code_lengths(lit_lens + dist_lens, maximal)
            else:
                runs = rle_code_lengths(lit_lens, maximal) + [(i + hlit, *r) for i, *r in rle_code_lengths(dist_lens, maximal)]
            clen_tokens = [(s, xb, xv) for _, s, xb, xv, _ in runs]
        else:
            runs = None
        if clen_lens is None:
            f = [0] * 19
            for s, _, _ in clen_tokens:
                f[s] += 1
            clen_lens = huffman_lengths(f, 7)
        if hclen is None:
            hclen = max(4, 1 + max(i for i, s in enumerate(CLEN_ORDER) if clen_lens[s]))
        self.blocks.append({"type": 2, "bit": self.bit_position(), "tokens": len(tokens), "hlit": hlit, "hdist": hdist, "hclen": hclen,
                            "clen_lens": list(clen_lens), "runs": runs, "lit_lens": lit_lens, "dist_lens": dist_lens})
        self.raw_bits(1 if final else 0, 1).raw_bits(2, 2)
        self.raw_bits(hlit - 257, 5).raw_bits(hdist - 1, 5).raw_bits(hclen - 4, 4)
        for i in range(hclen):
            self.raw_bits(clen_lens[CLEN_ORDER[i]], 3)
        cc = canonical(clen_lens)
        for s, xb, xv in clen_tokens:
            c, k = cc[s]
            self.raw_bits(c | xv << k, k + xb)
        self.blocks[-1]["header_bits"] = self.bit_position() - self.blocks[-1]["bit"]
        if header_only:
            return self
        lit_codes, dist_codes = canonical(lit_lens), canonical(dist_lens)
        t0 = self.bit_position()
        sub = None if trace is None else []
        self.raw_bits(*encode_tokens(tokens, lit_codes, dist_codes, long258, sub))
        if trace is not None:
            trace += [(t0 + b, k) for b, k in sub]
        if eob:
            self.raw_bits(*lit_codes[EOB])
        return self


def tokenize(data, max_dist=32768, min_len=3, max_len=258):
    """A plain greedy matcher (the last position of every three-byte string): real text as tokens."""
    tokens, last, i, n = [], {}, 0, len(data)
    while i < n:
        key = data[i:i + 3]
        j = last.get(key)
        length = 0
        if j is not None and i - j <= max_dist and i + 3 <= n:
            limit = min(max_len, n - i)
            length = 3
            while length < limit and data[j + length] == data[i + length]:
                length += 1
        if length >= max(min_len, 3):
            tokens.append((length, i - j))
            for k in range(i, min(i + length, n - 2)):
                last[data[k:k + 3]] = k
            i += length
        else:
            tokens.append(data[i])
            if i + 3 <= n:
                last[key] = i
            i += 1
    return tokens
