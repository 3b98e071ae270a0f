"""Enumerated inputs for the ORDER in which the scoring path adds its float64 block sums (csrc/assign_kernels.hip:
block_prefix_kernel, chunk_total_kernel, combine_parts_kernel; csrc/score_api.hip: score_sums_enqueue, wgs_score_total_from,
wgs_score_totals_all, the window carry of wgs_score_stream_push).  The twin of tests/score_cases.py, whose cells are cut so that
their float64 sums are exact in ANY order and which therefore cannot tell one order from another.  Here the sum of every 4096-site
block is exact in any order -- so the sweep, which adds inside a block in an order of its own, hands over the one block sum there is
-- and nearly every addition ACROSS blocks rounds, so that np.sum(vec, dtype=float) of glassy.py:38 is one number and a plausible
wrong order another.  NumPy and the standard library only.

THE TERMS.  One term is v = (float)log((double)s) with s the float32 likelihood sum of a pair (g0, g1) at a frequency a.  All
likelihoods are 0 or 1 (the same case as six-decimal Beagle text holds the same bits) and all frequencies lie next to 0 or next to 1:
    `low`  population   a = 2^-e (1 + j / 2^23), e = 16 .. 18, j a hash of (site, population): low bits that differ from site to site
    `high` population   a = (float)(1 - that)
    pair (0, 0)   s = a^2          v = -20.8 .. -25.0 at a low population      |v| < 2^-13 at a high one
    pair (0, 1)   s = 2 a (1 - a)  v = -9.7 .. -11.8 at either
    pair (1, 0)   s = (1 - a)^2    |v| < 2^-13 at a low population             v = -20.8 .. -25.0 at a high one
These are the three magnitude CLASSES `big` [16, 32), `mid` [8, 16) and `small` [2^-19, 2^-13): the terms of a class are multiples of
2^-19, 2^-20 and (at least) 2^-56, a block sum of `big` is about 2^16.5 and one of `small` 2^-5 .. 2^-2 with bits down to 2^-40 or
so.  A running total of 2^17 .. 2^21 keeps bits down to 2^-36 .. 2^-32 only: adding a `small` block to it rounds, and adding two of
them one after the other is not adding their sum.  (Frequencies nearer 0 and 1, 2^-20, make the same classes but fewer cells that
tell the orders apart: next to 1 a float32 frequency takes 17 values there.)

THE LAYOUT.  Every (individual, 4096-site block) holds ONE pair, so one class per population kind; an individual is a PATTERN of
classes over the blocks (PATTERNS: the class named is the one at a `low` population, a `high` one sees its mirror image, big <->
small).  The patterns are all fourteen mixed big/small patterns of two chunks (four blocks), repeated -- which holds every one of
them shifted by one block and by one chunk --, six with the `mid` class and periods of 2, 3, 5 and 6 blocks, and five with ONE big
block among small ones: the first, and the last block of the shapes of 7, 9, 10 and 17 blocks (the only one of the shape of 1).  The
25 individuals interleave over population slabs of 1, 2, 5, 8 and 9 columns; there are K_ALL = 13 populations, of which a test takes
the first 6 (one register batch of the sweeps) or all 13 (two).

THE SHAPES are given by block count, NBLOCKS x TAILS: every exit of block_prefix_kernel's loops (8 blocks at a time, then pairs, then
a single block), with the last block full, ragged inside a tile, and holding a single site.  A pattern is a function of the block
index alone, so every shape is a PREFIX of the largest one (17 blocks, 69632 sites): the oracle's per-site values are computed once.

THE LAST CHUNK.  One block of every shape is not a prefix.  NumPy sums a chunk pairwise, and the top split of a FULL chunk is the
block edge, 4096 + 4096 -- but a short chunk of n sites is split at n / 2 rounded down to a multiple of 8, inside its first block: a
last chunk of a full block and a partial one (an even block count with a ragged or single-site last block) is S[2c] + S[2c+1] only
if the partial sums of the whole CHUNK are exact, not just those of each block.  So in these shapes the partial block holds the pairs
of the block before it (closes_a_chunk, matrix_of), the chunk is of one class, and tests/test_order_cases_cpu.py asserts the
chunk-wide exactness in integers too.  With a `big` block before a `small` partial one NumPy's own sum is another number than
S[2c] + S[2c+1] (the CPU test shows it): the device's totals are np.sum's while every chunk's partial sums are exact, which 8192
float32 values within 2^14 of each other always are -- DESIGN section 3.4 says so.

THE ORDERS.  numpy_order is the claim: total = total + (S[2c] + S[2c+1]), chunk after chunk from 0.  WRONG_ORDERS are what a
plausible bug would compute instead; each is a plain loop over the exact block sums, written for all cells at once (S is
(blocks, cells): the additions are elementwise IEEE float64 additions).  cannot_differ says, by reasoning, at which block counts an
order is numpy_order whatever the data; everywhere else tests/test_order_cases_cpu.py requires it to differ from np.sum in at least
MIN_DIFFERENT cells.  Two orders can never show and are named here for that reason only: a restart at every 8192 sites is
total + chunk either way, and combine_parts_kernel adds partial sums of one block, which are exact in any order."""
import numpy as np

from fisher_cases import F32, ids_for, interleave

BLOCK, CHUNK = 4096, 8192
NBLOCKS = (1, 2, 3, 7, 8, 9, 10, 15, 16, 17)
TAILS = ("full", "ragged", "single")
RAGGED_SITES = 2 * 64 + 37                                   # two tiles and a ragged third
SHAPES = tuple((b, t) for b in NBLOCKS for t in TAILS)
MAX_BLOCKS = max(NBLOCKS)
M_ALL = MAX_BLOCKS * BLOCK
SLABS = (1, 2, 5, 8, 9)
K_ALL = 13
K_TESTED = (6, 13)                                           # one register batch (6, two pairs per wave) and two (7 + 6)
MIN_DIFFERENT = 8

CLASSES = ("big", "mid", "small")
CLASS_RANGE = {"big": (16.0, 32.0), "mid": (8.0, 16.0), "small": (2.0 ** -19, 2.0 ** -13)}      # lo <= |v| < hi
PAIR_OF = {"B": (0.0, 0.0), "M": (0.0, 1.0), "S": (1.0, 0.0)}
CLASS_AT = {"low": {"B": "big", "M": "mid", "S": "small"}, "high": {"B": "small", "M": "mid", "S": "big"}}


def _single(j):
    return "".join("B" if b == j else "S" for b in range(MAX_BLOCKS))


PATTERNS = (tuple("".join("B" if bits >> j & 1 else "S" for j in range(4)) for bits in range(1, 15)) +
            ("MS", "SSM", "BMS", "SMB", "BSMSMB", "SBMMS") +
            tuple(_single(j) for j in (0, 6, 8, 9, 16)))
# population k: (kind, e) -- a = 2^-e (1 + j / 2^23) or its complement
FAMILIES = (("low", 18), ("high", 18), ("low", 17), ("high", 17), ("low", 16), ("high", 16), ("low", 18), ("high", 18), ("low", 17),
            ("high", 17), ("low", 16), ("high", 16), ("low", 18))
assert len(FAMILIES) == K_ALL and len(PATTERNS) == sum(SLABS)


def sites_of(shape):
    nblocks, tail = shape
    return (nblocks - 1) * BLOCK + {"full": BLOCK, "ragged": RAGGED_SITES, "single": 1}[tail]


def pattern_class(i, block):
    """The letter (B, M, S) individual i holds in a block."""
    p = PATTERNS[i]
    return p[block % len(p)]


def frequencies(m=M_ALL):
    """(m, K_ALL) float32."""
    site = np.arange(m, dtype=np.uint64)[:, None]
    k = np.arange(K_ALL, dtype=np.uint64)[None, :]
    j = (((site + np.uint64(1)) * np.uint64(2654435761) + k * np.uint64(40503) * np.uint64(65537)) >> np.uint64(9)) % np.uint64(1 << 23)
    A = np.empty((m, K_ALL), dtype=F32)
    for col, (kind, e) in enumerate(FAMILIES):
        low = 2.0 ** -e * (1.0 + j[:, col].astype(np.float64) / 2.0 ** 23)             # exact, and a float32
        A[:, col] = low if kind == "low" else 1.0 - low
    return A


def build():
    """dict(L (M_ALL, 2n) float32 of 0 and 1, A (M_ALL, K_ALL), labels (n,), sizes, IDs, letters (n, MAX_BLOCKS) of B / M / S)."""
    labels = interleave(SLABS)
    n = len(labels)
    letters = np.array([[pattern_class(i, b) for b in range(MAX_BLOCKS)] for i in range(n)])
    L = np.empty((M_ALL, 2 * n), dtype=F32)
    for i in range(n):
        for b in range(MAX_BLOCKS):
            L[b * BLOCK:(b + 1) * BLOCK, 2 * i], L[b * BLOCK:(b + 1) * BLOCK, 2 * i + 1] = PAIR_OF[letters[i, b]]
    return dict(L=L, A=frequencies(), labels=labels, sizes=SLABS, IDs=ids_for(labels), letters=letters)


_case, _reference, _tails, _expected = [], [], {}, {}


def case():
    """The largest case, made once, shared, read-only; the case of a shape is its first sites_of(shape) sites (matrix_of)."""
    if not _case:
        c = build()
        for a in (c["L"], c["A"]):
            a.setflags(write=False)
        _case.append(c)
    return _case[0]


def closes_a_chunk(shape):
    """Whether the shape's last block is a partial one that closes a chunk: it then holds the pairs of the block before it (THE LAST
    CHUNK)."""
    return shape[0] % 2 == 0 and shape[1] != "full"


def letter(i, block, shape=None):
    """The letter (B, M, S) individual i holds in a block of a shape."""
    if shape is not None and closes_a_chunk(shape) and block == shape[0] - 1:
        block -= 1
    return pattern_class(i, block)


def claimed_class(i, k, block, shape=None):
    return CLASS_AT[FAMILIES[k][0]][letter(i, block, shape)]


def matrix_of(shape):
    """(L (m, 2n), A (m, K_ALL)) of a shape, read-only: the first m sites of case(), the last block rewritten where it closes a chunk."""
    c, m = case(), sites_of(shape)
    L, A = c["L"][:m], c["A"][:m]
    if closes_a_chunk(shape):
        L = L.copy()
        lo = (shape[0] - 1) * BLOCK
        L[lo:] = c["L"][lo - BLOCK:m - BLOCK]
        L.setflags(write=False)
    return L, A


def permutation(i, K):
    """The columns of A individual i's K populations point at in the per-individual test (K_ALL is prime: every stride walks through
    all columns)."""
    return (i + np.arange(K) * (1 + i % (K_ALL - 1))) % K_ALL


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def per_site(orc, L, A, threads=4):
    """(n, K, m) float32: glassy_cy.loglike of the oracle into zeros for every cell."""
    n, K, m = L.shape[1] // 2, A.shape[1], L.shape[0]
    L, A = np.ascontiguousarray(L), np.ascontiguousarray(A)
    V = np.zeros((n, K, m), dtype=F32)
    for i in range(n):
        for k in range(K):
            orc.loglike(L, A, V[i, k], threads, i, k)
    V.setflags(write=False)
    return V


class Values:
    """The oracle's per-site values of a shape: those of the largest case (computed once, shared, read-only) and, where the shape's
    last block is rewritten, that block's own."""

    def __init__(self, shape, V, tail):
        self.shape, self.m, self.V, self.tail = shape, sites_of(shape), V, tail
        self.n, self.K = V.shape[:2]

    def vector(self, i, k):
        """A float32 vector of its own, as glassy.py:36 makes one."""
        vec = np.array(self.V[i, k, :self.m], dtype=F32)
        if self.tail is not None:
            vec[self.m - self.tail.shape[-1]:] = self.tail[i, k]
        return vec

    def block(self, b):
        """(n, K, sites) float32: the terms of block b."""
        if self.tail is not None and b == self.shape[0] - 1:
            return self.tail
        return self.V[:, :, b * BLOCK:min((b + 1) * BLOCK, self.m)]


def reference(orc, shape):
    """The Values of a shape."""
    if not _reference:
        c = case()
        _reference.append(per_site(orc, c["L"], c["A"]))
    if closes_a_chunk(shape) and shape not in _tails:
        L, A = matrix_of(shape)
        lo = (shape[0] - 1) * BLOCK
        _tails[shape] = per_site(orc, L[lo:], A[lo:], threads=1)
    return Values(shape, _reference[0], _tails.get(shape))


def expected(vals):
    """(n, K_ALL) float64: np.sum(vec, dtype=float) of glassy.py:38 for every cell -- NumPy itself, called as the reference calls it.
    Once per shape, shared, read-only."""
    if vals.shape not in _expected:
        out = np.empty((vals.n, vals.K), dtype=np.float64)
        for idx in np.ndindex(out.shape):
            out[idx] = np.sum(vals.vector(*idx), dtype=float)
        out.setflags(write=False)
        _expected[vals.shape] = out
    return _expected[vals.shape]


def block_sums(vals):
    """(blocks, n, K) float64: the sum of every 4096-site block (exact in any order: exact_margin)."""
    return np.stack([vals.block(b).astype(np.float64).sum(axis=-1) for b in range(vals.shape[0])])


def exact_margin(v):
    """For the terms v (..., sites) float32 of one block per leading index, in integers: with g = (the least binary exponent of a
    term) - 24 every term is an integer multiple of 2^g (checked), and the sum of |v| / 2^g is returned, (...) int64.  A sum below
    2^53 means that every partial sum of the block, in any order, is a multiple of 2^g below 2^(g + 53): a float64, exactly."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    assert (v > 0).all() and np.isfinite(v).all()
    g = np.frexp(v)[1].min(axis=-1, keepdims=True) - 24
    q = np.ldexp(v, -g)
    assert (q == np.floor(q)).all() and (q < 2.0 ** 40).all()
    return q.astype(np.int64).sum(axis=-1)


# ---- the orders: S is (blocks, ...) float64, every function returns S.shape[1:] -------------------------------------------------------------
def chunk_sums(S):
    """(ceil(blocks / 2), ...): S[2c] + S[2c+1], the last block alone where their number is odd."""
    return np.stack([S[b] + S[b + 1] if b + 1 < len(S) else S[b] for b in range(0, len(S), 2)]) if len(S) else S[:0]


def numpy_order(S, start=None):
    """np.sum(vec, dtype=float): chunk after chunk of 8192 sites onto the running total."""
    total = np.zeros(S.shape[1:]) if start is None else start
    for b in range(0, len(S), 2):
        total = total + ((S[b] + S[b + 1]) if b + 1 < len(S) else S[b])
    return total


def plain_order(S):
    """Block after block."""
    total = np.zeros(S.shape[1:])
    for b in range(len(S)):
        total = total + S[b]
    return total


def pair_split_order(S, where):
    """(total + S[2c]) + S[2c+1] instead of total + (S[2c] + S[2c+1]) in block_prefix_kernel's unrolled loop (the first 8 *
    (blocks // 8) blocks), in its tail (the rest), or in both (`all`: plain_order, written the other way)."""
    total = np.zeros(S.shape[1:])
    unrolled = len(S) // 8 * 8
    for b in range(0, len(S), 2):
        split = where == "all" or (where == "unrolled") == (b < unrolled)
        if b + 1 >= len(S):
            total = total + S[b]
        elif split:
            total = (total + S[b]) + S[b + 1]
        else:
            total = total + (S[b] + S[b + 1])
    return total


def shard_totals_added(S, cuts):
    """Every shard [cut, next cut) (in blocks, multiples of 2) summed in NumPy's order from zero, the totals added in shard order."""
    edges = [0] + [c for c in cuts if 0 < c < len(S)] + [len(S)]
    total = np.zeros(S.shape[1:])
    for lo, hi in zip(edges[:-1], edges[1:]):
        total = total + numpy_order(S[lo:hi])
    return total


def restart_order(S, window_sites):
    """A window that restarted the running total: shard_totals_added at every multiple of the window."""
    w = window_sites // BLOCK
    return shard_totals_added(S, list(range(w, len(S), w)))


def carry_last_order(S, cuts):
    """chunk_total_kernel adding the carry behind its chunks, ((0 + C0) + C1 ...) + carry, shard after shard."""
    edges = [0] + [c for c in cuts if 0 < c < len(S)] + [len(S)]
    carry = None
    for lo, hi in zip(edges[:-1], edges[1:]):
        run = np.zeros(S.shape[1:])
        for c in chunk_sums(S[lo:hi]):
            run = run + c
        carry = run if carry is None else run + carry
    return carry


def continued_order(S, cuts):
    """What the shards and the windows are meant to do: every shard continues the total of the one before (numpy_order, cut up)."""
    edges = [0] + [c for c in cuts if 0 < c < len(S)] + [len(S)]
    total = None
    for lo, hi in zip(edges[:-1], edges[1:]):
        total = numpy_order(S[lo:hi], total)
    return total


SHARD_CUTS = (4, 8)                                         # blocks: the two cuts of the three-shard orders
SHARD_SHAPES = ((17, "ragged"), (10, "single"))             # what tests/test_gpu_order_cases.py cuts into shards on one device


def shard_cuts(shape):
    """The cuts (tuples of block numbers) of a shape in the shard test: every multiple of 8192 sites, and two cuts at once."""
    chunks = (shape[0] + 1) // 2
    return [(2 * c,) for c in range(1, chunks)] + [(2 * a, 2 * b) for a, b in ((2, 4), (1, 6)) if b < chunks]


def shards_can_differ(shape, cuts):
    """Whether a shard behind the first holds a block beyond its first chunk (see cannot_differ)."""
    edges = list(cuts) + [shape[0]]
    return any(hi - lo > 2 for lo, hi in zip(edges[:-1], edges[1:]))
WRONG_ORDERS = {
    "plain block order": plain_order,
    "(total + S[2c]) + S[2c+1]": lambda S: pair_split_order(S, "all"),
    "... in the unrolled loop only": lambda S: pair_split_order(S, "unrolled"),
    "... in the tail only": lambda S: pair_split_order(S, "tail"),
    "restart every 16384 sites": lambda S: restart_order(S, 16384),
    "restart every 24576 sites": lambda S: restart_order(S, 24576),
    "per-shard totals added": lambda S: shard_totals_added(S, SHARD_CUTS),
    "carry added last": lambda S: carry_last_order(S, SHARD_CUTS),
}


def cannot_differ(order, nblocks):
    """Whether a wrong order is numpy_order at this block count whatever the data -- by reasoning, not by looking at the sums:
    plain order and the pair split need a chunk of TWO blocks behind a total that is not zero (0 + S0 is exact, and (0 + S0) + S1 is
    S0 + S1): a fourth block; split in the unrolled loop only, an eighth block; in the tail only, a pair of blocks in a tail that does
    not start the sum -- or a tail of four blocks that does.  A restart (a shard, a late carry) shows only where a window that is not
    the first holds two chunks, (T + Ca) + Cb against T + (Ca + Cb): a block beyond the window's first chunk."""
    tail = nblocks % 8
    return {
        "plain block order": nblocks < 4,
        "(total + S[2c]) + S[2c+1]": nblocks < 4,
        "... in the unrolled loop only": nblocks < 8,
        "... in the tail only": tail < 2 if nblocks >= 8 else tail < 4,
        "restart every 16384 sites": nblocks <= 4 + 2,
        "restart every 24576 sites": nblocks <= 6 + 2,
        "per-shard totals added": nblocks <= SHARD_CUTS[0] + 2,
        "carry added last": nblocks <= SHARD_CUTS[0] + 2,
    }[order]


NEVER_DIFFERENT = ("restart every 8192 sites (total + chunk either way)",
                   "the order of combine_parts_kernel (the partial sums of one block are exact in any order)")


def different_cells(a, b):
    return int(np.sum(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)))


# ---- the text form ----------------------------------------------------------------------------------------------------------------------
def beagle_text(L):
    """The matrix as six-decimal Beagle text (every likelihood is 0 or 1: 0.000000, 1.000000 and the third 1 - g0 - g1)."""
    m, n = L.shape[0], L.shape[1] // 2
    g0, g1 = L[:, 0::2].astype(np.int64), L[:, 1::2].astype(np.int64)
    assert ((g0 == L[:, 0::2]) & (g1 == L[:, 1::2]) & (g0 >= 0) & (g1 >= 0) & (g0 + g1 <= 1)).all()
    v = np.stack([g0, g1, 1 - g0 - g1], axis=2).reshape(m, 3 * n)
    txt = np.empty((m, 3 * n, 9), dtype=np.uint8)
    txt[:] = np.frombuffer(b"\t0.000000", dtype=np.uint8)
    txt[:, :, 1] += v.astype(np.uint8)
    rows = txt.reshape(m, 27 * n)
    head = "marker\tallele1\tallele2" + "".join("\tInd%d\tInd%d\tInd%d" % (i, i, i) for i in range(n)) + "\n"
    return head.encode() + b"".join(b"chr1_%d\tA\tC" % (s + 1) + rows[s].tobytes() + b"\n" for s in range(m))


def parse_text(text):
    """(m, 2n) float32 from Beagle text: the first two of every three likelihoods, through Python's float."""
    lines = text.decode().splitlines()[1:]
    vals = np.array([[float(t) for t in line.split("\t")[3:]] for line in lines], dtype=np.float64).astype(F32)
    n = vals.shape[1] // 3
    L = np.empty((len(lines), 2 * n), dtype=F32)
    L[:, 0::2], L[:, 1::2] = vals[:, 0::3], vals[:, 1::3]
    return L
