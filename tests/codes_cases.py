"""Enumerated key sets for the class encoder (csrc/codes_kernels.hip: class_encode_kernel) -- the statement of its contract.

The encoder's limits all meet in one kernel: T hash slots per SNP (64 / 128 / 256 = 16 / 8 / 4 SNPs per wavefront), ENC_RMAX
probe rounds per buffer, 254 classes, the dictionary's rows (drows), the rows of a slab's own dictionary (lrows), the one bit
pattern used as KEY_EMPTY, and 616 classes per aligned group of SNPs of the coded scoring sweep.  Generator output never comes
near any of them, so the matrices here are built key by key: probe chains of known length (the kernel's hash is restated below),
class counts on both sides of every limit, classes that first appear at the very end of a slab, keys that differ in one bit.
NumPy only: tests/test_codes_cases_cpu.py holds this file to its own claims, tests/test_gpu_encoder.py holds the encoder to them.

A matrix is laid out for the encoder's tiles of 64 SNPs.  Every adversarial SNP stands between plain low-depth SNPs (expectation
`coded`: nothing about a rich SNP may affect the others) and every case stands at each of POSITIONS -- the first and last SNP of
a tile and of a wavefront's share of it, for all three geometries -- and in the last, partial tile.

What the sample pass (csrc/codes.hip: wgs_beagle_codes_plan) makes of a matrix is part of its layout: a matrix is coded at all only
while fewer than 1 % of its SNPs have 200 classes or more, and the dictionary gets its full T - T/8 rows only when more than 0.1 %
of them have 250 or more.  Matrices are therefore padded with plain tiles, and carry a few `ballast` SNPs of 256 classes.

The ORDER of a SNP's classes is the kernel's own business wherever two lanes share the SNP; order_matrix() is the one place where it
is well defined, and stated."""
import functools

import numpy as np

import synth

ENC_SLOTS = 1024            # hash slots per wavefront
ENC_UQ = 2                  # quads per lane and buffer
ENC_RMAX = 24               # probe rounds per buffer before a SNP is given up as rich
MAX_CLASSES = 254
BATCH_ROWS_CAP = 616        # classes an aligned group of score_batch SNPs may sum to
GEOMETRIES = (64, 128, 256)
KEY_EMPTY_WORD = 0xFFFFFFFF
# first / last SNP of a tile (0, 63), of a share of 16 SNPs (16, 47), of 8 (56, 7), of 4 (36, 27): no two adjacent, two per aligned 16
POSITIONS = (0, 7, 16, 27, 36, 47, 56, 63)
PLAIN_CLASSES = 6           # most classes of a plain SNP
EMPTY_SLAB = 3


class Geometry:
    def __init__(self, T, slab_sizes=None):
        self.T = T
        self.snps = ENC_SLOTS // T                 # SNPs per wavefront
        self.cols = 64 // self.snps                # lanes per SNP
        self.buffer = 4 * self.cols * ENC_UQ       # individuals per buffer: 32, 64, 128
        self.hshift = 32 - T.bit_length() + 1
        self.drows = min(MAX_CLASSES, T - T // 8)  # rows of the dictionary once the sample pass has seen SNPs of 250 classes
        self.score_batch = self.snps               # SNPs per table of the coded scoring sweep the group matrix is built for
        # populations: a large one (256 classes need that many individuals), 1, one below a buffer, none, 3, one above a buffer, 4, 5
        self.slab_sizes = slab_sizes or (260, 1, self.buffer - 1, 0, 3, self.buffer + 1, 4, 5)
        self.slab_start = np.concatenate([[0], np.cumsum(self.slab_sizes)]).astype(np.int64)
        self.n = int(self.slab_start[-1])
        self.labels = np.repeat(np.arange(len(self.slab_sizes)), self.slab_sizes).astype(np.int32)

    def limit(self):
        return min(self.T, self.drows, MAX_CLASSES)


# ---- the kernel's hash, restated
_M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def rotl32(x, r):
    x = _u64(x)
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & _M32


def umul24(a, b):
    """__umul24: the low 32 bits of the product of the low 24 bits of each operand"""
    return ((_u64(a) & np.uint64(0xFFFFFF)) * (_u64(b) & np.uint64(0xFFFFFF))) & _M32


def hash32(g0, g1):
    x = _u64(g0) ^ rotl32(g1, 13)
    return umul24(x, 0x9E3779) ^ rotl32(umul24(x >> np.uint64(8), 0x85EBCB), 3)


def home_slot(g0, g1, T):
    return (hash32(g0, g1) >> np.uint64(Geometry(T).hshift)).astype(np.int64)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ---- keys a Beagle file can hold: (k0 / 10^6, k1 / 10^6) as float32, k0 + k1 <= 10^6
@functools.lru_cache(maxsize=None)
def key_pool():
    rng = np.random.Generator(np.random.PCG64(20261019))
    k0 = rng.integers(0, 1_000_001, size=600_000)
    k1 = rng.integers(0, 1_000_001, size=600_000)
    ok = k0 + k1 <= 1_000_000
    pairs = np.unique(np.stack([k0[ok], k1[ok]], axis=1), axis=0)
    pairs = pairs[rng.permutation(len(pairs))]
    g0, g1 = bits(pairs[:, 0] / 1e6), bits(pairs[:, 1] / 1e6)
    return g0, g1, home_slot(g0, g1, 256)


@functools.lru_cache(maxsize=None)
def buckets(T):
    """per home slot of a T-slot table: the pool's keys with that home (indices into key_pool())"""
    home = key_pool()[2] // (256 // T)             # hash >> (32 - log2 T)
    order = np.argsort(home, kind="stable")
    cuts = np.searchsorted(home[order], np.arange(T + 1))
    return [order[cuts[h]:cuts[h + 1]] for h in range(T)]


def keys_at(T, h, c, skip=0):
    """c pool keys whose home slot in a T-slot table is h"""
    idx = buckets(T)[h][skip:skip + c]
    assert len(idx) == c
    g0, g1, _ = key_pool()
    return g0[idx], g1[idx]


def keys_spread(T, c, first=0):
    """c pool keys with c different home slots (c <= T): no lookup of such a SNP ever probes twice"""
    hs = (first + np.arange(c) * 1) % T if c > T // 2 else (first + np.arange(c) * (T // c)) % T
    g0, g1, _ = key_pool()
    idx = np.array([buckets(T)[h][1] for h in hs])
    return g0[idx], g1[idx]


def keys_random(c, seed):
    """c distinct pool keys wherever they hash"""
    g0, g1, _ = key_pool()
    idx = np.random.Generator(np.random.PCG64(seed)).choice(len(g0), size=c, replace=False)
    return g0[idx], g1[idx]


class Row:
    """one SNP: the class of every individual (ids into the key list), its case name and expectation"""

    def __init__(self, name, keys, ids, expect, **facts):
        self.name, self.expect, self.facts = name, expect, facts
        self.g0, self.g1 = np.asarray(keys[0], dtype=np.uint32)[ids], np.asarray(keys[1], dtype=np.uint32)[ids]


def expectation_of_count(G, c):
    """rich beyond min(T, drows, 254) classes; below, long probe runs are legitimate while the table is more than a quarter full"""
    if c > G.limit():
        return "rich"
    return "either" if c > G.T // 4 else "coded"


def slab_range(G, g):
    return int(G.slab_start[g]), int(G.slab_start[g + 1])


# ---- the cases
CHAIN_LENGTHS = (2, 8, 16, 24, 25, 26, 40)
CHAIN_HOMES = ("mid", "last", "last2")             # slot 5, T - 1, T - 2: the last two wrap to slot 0
# the keys first met in one buffer; at even distances over the first slab (in different buffers while there are no more keys than the
# slab has buffers -- 9, 5 or 3 by geometry -- and several to a buffer beyond that); dealt over the slabs in turn
CHAIN_SPREADS = ("buffer", "first_slab", "slabs")


def slab_buffers(G, g):
    """buffers in the walk of slab g"""
    return -(-((G.slab_sizes[g] + 3) // 4) // (G.cols * ENC_UQ))


def chain_row(G, c, home, spread):
    h = {"mid": 5, "last": G.T - 1, "last2": G.T - 2}[home]
    g0, g1 = keys_at(G.T, h, c)
    ids = np.zeros(G.n, dtype=np.int64)            # everybody else holds the chain's first key
    if spread == "buffer":
        ids[:c] = np.arange(c)                     # the first c individuals of the first slab
    elif spread == "first_slab":
        ids[(np.arange(c) * 260) // c] = np.arange(c)
    else:
        slabs = [g for g, s in enumerate(G.slab_sizes) if s]
        used = {g: 0 for g in slabs}
        j, turn = 0, 0
        while j < c:
            g = slabs[turn % len(slabs)]
            turn += 1
            if used[g] < G.slab_sizes[g]:
                ids[G.slab_start[g] + used[g]] = j
                used[g] += 1
                j += 1
    return Row("chain_%d_%s_%s" % (c, home, spread), (g0, g1), ids, "coded" if c <= ENC_RMAX else "either", chain=c, spread=spread, home=h)


def chain_cases(G):
    return [chain_row(G, c, home, spread) for spread in CHAIN_SPREADS for home in CHAIN_HOMES for c in CHAIN_LENGTHS]


def lane_cases(G):
    """several lanes, one new key"""
    B = G.buffer
    a0, a1 = keys_at(G.T, 9, 2)
    b0, b1 = keys_at(G.T, 40, 1)
    keys = (np.concatenate([b0, a0]), np.concatenate([b1, a1]))      # 0: the background, 1 and 2: two keys with one home slot
    rows = []
    ids = np.zeros(G.n, dtype=np.int64)
    ids[2 * B + 4:2 * B + 8] = 1                   # one new key in all four individuals of a quad of the third buffer
    rows.append(Row("lanes_new_key_fills_a_quad", keys, ids, "coded"))
    ids = np.zeros(G.n, dtype=np.int64)
    ids[B:2 * B] = 1                               # ... in every quad of the second buffer: every lane of the SNP inserts it at once
    rows.append(Row("lanes_new_key_fills_a_buffer", keys, ids, "coded"))
    ids = np.zeros(G.n, dtype=np.int64)
    ids[B:2 * B] = 1 + (np.arange(B) // 4) % 2     # two new keys with one home slot, in alternate quads of one buffer
    rows.append(Row("lanes_two_new_keys_one_home", keys, ids, "coded"))
    return rows


def limit_counts(G):
    T = G.T
    return sorted({T, T + 1, T - T // 8, T - T // 8 + 1, T // 4, T // 4 + 1, 8, 9, 16, 17, 24, 25, 63, 64, 65, 127, 128, 129, 253, 254, 255, 256})


def count_row(G, c, name=None):
    """c classes, all of them in the first slab (one individual each, then the first few again); the other slabs hold the first three"""
    keys = keys_random(c, 1000 + c)
    ids = np.arange(G.n, dtype=np.int64) % min(c, 3)
    ids[:260] = np.arange(260) % min(c, 4)
    ids[:min(c, 260)] = np.arange(min(c, 260))
    return Row(name or "count_%d" % c, keys, ids, expectation_of_count(G, c), count=c)


def limit_cases(G):
    """Random keys probe, and at 7/8 load a random set may run past ENC_RMAX rounds: count_<drows> is `either`, and the 128- and 256-slot
    tables do give it up.  One more row therefore holds exactly drows classes whose keys have home slots of their own: no lookup probes
    twice, so it must be coded -- the dictionary's last row is usable, `ncls > drows` and not `>=`."""
    rows = [count_row(G, c) for c in limit_counts(G)]
    c = G.drows
    ids = np.arange(G.n, dtype=np.int64) % 3
    ids[:260] = np.arange(260) % c
    rows.append(Row("count_%d_spread" % c, keys_spread(G.T, c, first=11), ids, "coded", count=c, own_homes=True))
    return rows


def appear_cases(G):
    """where a class first appears"""
    rows = []
    base = keys_random(5, 77)
    new = keys_random(3, 78)
    keys = (np.concatenate([base[0], new[0]]), np.concatenate([base[1], new[1]]))     # 0 .. 4: met early by everybody; 5, 6, 7: new
    common = np.arange(G.n, dtype=np.int64) % 5
    for g, size in enumerate(G.slab_sizes):
        if size == 0 or g == 0:
            continue
        ids = common.copy()
        ids[G.slab_start[g + 1] - 1] = 5
        last = g == len(G.slab_sizes) - 1
        rows.append(Row("appear_last_of_slab_of_%d%s" % (size, "_and_matrix" if last else ""), keys, ids, "coded"))
    # a quad straddling a slab's end: the slab one below a buffer ends inside its last quad, the next populated slab begins with a new class too
    ids = common.copy()
    ids[G.slab_start[3] - 2:G.slab_start[3]] = (5, 6)
    ids[G.slab_start[4]] = 7
    rows.append(Row("appear_in_a_quad_straddling_a_slab_end", keys, ids, "coded"))
    # the first individual after the empty slab
    ids = common.copy()
    ids[G.slab_start[EMPTY_SLAB + 1]] = 5
    rows.append(Row("appear_after_an_empty_slab", keys, ids, "coded"))
    # a slab that meets only classes numbered 64 or higher: the first 64 individuals of the first slab hold 64 classes of their own, its
    # second buffer brings 16 more (classes are numbered buffer by buffer), and the slab one above a buffer holds only those 16
    c = 80
    hk = keys_random(c, 79)
    ids = np.arange(G.n, dtype=np.int64) % 4
    ids[:64] = np.arange(64)
    ids[max(G.buffer, 64):max(G.buffer, 64) + 16] = 64 + np.arange(16)
    a, b = slab_range(G, 5)
    ids[a:b] = 64 + np.arange(b - a) % 16
    rows.append(Row("appear_slab_of_high_classes_only", hk, ids, expectation_of_count(G, c), count=c))
    return rows


def bit_cases(G):
    rows = []
    a, b = bits(0.333333), bits(0.25)
    alt = np.arange(G.n, dtype=np.int64) % 2
    rows.append(Row("bits_lowest_mantissa_bit_of_g0", (np.array([a, a ^ 1]), np.array([b, b])), alt, "coded"))
    rows.append(Row("bits_lowest_mantissa_bit_of_g1", (np.array([a, a]), np.array([b, b ^ 1])), alt, "coded"))
    rows.append(Row("bits_swapped_pair", (np.array([a, b]), np.array([b, a])), alt, "coded"))
    z, nz = 0x00000000, 0x80000000
    four = np.arange(G.n, dtype=np.int64) % 4
    rows.append(Row("bits_signed_zeros", (np.array([z, nz, z, nz]), np.array([z, z, nz, nz])), four, "coded"))
    nans = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, KEY_EMPTY_WORD, a])
    other = np.array([b, b, b, b, 0x7FC00000, KEY_EMPTY_WORD])
    rows.append(Row("bits_nan_payloads", (nans, other), np.arange(G.n, dtype=np.int64) % 6, "coded"))
    ids = four.copy()
    ids[G.buffer + 5] = 4                          # one individual holds KEY_EMPTY; slot 0 is its home, and a later key's too
    e0, e1 = keys_at(G.T, 0, 1)
    k0, k1 = keys_random(4, 80)
    ids[3 * G.buffer + 2] = 5
    rows.append(Row("bits_key_empty", (np.concatenate([k0, [KEY_EMPTY_WORD], e0]), np.concatenate([k1, [KEY_EMPTY_WORD], e1])), ids, "rich", sample_rich=True))
    return rows


def group_rows(G):
    """The scoring group rule: aligned groups of score_batch SNPs whose classes sum to exactly BATCH_ROWS_CAP (all stay coded), to
    one more (the richest goes rich, and only it), and to one more with the largest count held by three SNPs (the first of them goes).
    Every SNP's keys have home slots of their own, so none of them can go rich for its probes.  Returns {kind: [Row]}."""
    batch = G.score_batch
    base = BATCH_ROWS_CAP // batch                 # 38, 77, 154
    exact = [base] * batch
    exact[batch // 2] += BATCH_ROWS_CAP - base * batch
    over = list(exact)
    over[batch // 2] += 1
    top = base + 3
    rest, left = batch - 3, BATCH_ROWS_CAP + 1 - 3 * top
    others = [left // rest + (1 if i < left % rest else 0) for i in range(rest)]
    assert max(others) < top and min(others) > 0
    tops = (1, batch - 2, batch - 1)               # the lowest lane of the three is the one that goes
    tie = [top if i in tops else others.pop(0) for i in range(batch)]
    assert sum(exact) == BATCH_ROWS_CAP and sum(over) == sum(tie) == BATCH_ROWS_CAP + 1 and len(tie) == batch
    out = {}
    for kind, counts in (("exact", exact), ("over", over), ("tie", tie)):
        rows = []
        victim = None if kind == "exact" else int(np.argmax(counts))
        for i, c in enumerate(counts):
            keys = keys_spread(G.T, c, first=7 * i)
            ids = np.arange(G.n, dtype=np.int64) % c
            rows.append(Row("group_%s" % kind, keys, ids, "rich" if i == victim else "coded", count=c, group=kind))
        out[kind] = rows
    return out


def plain_row(G, rng):
    keys = keys_spread(G.T, PLAIN_CLASSES, first=int(rng.integers(0, G.T)))
    c = int(rng.integers(2, PLAIN_CLASSES + 1))
    return Row("plain", keys, rng.integers(0, c, size=G.n), "coded")


def ballast_row(G):
    return count_row(G, 256, "ballast")


def heavy(row):
    """what the sample pass may count as 200 classes or more (it walks every SNP through a 256-slot table)"""
    return row.facts.get("count", 0) >= 200 or row.facts.get("chain", 0) > ENC_RMAX or row.facts.get("sample_rich", False)


class Matrix:
    def __init__(self, name, G, rows, where):
        self.name, self.G, self.m, self.n = name, G, len(rows), G.n
        self.labels = G.labels
        self.L = np.empty((self.m, 2 * G.n), dtype=np.float32)
        Lb = self.L.view(np.uint32)
        for i, r in enumerate(rows):
            Lb[i, 0::2] = r.g0
            Lb[i, 1::2] = r.g1
        self.names = np.array([r.name for r in rows])
        self.expect = np.array([r.expect for r in rows])
        self.facts = [r.facts for r in rows]
        self.where = where                            # per SNP: "tile" (one of POSITIONS), "partial" (the last tile) or "" (plain, ballast)
        self.counts = synth.classes_per_snp(self.L)
        self.slab_counts = np.zeros((self.m, len(G.slab_sizes)), dtype=np.int64)
        for g, size in enumerate(G.slab_sizes):
            if size:
                a, b = slab_range(G, g)
                self.slab_counts[:, g] = synth.classes_per_snp(self.L[:, 2 * a:2 * b])

    def digest(self):
        return synth.digest(self.L)


def assemble(name, G, cases, seed):
    """Tile t holds case t at every one of POSITIONS; the last tile (m % 64 != 0) holds every case once more, one in four SNPs;
    plain SNPs everywhere else.  Plain tiles and ballast SNPs are added until the sample pass codes the matrix with drows = T - T/8."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nc = len(cases)
    assert nc <= 16
    case_tiles = nc                                   # a tile per case: what the case does to its tile (tile_rows) is its own doing
    seats_full = [(64 * t + p, t) for t in range(case_tiles) for p in POSITIONS]
    placed = [j for _, j in seats_full] + list(range(nc))
    n_heavy = sum(heavy(cases[j]) for j in placed)
    n_sure = sum(cases[j].facts.get("count", 0) >= 250 for j in placed)
    tiles = case_tiles
    while True:
        m = 64 * (tiles + 1) + 63
        n_ballast = max(0, m // 1000 + 2 - n_sure)
        assert n_ballast <= 8
        if (n_heavy + n_ballast) * 100 < m - 100:
            break
        tiles += 1
    rows = [None] * m
    where = np.array([""] * m, dtype=object)
    for at, j in seats_full:
        rows[at] = cases[j]
        where[at] = "tile"
    for i in range(n_ballast):                         # in the tile before the last: positions of their own
        rows[64 * tiles + 9 + 16 * (i % 4) + 2 * (i // 4)] = ballast_row(G)
    # the last tile: 63 SNPs, cases at 1, 5, 9 ... -- four per aligned 16, heaviest with lightest, so no group exceeds BATCH_ROWS_CAP
    order = sorted(range(nc), key=lambda j: -cases[j].facts.get("count", 0))
    seats = [[] for _ in range(4)]
    for k, j in enumerate(order):
        seats[k % 4 if (k // 4) % 2 == 0 else 3 - k % 4].append(j)
    for q, members in enumerate(seats):
        assert len(members) <= 4 and sum(cases[j].facts.get("count", 8) for j in members) + 12 * PLAIN_CLASSES <= BATCH_ROWS_CAP
        for k, j in enumerate(members):
            rows[64 * (tiles + 1) + 16 * q + 1 + 4 * k] = cases[j]
            where[64 * (tiles + 1) + 16 * q + 1 + 4 * k] = "partial"
    for i in range(m):
        if rows[i] is None:
            rows[i] = plain_row(G, rng)
    return Matrix(name, G, rows, where)


def assemble_groups(G, seed):
    """The group-rule matrix: a tile per kind of group, which holds it in its first and in its last aligned group; all three in the
    last, partial tile; plain tiles until the sample pass chooses score_batch = G.score_batch and a dictionary that holds every SNP."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kinds = group_rows(G)
    names = ("exact", "over", "tie")
    batch = G.score_batch
    tiles, part = 31, 3 * batch + 2
    m = 64 * tiles + part
    rows = [None] * m
    where = np.array([""] * m, dtype=object)
    for t in range(3):
        for at, kind in ((0, names[t]), (64 - batch, names[t])):
            for i, r in enumerate(kinds[kind]):
                rows[64 * (2 * t + 1) + at + i] = r
                where[64 * (2 * t + 1) + at + i] = "tile"
    for k, kind in enumerate(names):
        for i, r in enumerate(kinds[kind]):
            rows[64 * tiles + k * batch + i] = r
            where[64 * tiles + k * batch + i] = "partial"
    for i in range(m):
        if rows[i] is None:
            rows[i] = plain_row(G, rng)
    return Matrix("groups", G, rows, where)


# ---- the order of the classes.  Classes are numbered in order of appearance, but which of two lanes of a SNP meets a class first is
# the kernel's own business -- except where all of a SNP's individuals fall in ONE lane's walk.  A slab of at most 4 individuals is one
# quad, quad 0 is column 0's, and a lane takes its lookups in the order of the individuals and the slabs in their order: in a matrix of
# such slabs only, individual i's code is the number of distinct bit patterns among the individuals before the first one that holds i's.
ORDER_SLABS = (4, 1, 3, 0, 2, 4, 4)
ORDER_M = 7 * 64 + 37


def first_appearance(L):
    """(m, 2n) float32 -> (m, n): per SNP the rank of every individual's (g0, g1) bit pattern in order of first appearance"""
    Lb = np.asarray(L).view(np.uint32)
    key = Lb[:, 0::2].astype(np.uint64) | (Lb[:, 1::2].astype(np.uint64) << np.uint64(32))
    out = np.zeros(key.shape, dtype=np.int64)
    for i, row in enumerate(key.tolist()):
        rank = {}
        out[i] = [rank.setdefault(k, len(rank)) for k in row]
    return out


def order_rows(G):
    """What a single lane can meet: every individual a new class (18 keys with home slots of their own; 18 with ONE home slot, T - 2, so
    that each is found a probe later than the one before, past slot T - 1), one class, a new class in the matrix's last individual,
    returns to earlier classes between new ones, and random walks over keys of which half share a home slot."""
    n = G.n
    spread, chain = keys_spread(G.T, n, first=3), keys_at(G.T, G.T - 2, n)
    every = np.arange(n, dtype=np.int64)
    fixed = [Row("order_all_new", spread, every, "coded"), Row("order_all_new_one_home", chain, every, "coded", chain=n, home=G.T - 2),
             Row("order_one_class", spread, 0 * every, "coded"), Row("order_new_in_the_last", spread, every // (n - 1), "coded"),
             Row("order_returns", chain, np.array([0, 1, 0, 2, 2, 1, 3, 0, 4, 3, 5, 5, 1, 6, 0, 7, 6, 8]), "coded")]
    rows = []
    for i in range(ORDER_M):                           # seven kinds of row, seven full tiles: every kind stands at every SNP of a tile
        kind = (i % 64 + i // 64) % 7
        if kind < len(fixed):
            rows.append(fixed[kind])
            continue
        rng = np.random.Generator(np.random.PCG64(500 + i))
        c = int(rng.integers(2, 13))
        pick = rng.permutation(12)[:c]                 # of 6 keys with one home slot and 6 with their own
        keys = (np.concatenate([chain[0][:6], spread[0][:6]])[pick], np.concatenate([chain[1][:6], spread[1][:6]])[pick])
        rows.append(Row("order_random", keys, rng.integers(0, c, size=n), "coded"))
    return rows


@functools.lru_cache(maxsize=None)
def order_matrix(T):
    """The matrix of ORDER_SLABS for a T-slot table; `.rank` is the code every individual must get.  Read-only."""
    G = Geometry(T, ORDER_SLABS)
    M = Matrix("order", G, order_rows(G), np.array([""] * ORDER_M, dtype=object))
    M.rank = first_appearance(M.L)
    M.L.setflags(write=False)
    return M


# ---- chains the sample pass cannot hide.  A matrix is coded only while fewer than 1 % of its SNPs look rich to the sample pass, and the
# chain matrices of build() carry so many chains that an encoder which gives up too early -- fewer probe rounds, a probe that does not
# wrap -- fails them only by declining to code them at all.  Here the longest chains that must be coded (ENC_RMAX keys in one buffer;
# 16 keys whose home is the table's last slot) stand in 8 of 997 SNPs: the matrix is coded whatever becomes of them, and they answer
# for themselves.
SPARSE_M = 15 * 64 + 37
SPARSE_SEATS = (0, 3 * 64 + 63, 5 * 64 + 16, 7 * 64 + 47, 9 * 64 + 36, 11 * 64 + 7, 15 * 64 + 1, 15 * 64 + 36)


@functools.lru_cache(maxsize=None)
def sparse_chain_matrix(T):
    G = Geometry(T)
    rng = np.random.Generator(np.random.PCG64(600))
    cases = [chain_row(G, ENC_RMAX, "mid", "buffer"), chain_row(G, 16, "last", "buffer"), chain_row(G, ENC_RMAX, "last2", "slabs"),
             chain_row(G, 16, "last", "first_slab")]
    rows = [plain_row(G, rng) for _ in range(SPARSE_M)]
    where = np.array([""] * SPARSE_M, dtype=object)
    for k, at in enumerate(SPARSE_SEATS):
        rows[at] = cases[k % len(cases)]
        where[at] = "partial" if at >= 64 * (SPARSE_M // 64) else "tile"
    M = Matrix("sparse_chains", G, rows, where)
    M.L.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def build(T):
    """The matrices of one geometry (T hash slots per SNP), in a fixed order.  Shared by the tests: read-only."""
    G = Geometry(T)
    out = []
    # at most 4 cases a matrix that the sample pass may count as rich (1 % of its SNPs), at most 12 cases in all, dealt round robin
    for name, cases, seed in (("chains", chain_cases(G), 100), ("limits", limit_cases(G), 200)):
        hard = [c for c in cases if heavy(c)]
        light = [c for c in cases if not heavy(c)]
        parts = max((len(hard) + 3) // 4, (len(cases) + 11) // 12)
        for k in range(parts):
            out.append(assemble("%s_%d" % (name, k), G, hard[k::parts] + light[k::parts], seed + k))
    out.append(assemble("edges_0", G, lane_cases(G) + appear_cases(G), 300))
    out.append(assemble("edges_1", G, bit_cases(G), 301))
    out.append(assemble_groups(G, 400))
    for M in out:
        M.L.setflags(write=False)
    return tuple(out)
