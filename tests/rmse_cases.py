"""Enumerated inputs for the block-parallel emulation of the reference's serial float32 convergence sum (csrc/em_kernels.hip:
rmse_block_sum_kernel, rmse_predict_kernel, rmse_candidates_kernel with chain_step, rmse_walk_kernel, chain_set_carry_kernel), built for
what random vectors never reach: the candidates of the neighbouring binades, every shift and remainder class of chain_step at both
entry parities, subnormal, infinite and NaN squares and carries, and the loop shapes of the walk and of the prediction.  NumPy and
Python integers only; the twin of tests/em_cases.py, tests/fisher_cases.py and tests/score_cases.py.

A CASE is (a, b, carry): the chain is  res = carry; res = res + (a[i] - b[i]) * (a[i] - b[i])  in float32 and index order
(emMAF_cy.pyx:30-31).  A wanted square is reachable only as such a product: root() finds a float32 d with fl(d * d) equal to it --
d * d is monotone in d, so the neighbours of sqrt are an exhaustive search -- and a class none of whose members has a root is listed
as unreachable (grid_classes()).  Where it is exact, a = 2d and b = d, so that the subtraction is not idle.

THE TRUTH of a case (truth()) mirrors nothing of the kernels:
    entries, final   the float32 running value at every block entry and at the end: np.add.accumulate in float32, strictly serial
    expo             the biased exponent predicted for block k: the EXACT sum (Python integers) of carry and all earlier squares, rounded
                     to float32; -1 for an all-zero block; 0 where the block's or an earlier block's sum is NaN and where the prefix
                     rounds to a zero, subnormal or infinite float32
    cand             per block and candidate exponent expo - 1, expo, expo + 1, for an even and an odd entry mantissa: the integer by
                     which the block moves a mantissa on the grid u = 2^(exponent - 150) -- M <- RN_even(M + d / u) term after term --
                     saturated at 2^40; a block with a NaN or infinite square and an exponent outside 1 .. 254 do not fit (2^40).
                     increment_by_definition() is that sentence in Fractions; increments() gives the same numbers quickly (terms that
                     are no tie are rounded on their own and summed, the ties are resolved in order) and the CPU test holds the two
                     together and both to the literal float32 chain
    serial           the NECESSARY serial blocks, from the reference chain alone: non-zero blocks whose entry is no positive normal
                     number, whose entry and exit exponents differ, that hold a term that is not finite, whose predicted exponent is 0
                     or more than one away from the entry's
    margin           the smallest relative distance of an exact prefix from a power of two and from the float32 overflow limit, over the
                     block starts where the order of the device's float64 additions could matter at all (not where every partial sum is
                     exact in float64 whatever the order: all terms multiples of 2^g and the total below 2^(g + 53))

THE FAMILIES: term_grid(be, parity), and cases() of ahead, behind, edges, long, hostile, carries; jobs() batches cases of the others.
See each builder."""
import functools
import hashlib
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
RB = 4096                         # elements per block (csrc/em_kernels.hip: RB)
SAT = 1 << 40                     # "does not fit"
INF, NAN = float("inf"), float("nan")
GRID_BE = (1, 2, 3, 24, 25, 100, 127, 150, 253, 254)
MARGIN = 2.0 ** -40               # what the CPU test asks of truth()["margin"]
ONE, TOP = 1 << 23, 1 << 24


# ---------------------------------------------------------------------------------------------------------------- float32 helpers
def from_bits(u):
    return np.array(u, dtype=np.uint32).view(F32)[()]


def bits(x):
    return int(np.array(x, dtype=F32).view(np.uint32))


def make(be, mant):
    """The positive float32 with biased exponent be (1 .. 254) and 24-bit mantissa mant (hidden bit included)."""
    assert 1 <= be <= 254 and ONE <= mant < TOP
    return from_bits((be << 23) | (mant & 0x7FFFFF))


def exponent(x):
    return (bits(x) >> 23) & 0xFF


def mantissa(x):
    return (bits(x) & 0x7FFFFF) | ONE


def positive_normal(x):
    return bits(x) >> 31 == 0 and 1 <= exponent(x) <= 254


def nblocks(m):
    return (m + RB - 1) // RB


def squares(a, b):
    with np.errstate(all="ignore"):
        d = np.subtract(a, b, dtype=F32)
        return np.multiply(d, d, dtype=F32)


def root(T):
    """A positive float32 d with fl(d * d) == T, or None.  d * d does not decrease with d, so if the seven floats around sqrt(T) miss T
    every float does: the search is exhaustive."""
    T = F32(T)
    if not (T > 0) or not np.isfinite(T):
        return None
    d0 = F32(math.sqrt(float(T)))
    near, lo, hi = [d0], d0, d0
    for _ in range(3):
        lo, hi = np.nextafter(lo, F32(0)), np.nextafter(hi, F32(INF))
        near += [lo, hi]
    with np.errstate(all="ignore"):
        for d in near:
            if d > 0 and np.multiply(d, d, dtype=F32) == T:
                return F32(d)
    return None


def ulps(x, E):
    """The float32 x * 2^(E - 150) -- x units of the grid of biased exponent E -- or None where that is no float32."""
    v = Fraction(x) * Fraction(2) ** (E - 150)
    if v >= Fraction(2) ** 128:
        return None
    f = F32(float(v))
    return f if Fraction(float(f)) == v else None


# ---------------------------------------------------------------------------------------------------------------- the truth
def reference_chain(sq, carry):
    """(float32 value at every block entry, final value) of the strict serial float32 accumulation."""
    with np.errstate(all="ignore"):
        acc = np.add.accumulate(np.concatenate((np.array([carry], dtype=F32), sq)), dtype=F32)
    return acc[np.arange(nblocks(len(sq))) * RB].copy(), acc[-1]


def decompose(sq):
    """finite sq = im * 2^(shift - 172) with im = 0 or 2^23 <= im < 2^24 (int64 arrays), and the mask of the finite ones."""
    fin = np.isfinite(sq)
    mant, ex = np.frexp(np.where(fin, sq, 0).astype(np.float64))
    im = np.rint(mant * 2.0 ** 24).astype(np.int64)
    return im, np.where(im > 0, ex.astype(np.int64) + 148, 0), fin


def as_units(x):
    """The finite float32 x >= 0 as an integer multiple of 2^-172."""
    v = Fraction(float(x)) * (1 << 172)
    assert v.denominator == 1 and v >= 0
    return int(v)


def rounded_exponent(P):
    """Biased exponent of the float32 nearest P * 2^-172 (0: zero, subnormal or infinite).  Within 2^-25 of a limit the answer depends
    on the rounding; the cases stay 2^-40 and more away from them, and where they do not, every sum is exact."""
    if P <= 0:
        return 0
    L = P.bit_length()
    if L > 24:
        q, r = divmod(P, 1 << (L - 24))
        half = 1 << (L - 25)
        if r > half or (r == half and q & 1):
            q += 1
        if q == TOP:
            L += 1
    e = L - 46                                 # 2^(L-1) * 2^-172 = 2^(e - 127)
    if e <= 0:                                 # on the subnormal grid of 2^-149 = 2^23 units: FLT_MIN where it rounds up to 2^23 of them
        q, r = divmod(P, ONE)
        return 1 if q + (r > ONE // 2 or (r == ONE // 2 and q & 1)) >= ONE else 0
    return e if e <= 254 else 0


def edge_margin(P):
    L = P.bit_length()
    d = min(P - (1 << (L - 1)), (1 << L) - P, abs(P - ((1 << 300) - (1 << 275))))      # 2^128 - 2^103: where float32 overflows
    return d / P


def increments(im, shift, bad, E, want_ties=False):
    """(increment for an even, for an odd entry mantissa) of the block whose non-zero finite squares are im * 2^(shift - 172), in order,
    on the grid of biased exponent E; bad: the block holds a square that is not finite."""
    if bad or not 1 <= E <= 254:
        return (SAT, SAT, 0) if want_ties else (SAT, SAT)
    if len(im) == 0:
        return (0, 0, 0) if want_ties else (0, 0)
    t = E + 22 - shift                                        # d / u = im * 2^-t
    if (t <= -17).any():                                      # im >= 2^23: at least 2^40
        return (SAT, SAT, 0) if want_ties else (SAT, SAT)
    whole = t <= 0
    tt = np.clip(t, 1, 62)
    q = np.where(whole, im << np.clip(-t, 0, 16), im >> tt)
    rem = np.where(whole, 0, im & ((np.int64(1) << tt) - 1))
    half = np.where(whole, 1, np.int64(1) << (tt - 1))
    base = q + (rem > half)
    tie = rem == half
    before = np.concatenate(([0], np.cumsum(base)))
    out = []
    for p in (0, 1):
        extra = 0
        for i in np.flatnonzero(tie):
            extra += (p + int(before[i]) + extra + int(q[i])) & 1         # RN_even(M + q + 1/2): up where M + q is odd
        out.append(min(int(before[-1]) + extra, SAT))
    return (out[0], out[1], int(tie.sum())) if want_ties else tuple(out)


def increment_by_definition(sq_block, E, p):
    """The sentence of the module docstring in Fractions: M <- round_half_even(M + d / u) from a mantissa of parity p."""
    if not 1 <= E <= 254 or not np.isfinite(sq_block).all():
        return SAT
    u = Fraction(2) ** (E - 150)
    M = M0 = ONE + p
    for d in sq_block[sq_block != 0]:
        M = round(M + Fraction(float(d)) / u)                 # Python rounds a Fraction half to even
        if M - M0 >= SAT:
            return SAT
    return M - M0


def truth(a, b, carry):
    sq = squares(a, b)
    m, nb = len(sq), nblocks(len(sq))
    entries, final = reference_chain(sq, F32(carry))
    im, shift, fin = decompose(np.concatenate((sq, np.zeros(nb * RB - m, dtype=F32))))
    sqp = np.concatenate((sq, np.zeros(nb * RB - m, dtype=F32))).reshape(nb, RB)
    im, shift = im.reshape(nb, RB), shift.reshape(nb, RB)
    has_nan, has_inf = np.isnan(sqp).any(axis=1), np.isinf(sqp).any(axis=1)
    w = np.bincount((np.arange(nb)[:, None] * 512 + shift).ravel(), weights=im.ravel().astype(np.float64), minlength=nb * 512).reshape(nb, 512)
    sums = [sum(int(w[k, s]) << int(s) for s in np.flatnonzero(w[k])) for k in range(nb)]
    low = np.where(im > 0, shift + np.log2(np.maximum(im & -im, 1)).astype(np.int64), 1 << 20).min(axis=1)   # the blocks' lowest set bit

    c = F32(carry)
    nan, inf = bool(np.isnan(c)), bool(np.isinf(c))
    run = 0 if nan or inf else as_units(c)
    g = (run & -run).bit_length() - 1 if run else 1 << 20
    expo, margin, added = np.zeros(nb, dtype=np.int32), INF, False
    for k in range(nb):
        if sums[k] == 0 and not has_nan[k] and not has_inf[k]:
            expo[k] = -1
            continue
        if not (nan or has_nan[k] or inf):
            expo[k] = rounded_exponent(run)
            if added and run > 0 and not run < 1 << (g + 53):
                margin = min(margin, edge_margin(run))
        nan, inf = nan or bool(has_nan[k]), inf or bool(has_inf[k])
        run, g, added = run + sums[k], min(g, int(low[k])), True

    cand = np.full((nb, 6), SAT, dtype=np.int64)
    ties = np.zeros((nb, 3), dtype=np.int64)
    for k in np.flatnonzero(expo > 0):
        nz = im[k] > 0
        for ci in range(3):
            cand[k, 2 * ci], cand[k, 2 * ci + 1], ties[k, ci] = increments(im[k][nz], shift[k][nz], bool(has_nan[k] or has_inf[k]), int(expo[k]) - 1 + ci, True)

    serial, applied = [], []
    for k in np.flatnonzero(expo != -1):
        entry, leave = entries[k], entries[k + 1] if k + 1 < nb else final
        be = exponent(entry)
        if (not positive_normal(entry) or be != exponent(leave) or has_nan[k] or has_inf[k] or expo[k] == 0 or abs(int(expo[k]) - be) > 1):
            serial.append(int(k))
        else:
            ci = be - int(expo[k]) + 1
            applied.append((int(k), ci, mantissa(entry) & 1, int(ties[k, ci])))
    return {"sq": sq, "entries": entries, "final": final, "expo": expo, "cand": cand, "serial": serial, "applied": applied, "margin": margin,
            "sums": sums, "nonfinite": has_nan | has_inf}


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, family, name, a, b, carry, **claims):
        self.family, self.name = family, name
        self.a, self.b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
        self.carry = F32(carry)
        self.claims = claims
        assert self.a.shape == self.b.shape and self.a.ndim == 1 and len(self.a) > 0
        for v in (self.a, self.b):
            v.setflags(write=False)

    @property
    def m(self):
        return len(self.a)

    @functools.cached_property
    def truth(self):
        return truth(self.a, self.b, self.carry)

    def __repr__(self):
        return "%s/%s" % (self.family, self.name)


def put(a, b, at, d, doubled):
    """square d * d at index `at`: (d, 0), or (2d, d) where that is exact."""
    d = F32(d)
    if doubled and np.isfinite(F32(2) * d) and F32(2) * d - d == d:
        a[at], b[at] = F32(2) * d, d
    else:
        a[at], b[at] = d, 0


# ---- term_grid -------------------------------------------------------------------------------------------------------------------
def class_mantissas(sh):
    """{remainder class: candidate 24-bit mantissas md, lowest first} of a normal square d = md * 2^(bd - 150) met by a chain at
    be = bd + sh: d / u = md * 2^-sh.  An empty list: the class does not exist at this shift."""
    if sh <= 0:
        return {"whole": list(range(ONE, ONE + 64)), "whole, all ones": [TOP - 1]}
    if sh >= 25:
        return {"absorbed": list(range(ONE, ONE + 64)), "absorbed, all ones": [TOP - 1]}
    half, mask = 1 << (sh - 1), (1 << sh) - 1
    rems = {"zero": [0], "below half": [r for r in (1, half - 1, half // 2 + 1) if 0 < r < half], "tie": [half],
            "above half": [r for r in (half + 1, mask - 1, half + half // 2 + 1) if half < r < mask], "all ones": [mask] if mask != half else []}
    his = range(ONE >> sh, min((ONE >> sh) + 64, 1 << (24 - sh)))
    return {name: sorted({(hi << sh) | r for hi in his for r in rs if ((hi << sh) | r) >= ONE}) for name, rs in rems.items()}


@functools.lru_cache(maxsize=None)
def grid_classes(be):
    """(classes, unreachable, absent) at entry exponent be: classes = [(name, d, weight)] with d * d the class's square and weight its
    size in units of the grid of be; unreachable = names none of whose candidates is a float32 product d * d; absent = names with
    no candidate at all."""
    found, unreachable, absent = [], [], []

    def want(name, targets):
        targets = list(targets)
        if not targets:
            absent.append(name)
            return
        for T in targets:
            d = root(T)
            if d is not None:
                found.append((name, d, float(Fraction(float(T)) / Fraction(2) ** (be - 150))))
                return
        unreachable.append(name)

    for sh in range(-17, 27):
        bd = be - sh
        if not 1 <= bd <= 254:
            continue
        for name, mds in class_mantissas(sh).items():
            want("sh %+d %s" % (sh, name), (make(bd, md) for md in mds))
    # subnormal squares md * 2^-149, md < 2^23 (bd_raw == 0): the smallest, one in the middle, the largest
    want("subnormal smallest", [from_bits(1)])
    want("subnormal middle", (from_bits(x) for x in range(1 << 22, (1 << 22) + 64)))
    want("subnormal largest", (from_bits(x) for x in range(ONE - 1, ONE - 65, -1)))
    return found, unreachable, absent


@functools.lru_cache(maxsize=2)
def term_grid(be, parity):
    """One case per rotation r of the class lists, all from the carry 2^(be-127) * (1 + parity * 2^-23).  Blocks 0 to 2 share the classes
    the chain can take without leaving its binade -- the fast path applies all three at entry exponent be --, block 3 holds those that
    carry it out.  In rotation r class (i + r) % N of a block's N stands at element i and at element 4095 - i: every class is first and
    last of a block once, and with it in slot 0 .. 15 of the candidates kernel's thread 0 and thread 255; between them are +0 squares."""
    classes, _, _ = grid_classes(be)
    order = {c[0]: i for i, c in enumerate(classes)}
    fit, out, used = [[], [], []], [], [0, 0, 0]
    for c in sorted(classes, key=lambda c: c[2]):
        need = 2 * (int(c[2]) + 2)
        if sum(used) + need <= ONE - (1 << 20):
            k = used.index(min(used))
            fit[k].append(c)
            used[k] += need
        else:
            out.append(c)
    for f in fit:                              # (at be = 1, 2, 3 few classes fit: a block left empty takes the lightest one again)
        if not f:
            f.append(min(classes, key=lambda c: c[2]))
    lists = [sorted(f, key=lambda c: order[c[0]]) for f in fit + [out]]
    cases = []
    for r in range(max(len(x) for x in lists)):
        a, b = np.zeros(4 * RB, dtype=F32), np.zeros(4 * RB, dtype=F32)
        for k, cls in enumerate(lists):
            for i in range(len(cls)):
                d = cls[(i + r) % len(cls)][1]
                put(a, b, k * RB + i, d, (i + r) & 1)
                put(a, b, k * RB + RB - 1 - i, d, (i + r + 1) & 1)
        cases.append(Case("term_grid", "be %d parity %d rotation %d" % (be, parity, r), a, b, make(be, ONE | parity), be=be, parity=parity,
                          blocks=[[c[0] for c in x] for x in lists], rotation=r))
    return tuple(cases)


# ---- ahead / behind --------------------------------------------------------------------------------------------------------------
def nearest_root(md0, bd, step):
    """the first reachable square make(bd, md0 + j * step), j = 0 .. 63"""
    for j in range(64):
        d = root(make(bd, md0 + j * step))
        if d is not None:
            return d
    return None


def pool(E):
    """reachable squares of 1/2 (a tie), 1/4, 3/4, 5/4, 3/2, 5/2, 3, 9/2 and 15/2 units of the grid of E"""
    out = []
    for x in (Fraction(1, 2), Fraction(1, 4), Fraction(3, 4), Fraction(5, 4), Fraction(3, 2), Fraction(5, 2), Fraction(3), Fraction(9, 2), Fraction(15, 2),
              Fraction(1), Fraction(9, 4), Fraction(25, 2), Fraction(49, 2), Fraction(81, 2)):
        T = ulps(x, E)
        d = root(T) if T is not None else None
        if d is not None:
            out.append((x, d))
    return out


def drift(kind, E0, seed):
    """`ahead`: carry (2 - 2^-10) * 2^(E0-127) and two blocks of squares just above half a unit of the grid of E0 -- each rounds up to a
    whole unit, so the float32 sum reaches the next binade after 8192 of them while the exact prefix is 2^-11 short of it: the blocks
    behind are entered one exponent ABOVE the predicted one (candidate 2).  `behind`: carry (2 - 2^-12) * 2^(E0-127) and two blocks of
    squares just below half a unit -- each is absorbed, the exact prefix crosses after 4099 of them: the blocks behind are entered one
    exponent BELOW the predicted one (candidate 0).  Four sparse blocks follow, of ties and mixed remainders drawn from pool() at the
    exponent the chain has there."""
    rng = np.random.default_rng(seed)
    if kind == "ahead":
        carry, filler, E1 = make(E0, TOP - (1 << 13)), nearest_root(ONE + (1 << 13), E0 - 24, 1), E0 + 1
    else:
        carry, filler, E1 = make(E0, TOP - (1 << 11)), nearest_root(TOP - (1 << 14), E0 - 25, -1), E0
    if filler is None or E0 - 25 < 1:
        return None
    a, b = np.zeros(6 * RB, dtype=F32), np.zeros(6 * RB, dtype=F32)
    for i in range(2 * RB):
        put(a, b, i, filler, i & 1)
    if kind == "ahead":                          # ties and mixed remainders in the blocks the centre candidate carries as well
        for at, (x, d) in zip((5, 77, 1000, 4000), pool(E0)[:4]):
            put(a, b, at, d, 1)
    terms = pool(min(E1, 254))
    for k in range(2, 6):
        at = np.sort(rng.choice(RB, size=14, replace=False))
        at[0], at[-1] = 0, RB - 1
        for i in at:
            put(a, b, k * RB + i, terms[rng.integers(len(terms))][1], i & 1)
    return Case(kind if E0 < 254 else "hostile", "%sE0 %d seed %d" % ("" if E0 < 254 else kind + " into +inf, ", E0, seed), a, b, carry, E0=E0)


def drift_family(kind, top=False):
    """For each entry exponent the first seed whose sparse blocks are entered with an even and with an odd mantissa, each by a block
    that holds a tie (the CPU test asserts it).  E0 = 253 and 254 are the top: at 253 `behind` predicts 254, whose upper neighbour does
    not exist; at 254 (top: these two cases stand in the `hostile` family) `ahead` overflows to +inf and `behind`'s prefix rounds to +inf,
    and the fallback takes the blocks."""
    want = 2 if kind == "ahead" else 0
    out = []
    for E0 in ((254,) if top else (27, 127, 253)):
        best = None
        for seed in range(40):
            c = drift(kind, E0, seed)
            if c is None:
                break
            best = best or c
            if E0 == 254 or {(ci, p) for _, ci, p, t in c.truth["applied"] if t and ci == want} == {(want, 0), (want, 1)}:
                best = c
                break
        if best is not None:
            out.append(best)
    return out


# ---- edges -----------------------------------------------------------------------------------------------------------------------
def sparse(n_blocks, seed, tail=RB, start=-56, per_block=12, carry=0.0, family="edges", name=None):
    """Blocks of `per_block` non-zero squares (j * 2^e)^2, j < 64, the first and the last element of every block among them; e rises by
    one every `step` blocks, so the chain crosses two binades per `step` blocks, ties come with every odd j in every other binade, and no
    two blocks of a scale share their sum."""
    rng = np.random.default_rng(seed)
    m = (n_blocks - 1) * RB + tail
    step = max(16, -(-n_blocks // 100))
    a, b = np.zeros(m, dtype=F32), np.zeros(m, dtype=F32)
    seen = set()
    for k in range(n_blocks):
        n_el = min(RB, m - k * RB)
        cnt = min(n_el, per_block)
        while True:
            j = rng.integers(1, 64, size=cnt)
            key = (k // step, int((j * j).sum()))
            if key not in seen:
                seen.add(key)
                break
        at = np.sort(rng.choice(n_el, size=cnt, replace=False))
        at[0], at[-1] = 0, n_el - 1
        for i, jj in zip(at, j):
            put(a, b, k * RB + int(i), F32(jj) * F32(2.0 ** (start + k // step)), i & 1)
    return Case(family, name or "%d blocks, tail %d" % (n_blocks, tail), a, b, carry, n_blocks=n_blocks)


def landing(L, where):
    """The entry mantissa plus the block's increment is 2^24 + L (L = -1, 0, 1) on the grid of exponent 128, whose unit 2^-22 is the
    square of 2^-11 (4 units: of 2^-10); the element that takes the mantissa to 2^24 is the first, a middle or the last of block 1."""
    one, four = F32(2.0 ** -11), F32(2.0 ** -10)
    a, b = np.zeros(4 * RB, dtype=F32), np.zeros(4 * RB, dtype=F32)
    cross = {"first": 0, "middle": 2048, "last": RB - 1}[where]
    before = [] if where == "first" else [3, 64, 65, 255, 256, 1000, 1001, 1500, 2000, 2047]
    terms = [(i, one, 1) for i in before]
    if L == 1 and where == "last":
        terms.append((cross, four, 4))                         # from 2^24 - 3 to 2^24 + 1 in one step
    else:
        terms.append((cross, one, 1))
        if L == 1:
            terms.append((cross + 1, one, 1))
    lead = [(1, one, 1), (700, four, 4), (RB - 1, one, 1)]       # block 0 goes before, blocks 2 and 3 behind: halves of the new unit among them
    M0 = TOP + L - sum(t[2] for t in terms) - sum(t[2] for t in lead)
    for i, d, _ in lead:
        put(a, b, i, d, i & 1)
    for i, d, _ in terms:
        put(a, b, RB + i, d, i & 1)
    for k in (2, 3):
        for i, d in ((0, one), (17 * k, four), (2048, F32(3 * 2.0 ** -11)), (RB - 1, one)):
            put(a, b, k * RB + i, d, i & 1)
    return Case("edges", "landing 2^24%+d, %s" % (L, where), a, b, make(128, M0), landing=L, block=1)


def edges():
    out = [landing(L, where) for L in (-1, 0, 1) for where in ("first", "middle", "last")]
    z = sparse(3, 11, start=-12, carry=1.0, name="a block of zeros between two others")
    a, b = z.a.copy(), z.b.copy()
    a[RB:2 * RB] = b[RB:2 * RB] = 0
    out.append(Case("edges", z.name, a, b, z.carry))
    out += [sparse(2, 20 + t, tail=t, start=-12, carry=1.0, name="a trailing block of %d" % t) for t in (1, 63, 64, 65, 4095)]
    out += [sparse(nblocks(m), 30 + m, tail=m - (nblocks(m) - 1) * RB, start=-12, carry=0.5, per_block=8, name="m = %d" % m) for m in (1, 4095, 4096, 4097)]
    out += [sparse(n, 40 + n) for n in (63, 64, 65, 128, 129)]
    return out


def long_cases():
    """1025 and 2049 blocks: rmse_predict_kernel with 2 and with 3 blocks per thread.  Every block is non-zero, and the sum doubles every
    few blocks, so a prefix taken from the wrong place has the wrong exponent."""
    return [sparse(1025, 1025, start=-56), sparse(2049, 2049, start=-56)]


# ---- hostile ---------------------------------------------------------------------------------------------------------------------
def hostile():
    out = []
    base = sparse(5, 50, start=-12, carry=0.0)

    def poisoned(name, av, bv, at=RB + 100, carry=0.0):
        a, b = base.a.copy(), base.b.copy()
        a[at], b[at] = av, bv
        out.append(Case("hostile", name, a, b, carry))

    poisoned("a NaN input", NAN, 0.25)
    poisoned("inf - inf", INF, INF)
    poisoned("d * d overflows", 1e30, -1e30)
    poisoned("an infinite input", -INF, 1.0)
    poisoned("a NaN input in the last element", NAN, 0.0, at=5 * RB - 1)
    poisoned("an infinite input in the first element", INF, 0.0, at=0)
    a, b = base.a.copy(), base.b.copy()
    for at in (RB + 7, RB + 2000, RB + 2001, 2 * RB + 5):
        a[at], b[at] = 1.3e19, 0.0                             # 1.69e38 each: the third overflows the SUM, in mid-block
    out.append(Case("hostile", "the sum overflows in mid-chain", a, b, 0.0))
    for name, scale in (("subnormal to the end", 1e-21), ("leaves the subnormals in mid-block", 1e-20)):
        rng = np.random.default_rng(60)
        a, b = np.zeros(4 * RB + 65, dtype=F32), np.zeros(4 * RB + 65, dtype=F32)
        for k in range(5):
            n_el = min(RB, len(a) - k * RB)
            at = np.sort(rng.choice(n_el, size=12, replace=False))
            at[0], at[-1] = 0, n_el - 1
            a[k * RB + at] = (rng.integers(1, 8, size=12) * scale).astype(F32)
        out.append(Case("hostile", name, a, b, 0.0))
    return out + drift_family("ahead", top=True) + drift_family("behind", top=True)


# ---- carries ---------------------------------------------------------------------------------------------------------------------
CARRIES = (("+0", 0.0), ("the smallest subnormal", from_bits(1)), ("the largest subnormal", from_bits(ONE - 1)), ("FLT_MIN", from_bits(ONE)),
           ("mantissa 2^24 - 1", make(127, TOP - 1)), ("FLT_MAX", from_bits(0x7F7FFFFF)), ("+inf", INF), ("NaN", NAN))


def carries():
    small = sparse(3, 70, tail=65, start=-12)
    rng = np.random.default_rng(71)
    a, b = np.zeros(2 * RB + 63, dtype=F32), np.zeros(2 * RB + 63, dtype=F32)
    for k in range(3):
        at = np.sort(rng.choice(63, size=10, replace=False))
        for i in at:
            put(a, b, k * RB + int(i), F32(rng.integers(1, 64)) * F32(2.0 ** (-70 + 35 * k)), i & 1)
    return [Case("carries", "%s into the %s vector" % (cname, vname), va, vb, c)
            for vname, va, vb in (("small", small.a, small.b), ("wide", a, b)) for cname, c in CARRIES]


# ---- the families ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases(family):
    if family in ("ahead", "behind"):
        return tuple(drift_family(family))
    return tuple({"edges": edges, "long": long_cases, "hostile": hostile, "carries": carries}[family]())


FAMILIES = ("ahead", "behind", "edges", "long", "hostile", "carries")       # and term_grid(be, parity), built and dropped pair by pair
JOB_COUNTS = (1, 2, 3, 64, 65)


# what no input reaches at all (the classes no float32 product reaches are grid_classes(be)[1])
UNREACHABLE_AT_ALL = (
    "ahead and behind at entry exponent 1: every float32 is a multiple of 2^-149, the unit of the grid of exponent 1, so while the sum is "
    "below 2^-125 every addition is exact and the float32 chain IS the exact prefix; neither runs ahead of the other",
    "ahead and behind below entry exponent 26: their squares of half a unit less or more 2^-10 need eleven bits below half the unit",
)


@functools.lru_cache(maxsize=None)
def job_pool():
    """Cases of at most six blocks for the batches: rotation 0 of every term_grid, the cases of the other families, and sixteen more sparse
    chains, each padded with a = b = 0 to the length of the longest: 6 blocks.  No two jobs share their carry: a case whose carry an
    earlier one has already gets a carry of its own where it is built from +0, 0.5 or 1 (it is a new case then, with a truth of its
    own) and is left out otherwise (the second vector of NaN and +inf).  No two share what the kernels compute from them either (the CPU
    test asserts both)."""
    picked = [term_grid(be, parity)[0] for be in GRID_BE for parity in (0, 1)]
    for family in ("ahead", "behind", "edges", "hostile", "carries"):
        picked += [c for c in cases(family) if c.m <= 6 * RB]
    picked += [sparse(6, 200 + i, tail=1 + 255 * i, start=-12 - 3 * i, carry=0.0, name="sparse %d for the batches" % i) for i in range(16)]
    m = max(c.m for c in picked)
    out, carries_seen, seen, fresh = [], set(), set(), 0
    for c in picked:
        carry = c.carry
        if bits(carry) in carries_seen:
            if bits(carry) not in (0, bits(F32(0.5)), bits(F32(1.0))):
                continue
            fresh += 1
            carry = make(96 + 2 * fresh, ONE + 0x12345 * fresh)
        a, b = np.zeros(m, dtype=F32), np.zeros(m, dtype=F32)
        a[:c.m], b[:c.m] = c.a, c.b
        job = Case("jobs", "%r" % c, a, b, carry)
        key = (job.truth["expo"].tobytes(), job.truth["cand"].tobytes(), tuple(job.truth["sums"]))
        if key in seen:
            continue
        carries_seen.add(bits(carry))
        seen.add(key)
        out.append(job)
    return tuple(out)


def jobs(n):
    """A batch of n jobs: n cases of job_pool(), taken with a stride so that every family is in every batch of more than a few."""
    pool_ = job_pool()
    step = next(s for s in (7, 11, 13, 17) if math.gcd(s, len(pool_)) == 1)
    assert n <= len(pool_)
    return [pool_[(n + i * step) % len(pool_)] for i in range(n)]


def golden_cases():
    """The vectors the golden file records the reference's rmse1d of (from a zero carry, which is all rmse1d has): every case of every
    family, of term_grid rotation 0 of every entry exponent and parity."""
    return [c for family in FAMILIES for c in cases(family)] + [term_grid(be, parity)[0] for be in GRID_BE for parity in (0, 1)]


def digest(case):
    return hashlib.sha256(case.a.tobytes() + case.b.tobytes()).hexdigest()[:16]


def chain_diff(final, m):
    """emMAF_cy.pyx:32-33: res / (float)m in float32, then sqrt in double"""
    with np.errstate(all="ignore"):
        return math.sqrt(float(F32(final) / F32(m)))                 # (the sum of squares is never negative)


def describe(case, k=None):
    t = case.truth
    s = "%r: m %d, carry %r (0x%08x)" % (case, case.m, case.carry, bits(case.carry))
    if k is not None:
        s += "; block %d: entry %r (0x%08x, exponent %d), predicted %d, %s" % (
            k, t["entries"][k], bits(t["entries"][k]), exponent(t["entries"][k]), t["expo"][k], "necessary serial" if k in t["serial"] else "fast path")
    return s
