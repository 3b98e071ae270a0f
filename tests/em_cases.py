"""Enumerated inputs for the EM update (csrc/em_kernels.hip: em_sweep_kernel, em_sweep_group_kernel, em_coded_kernel with one and
with two iterations per sweep, em_coded_group_kernel), built for the places the generated matrices, the AMRE files and edge.npz never
reach: terms whose float32 sum s = (p0 + p1) + p2 is subnormal, a signed zero, negative, infinite or NaN, numerators p1 + 2 p2 that are
negative, many binades above the sum, subnormal or infinite, frequencies outside (0, 1) -- and each of them at a chosen column of a
population slab: in the first buffer of a sweep, in a later one (where the fixup-free loop has to restore its running sum before it
redoes the buffer), in the checked buffer that holds the odd tail or a left-out individual.  NumPy only; the twin of
tests/fisher_cases.py, whose pair and frequency lists it extends.

THE RULING CONSTRAINT.  A SNP's update is a serial float32 sum over its population, so one non-finite term poisons its site.  Every
(site, population) therefore carries exactly ONE enumerated cell (pair, f_old), at one slab column (`hot_col`); all other columns
carry the ordinary pairs of ORDINARY.  Every builder is deterministic and returns its inputs next to the claims they are built for;
tests/test_em_cases_cpu.py holds them to those claims on the oracle, tests/test_gpu_em_cases.py runs them through the library."""
import numpy as np

import fisher_cases as fc
import synth
from fisher_cases import F32, first_difference, ids_for, interleave, same_nan  # noqa: F401  (what the tests share)

# ---- the terms -----------------------------------------------------------------------------------------------------------------------
# fisher_cases.PAIRS, and:
#   (-0.0, 1.0000001)   the only way to a sum of -0.0: p0 = g0 (1-f)^2 is -0.0 only for g0 = -0.0 (atof("-0") in a Beagle file), and
#                       p2 = g2 f^2 only for g2 < 0, i.e. g1 > 1; at f = -0.0 all of p0, p1, p2 and the numerator are -0.0: -0/-0;
#   (2^-50, 0.5)        at f = -2^-50: p0 + p1 == 0 exactly, s = p2 = 2^-101 and num = -2^-50 + 2^-100: a NEGATIVE numerator 2^51
#                       times its positive sum (cancellation in the sum, none in the numerator);
#   (2^-100, 0.5)       at f = -2^-100 the same with a p2 that underflows: s = +0 and a negative numerator, -inf.
PAIRS_ADDED = ((-0.0, 1.0000001), (2.0 ** -50, 0.5), (2.0 ** -100, 0.5))
PAIRS = fc.PAIRS + PAIRS_ADDED
# fisher_cases.FREQS (0, -0.0, 1, the smallest subnormal, 2.0, the clamp bounds of 84, 16 and 3 individuals among them), and:
#   -0.25               a negative frequency of ordinary size: p1 < 0, negative numerators over positive sums at ordinary pairs;
#   0.8                 (0.6, 0.6) has num = -0.064 over s = 0.088 here: a negative numerator INSIDE (0, 1), so in `finite` too;
#   -2^-50, -2^-100     see the pairs above;
#   -1e-45              the negative smallest subnormal: p1 rounds to -1e-45 or to -0.0, sums of -0.0 + 0.5 q.
FREQS_ADDED = (-0.25, 0.8, -(2.0 ** -50), -(2.0 ** -100), -1e-45)
FREQS = fc.FREQS + FREQS_ADDED
# Frequencies at which EVERY pair with g0 > 0 and g1 > 0 has p0 = +inf and p1 = -inf or a NaN of its own -- the whole site is NaN in
# any population of two or more -- stand only at the anchor sites (below), so that the hostile variant stays under its cap:
#   1e20                (1 - f)^2 overflows float32: (1, 0) has s = +inf (and a quotient of 0), (0, 1) has s = num = -inf;
#   NaN                 everything is NaN.
EXTRA_CELLS = (((1, 0), 1e20), ((0, 1), 1e20), ((0.25, 0.5), float("nan")))
# The other columns: a few distinct pairs with full mantissas, ANGSD's pair that sums above 1 among them.
ORDINARY = ((0.666667, 0.333334), (0.333333, 0.333333), (0.123456, 0.654321), (0.57735, 0.31831), (0.9, 0.05))
VARIANTS = ("finite", "hostile")

S_CLASSES = ("s positive normal", "s positive subnormal", "s = +0", "s = -0", "s negative finite", "s = +inf", "s = -inf", "s = NaN")
NUM_CLASSES = ("num negative, s positive finite", "|num| > 2^24 s, s positive finite", "num = 0, s positive", "num subnormal", "num infinite",
               "half the quotient overflows float32")
CLASSES = S_CLASSES + NUM_CLASSES
# what the finite variant holds too (its frequencies lie strictly inside (0, 1); a sum of zero, an infinite or a NaN one gives a result the
# reference does not keep finite)
FINITE_CLASSES = ("s positive normal", "s positive subnormal", "s negative finite", "num negative, s positive finite", "num = 0, s positive",
                  "num subnormal")


def terms(g0, g1, f):
    """The term of emMAF_cy.pyx:19-22 for float32 g0, g1, f (broadcast), with its rounding sequence: p0, p1, p2 and s = (p0 + p1) + p2
    float32, num = p1 + 2 p2 and q = num / s float64 (the addend is q / 2: the scalings by 2 are exact)."""
    with np.errstate(all="ignore"):
        g0d, g1d, fd = (np.asarray(x, dtype=F32).astype(np.float64) for x in (g0, g1, f))
        omf = 1.0 - fd
        p0 = ((g0d * omf) * omf).astype(F32)
        p1 = (((g1d * 2.0) * fd) * omf).astype(F32)
        p2 = ((((1.0 - g0d) - g1d) * fd) * fd).astype(F32)
        s = ((p0 + p1).astype(F32) + p2).astype(F32)
        num = p1.astype(np.float64) + 2.0 * p2.astype(np.float64)
        q = num / s.astype(np.float64)
    return dict(p0=p0, p1=p1, p2=p2, s=s, num=num, q=q)


def classify(t):
    """CLASSES -> boolean mask over the terms `t` of terms().  The last class, |q / 2| beyond float32's largest finite value, is met
    by x/0 alone for likelihood pairs: a finite quotient stays below 2^76 (if (p0 + p1) + p2 cancels below 2^-24 of its largest
    operand, p0 + p1 was exactly 0 and q = 2 + p1 / p2 with p2 no smaller than 2^-149)."""
    s, num, q = t["s"], t["num"], t["q"]
    tiny = np.finfo(F32).tiny
    with np.errstate(all="ignore"):
        pos = np.isfinite(s) & (s > 0)
        num32 = num.astype(F32)
        return {"s positive normal": pos & (s >= tiny), "s positive subnormal": pos & (s < tiny), "s = +0": (s == 0) & ~np.signbit(s),
                "s = -0": (s == 0) & np.signbit(s), "s negative finite": np.isfinite(s) & (s < 0), "s = +inf": np.isposinf(s),
                "s = -inf": np.isneginf(s), "s = NaN": np.isnan(s),
                "num negative, s positive finite": pos & (num < 0), "|num| > 2^24 s, s positive finite": pos & (np.abs(num) > 2.0 ** 24 * s),
                "num = 0, s positive": pos & (num == 0), "num subnormal": (num32 != 0) & (np.abs(num32) < tiny), "num infinite": np.isinf(num),
                "half the quotient overflows float32": np.abs(0.5 * q) > float(np.finfo(F32).max)}


def redo(t):
    """The terms whose sum is not a positive finite float32: what sends a buffer of the fixup-free loops round again."""
    with np.errstate(all="ignore"):
        return ~(np.isfinite(t["s"]) & (t["s"] > 0))


def variant_lists(variant):
    """(pairs (np, 2) float32, freqs (nf,) float32) of a variant's grid.  hostile: everything.  finite: fisher_cases' finite lists (the
    pairs the reference keeps finite at every frequency strictly inside (0, 1), and those frequencies) with the additions that fit."""
    assert variant in VARIANTS
    if variant == "hostile":
        pairs, freqs = PAIRS, FREQS
    else:
        pairs = tuple(p for p in fc.PAIRS if p not in fc.NOT_FINITE_INSIDE) + PAIRS_ADDED[1:]
        freqs = tuple(f for f in FREQS if 0.0 < float(F32(f)) < 1.0)
    return np.array(pairs, dtype=np.float64).astype(F32), np.array(freqs, dtype=np.float64).astype(F32)


# ---- the places ------------------------------------------------------------------------------------------------------------------------
# fisher_cases.SIZES and 24, 25, 32, 40, 49.  The direct kernels take a buffer of 8 individuals, the coded ones one of 16; a buffer
# that is full and holds no left-out individual is `plain` (fixup-free in em_sweep_kernel, unconditional in coded_phase2), the one
# with the odd tail is `checked`.  1 and 2: no plain buffer at all; 7, 8, 9 and 15, 16, 17: one buffer and one buffer +- 1; 24, 25,
# 32, 33, 40, 49: two to six plain buffers of 8 and one to three of 16, with and without a tail; 2, 4, 8, 14, 16, 24, 32, 40: even.
SIZES = fc.SIZES + (24, 25, 32, 40, 49)
BUFFERS = (8, 16)
PLACES = ("first plain buffer, first column", "first plain buffer, last column", "first plain buffer", "later plain buffer", "checked buffer")
M_GRID = 7 * 64 + 13              # seven tiles and a partial one
STRIDE = 97                       # population k starts STRIDE cells after population k - 1: every cell stands in four or more populations
DENSE = 4                         # one site in four takes a cell whose sum is not a positive finite number


def place_of(size, col, buffer):
    """The place (one of PLACES) of slab column `col` in a population of `size`, for a kernel that walks buffers of `buffer`."""
    assert 0 <= col < size
    b = col // buffer
    if buffer * (b + 1) > size:
        return "checked buffer"
    if b > 0:
        return "later plain buffer"
    return {0: "first plain buffer, first column", buffer - 1: "first plain buffer, last column"}.get(col, "first plain buffer")


def marked_columns(size):
    """The first and the last column of every buffer of 8 (hence of 16), the last column of the population and the one before, and
    columns 3 and 5: what the sites s % DENSE == 1 walk through.  The left-out columns of loo_columns are among them."""
    return sorted({c for c in [3, 5, size - 2, size - 1] + list(range(0, size, 8)) + list(range(7, size, 8)) if 0 <= c < size})


def anchors(m):
    """The sites at which population k takes the representative of s-class (k + j) % 8 (j: the anchor's number): the first site, lane
    63 of the first tile, lane 0 of the second, and the last site."""
    return (0, 63, 64, m - 1)


def em_grid(variant, sizes=SIZES, m=M_GRID):
    """One enumerated cell per (site, population).  With the grid's cells numbered c = pair * nf + frequency,
        population k, site s      cell (s + STRIDE * k) % ncells, at slab column hot_col = (s + 3 * (s // 64)) % size_k
        the other columns c       ORDINARY[(c + k + s) % 5]
        individual                the populations interleave in file order (fisher_cases.interleave)
    except
        at the sites s % DENSE == 1, which take the grid's cells in need of the fixup in turn -- one with a finite quotient, one with an
        infinite one -- at the marked_columns of the population in turn, and
        at the anchors(m), where population k takes the representative of an s-class: the first cell of that class among the grid's
        and (hostile) EXTRA_CELLS.
    Every population walks through every one of its columns; a cell meets a different site, lane and column in each population it
    stands in.
    Returns dict(variant, L (m, 2n), f_old (K, m), IDs, labels, sizes, col_of (n,), members (K lists of individuals), cell (m, K) into
    pairs_tab (cells, 2) / f_tab (cells,), n_grid, hot_col (m, K), reps (class name -> cell), anchors)."""
    pairs, freqs = variant_lists(variant)
    n_pairs, nf = len(pairs), len(freqs)
    n_grid = n_pairs * nf
    pairs_tab = np.repeat(pairs, nf, axis=0)
    f_tab = np.tile(freqs, n_pairs)
    if variant == "hostile":
        pairs_tab = np.concatenate((pairs_tab, np.array([p for p, _ in EXTRA_CELLS], dtype=np.float64).astype(F32)))
        f_tab = np.concatenate((f_tab, np.array([f for _, f in EXTRA_CELLS], dtype=np.float64).astype(F32)))
    cls = classify(terms(pairs_tab[:, 0], pairs_tab[:, 1], f_tab))
    reps = {name: int(np.flatnonzero(cls[name])[0]) for name in S_CLASSES if cls[name].any()}
    rep_list = [reps[name] for name in S_CLASSES if name in reps]
    K = len(sizes)
    labels = interleave(sizes)
    n = len(labels)
    col_of = np.array([int((labels[:i] == labels[i]).sum()) for i in range(n)])
    s, k = np.arange(m)[:, None], np.arange(K)[None, :]
    cell = (s + STRIDE * k) % n_grid
    # the cells that need the fixup are few (one in twelve of `hostile`, one in thirty of `finite`): every DENSE-th site takes one of them
    # -- in turn one whose quotient is finite (a negative sum) and, in `hostile`, one whose quotient is infinite (x/0), so that every marked
    # column of every population, the left-out ones among them, meets sites that a single term poisons.  (The NaN terms keep to their
    # turn in the walk: the cap.)
    t_grid = terms(pairs_tab[:n_grid, 0], pairs_tab[:n_grid, 1], f_tab[:n_grid])
    needy = [np.flatnonzero(redo(t_grid) & np.isfinite(t_grid["q"])), np.flatnonzero(np.isinf(t_grid["q"]))]
    if len(needy[1]) == 0:
        needy[1] = needy[0]
    dense = np.arange(m) % DENSE == 1
    turn = s[dense] // DENSE
    cell[dense] = np.where(turn % 2 == 0, needy[0][(turn // 2 + turn // 14 + 5 * k) % len(needy[0])], needy[1][(turn // 2 + turn // 14 + k) % len(needy[1])])
    for j, a in enumerate(anchors(m)):
        cell[a] = [rep_list[(kk + j) % len(rep_list)] for kk in range(K)]
    hot_col = (s + 3 * (s // 64)) % np.array(sizes)[None, :]
    for kk, size in enumerate(sizes):                    # ... and stand at the columns that matter, in turn
        marked = marked_columns(size)
        hot_col[dense, kk] = [marked[(x // 2 + kk) % len(marked)] for x in np.arange(m)[dense] // DENSE]        # (a finite and an infinite one each)
    ordinary = np.array(ORDINARY, dtype=np.float64).astype(F32)
    which = (col_of[None, :] + labels[None, :] + s) % len(ordinary)                # (m, n)
    hot = hot_col[:, labels] == col_of[None, :]
    L = np.empty((m, 2 * n), dtype=F32)
    for h in (0, 1):
        L[:, h::2] = np.where(hot, pairs_tab[cell[:, labels], h], ordinary[which, h])
    f_old = np.ascontiguousarray(f_tab[cell].T)
    assert m > 3 * 64 and m % 64 and hot.sum() == m * K and STRIDE * 4 < m
    members = [np.flatnonzero(labels == kk) for kk in range(K)]
    return dict(variant=variant, L=L, f_old=f_old, IDs=ids_for(labels), labels=labels, sizes=tuple(sizes), col_of=col_of, members=members,
                cell=cell, pairs_tab=pairs_tab, f_tab=f_tab, n_grid=n_grid, hot_col=hot_col, reps=reps, anchors=anchors(m))


def cell_terms(grid):
    """terms() of the enumerated cell of every (site, population): arrays (m, K)."""
    c = grid["cell"]
    return terms(grid["pairs_tab"][c, 0], grid["pairs_tab"][c, 1], grid["f_tab"][c])


def cell_places(grid, cell):
    """Where a cell stands: [(population, its size, site, slab column, its place for buffers of 8, for buffers of 16)]."""
    out = []
    for s, k in np.argwhere(grid["cell"] == cell):
        size, col = grid["sizes"][k], int(grid["hot_col"][s, k])
        out.append((int(k), size, int(s), col, place_of(size, col, 8), place_of(size, col, 16)))
    return out


def describe(grid, k, site, skip_col=None):
    """The cell and place of (population k, site), for a failure message."""
    c = int(grid["cell"][site, k])
    size, col = grid["sizes"][k], int(grid["hot_col"][site, k])
    t = terms(grid["pairs_tab"][c, 0], grid["pairs_tab"][c, 1], grid["f_tab"][c])
    names = [name for name, mask in classify(t).items() if mask]
    return "population %d of %d, site %d (lane %d): cell %d = pair %r at f_old %r [%s] at column %d (%s / %s)%s" % (
        k, size, site, site % 64, c, tuple(float(x) for x in grid["pairs_tab"][c]), float(grid["f_tab"][c]), "; ".join(names), col,
        place_of(size, col, 8), place_of(size, col, 16), "" if skip_col is None else ", column %d left out" % skip_col)


# ---- a running sum of -0.0 ---------------------------------------------------------------------------------------------------------------
# The float32 sum starts at +0.0 and +0.0 + x is never -0.0 for x = -0.0 -- it takes a term that UNDERFLOWS: at f_old = -1e-45 (the
# negative smallest subnormal) the pair (1, 0.5) has p1 = -1e-45, s = 1 and half its quotient is -2^-150, the midpoint between -0.0 and
# -1e-45, which rounds to even: the sum becomes -0.0.  From then on the sign of every zero quotient counts: (0.9, 0.2) has p1 and p2
# that underflow to -0.0 (0.4 of the smallest subnormal, and -0.1 f^2), a numerator of -0.0 over s = 0.9, a quotient of -0.0, and
# -0.0 + -0.0 keeps the sign that -0.0 + +0.0 loses.  The reference returns -0.0 at every site.
ZERO_LEAD, ZERO_REST, ZERO_F = (1.0, 0.5), (0.9, 0.2), -1e-45
ZERO_SIZES = (1, 2, 8, 9, 16, 17, 24, 33)
M_ZEROS = 3 * 64 + 8


def negative_zero_sums(m=M_ZEROS, sizes=ZERO_SIZES):
    """dict(L, f_old (K, m), IDs, labels, sizes, members, lead_col (m, K)): populations of (0.9, 0.2) with one (1, 0.5) at slab column
    lead_col = (s + s // 64) % size (every column of every population: the first, so that a whole plain buffer follows the sum's turn
    to -0.0, the last of a buffer, the tail), all at f_old = -1e-45, interleaved in file order."""
    K = len(sizes)
    labels = interleave(sizes)
    n = len(labels)
    col_of = np.array([int((labels[:i] == labels[i]).sum()) for i in range(n)])
    s = np.arange(m)[:, None]
    lead_col = (s + s // 64) % np.array(sizes)[None, :]
    lead = lead_col[:, labels] == col_of[None, :]
    pair = np.array([ZERO_REST, ZERO_LEAD], dtype=np.float64).astype(F32)
    L = np.empty((m, 2 * n), dtype=F32)
    for h in (0, 1):
        L[:, h::2] = pair[lead.astype(int), h]
    f_old = np.full((K, m), ZERO_F, dtype=F32)
    assert m > 3 * 64 and m % 64
    return dict(L=L, f_old=f_old, IDs=ids_for(labels), labels=labels, sizes=tuple(sizes), col_of=col_of, lead_col=lead_col,
                members=[np.flatnonzero(labels == kk) for kk in range(K)])


def reference_zeros(orc):
    """(case, f (1, K, m)): the oracle's first update of negative_zero_sums().  Computed once, shared, read-only."""
    if "zeros" not in _reference:
        g = negative_zero_sums()
        f = np.stack([updates(orc.emMAF_update, columns(g["L"], g["members"][k]), g["f_old"][k], 1) for k in range(len(g["sizes"]))], axis=1)
        f.setflags(write=False)
        _reference["zeros"] = (g, f)
    return _reference["zeros"]


# ---- leave-one-out -----------------------------------------------------------------------------------------------------------------------
LOO_SIZES = (9, 17, 33, 49)       # one buffer of 8 and a tail; one of 16 and a tail; two and three of 16 and a tail
LOO_BATCHES = (1, 3, 4, 5)        # a lone fit, a short group, a full group, two groups (four fits share a tile in the float32 kernel)


def loo_columns(size):
    """The left-out slab columns of the (up to five) re-fits of a population: the first and the last column, one inside the first
    buffer, the first of the second buffer of 8 (or a second one inside the first), and the first of the second buffer of 16 (or the last but one).  As hot_col walks
    through every column, each fit meets sites whose enumerated cell is the column it leaves out (finite for it, poisoned for its
    group mates), a column of the same buffer, and a column of another buffer."""
    cols = [0, size - 1, 3, 8 if size > 9 else 7, 16 if size > 17 else size - 2 if size > 9 else 5]
    assert len(set(cols)) == 5 and all(0 <= c < size for c in cols)
    return cols


def loo_fits(grid, k, count):
    """(groups (count,), skips (count,) global individuals, their slab columns) of the first `count` re-fits of population k."""
    cols = loo_columns(grid["sizes"][k])[:count]
    return np.full(count, k, dtype=np.int32), grid["members"][k][cols].astype(np.int32), cols


# ---- what the reference makes of them -----------------------------------------------------------------------------------------------
UPDATES = 3
GOLDEN_SIZES = (1, 2, 8, 9, 17, 33)          # the populations tests/golden/em_cases.npz records (all of SIZES would be 500 KB)
GOLDEN_LOO = 17                              # ... and the population whose five re-fits it records
GOLDEN = {"finite": dict(variant="finite", sizes=GOLDEN_SIZES, m=M_GRID), "hostile": dict(variant="hostile", sizes=GOLDEN_SIZES, m=M_GRID)}
_grids, _reference = {}, {}


def grid_of(variant, sizes=SIZES):
    key = (variant, tuple(sizes))
    if key not in _grids:
        g = em_grid(variant, sizes)
        for a in (g["L"], g["f_old"], g["cell"], g["hot_col"]):
            a.setflags(write=False)
        _grids[key] = g
    return _grids[key]


def updates(update, L_pop, f_old, count=UPDATES):
    """(count, m) float32: f after 1 .. count updates by `update(L, f, t)` (in place, as emMAF_cy.emMAF_update), from f_old."""
    out = np.empty((count, len(f_old)), dtype=F32)
    f = np.array(f_old, dtype=F32)
    for u in range(count):
        update(L_pop, f, 1)
        out[u] = f
    return out


def columns(L, idx):
    """The file-order column gather of WGSassign.py:227-233."""
    idx = np.asarray(idx)
    out = np.empty((L.shape[0], 2 * len(idx)), dtype=F32)
    out[:, 0::2], out[:, 1::2] = L[:, 2 * idx], L[:, 2 * idx + 1]
    return out


def reference(orc, variant, sizes=SIZES):
    """(grid, f (UPDATES, K, m)): the oracle's frequencies after 1, 2 and 3 updates of every population from the enumerated f_old.
    Computed once, shared, read-only."""
    key = (variant, tuple(sizes))
    if key not in _reference:
        g = grid_of(variant, sizes)
        f = np.stack([updates(orc.emMAF_update, columns(g["L"], g["members"][k]), g["f_old"][k]) for k in range(len(sizes))], axis=1)
        f.setflags(write=False)
        _reference[key] = (g, f)
    return _reference[key]


def reference_loo(orc, variant, k, sizes=SIZES):
    """(grid, cols, f (UPDATES, 5, m)): the same for the five re-fits of population k, each without one of loo_columns."""
    key = (variant, tuple(sizes), "loo", k)
    if key not in _reference:
        g = grid_of(variant, sizes)
        _, skips, cols = loo_fits(g, k, 5)
        f = np.stack([updates(orc.emMAF_update, columns(g["L"], g["members"][k][g["members"][k] != i]), g["f_old"][k]) for i in skips], axis=1)
        f.setflags(write=False)
        _reference[key] = (g, cols, f)
    return _reference[key]


def predicted(grid, k, skip_col=None):
    """(nan (m,), inf (m,)) bool: what the s / num classification says of population k's first update (without column skip_col): NaN
    where a term is NaN (a sum or numerator that is NaN, 0/0, inf/inf) or quotients of +inf and -inf meet, infinite where quotients
    of one sign of infinity stand among finite ones.  (Finite quotients stay below 2^76: the float32 sum itself never overflows.)"""
    mem = grid["members"][k]
    if skip_col is not None:
        mem = np.delete(mem, skip_col)
    q = terms(grid["L"][:, 2 * mem], grid["L"][:, 2 * mem + 1], grid["f_old"][k][:, None])["q"]
    pinf, ninf = np.isposinf(q).any(axis=1), np.isneginf(q).any(axis=1)
    nan = np.isnan(q).any(axis=1) | (pinf & ninf)
    if len(mem) == 0:
        nan = np.ones(len(q), dtype=bool)            # 0 / (float)0
    return nan, (pinf | ninf) & ~nan


def digest(grid):
    return synth.digest(np.concatenate((grid["L"].ravel().view(np.uint32), grid["f_old"].ravel().view(np.uint32))))


def squares(f_new, f_old):
    """The per-site float32 squares (f_new - f_old)^2 of emMAF_cy.pyx:31."""
    with np.errstate(all="ignore"):
        d = (np.asarray(f_new, dtype=F32) - np.asarray(f_old, dtype=F32)).astype(F32)
        return (d * d).astype(F32)
