"""Holds the enumerated convergence chains of tests/rmse_cases.py to what they claim, without a GPU: the classes are where the builders
say, the increments by definition are what the literal float32 chain does, no predicted exponent hangs on the order of a float64 sum,
every candidate cell is applied by a block that holds a tie, the strict accumulation is the oracle's and the real reference's
(tests/golden/rmse_cases.npz), and the guard band of device.decide_converged never contradicts the serial sum on its worst cases."""
import math

import numpy as np
import pytest

import rmse_cases as rc

F32 = np.float32
PAIRS = [(be, parity) for be in rc.GRID_BE for parity in (0, 1)]


def small_cases():
    return [c for family in rc.FAMILIES if family != "long" for c in rc.cases(family)]


def test_class_coverage():
    """Every class grid_classes() found stands, over the rotations, at the first and the last element of a block and in the sixteen
    elements of the candidates kernel's thread 0 and thread 255; every class that is missing is named, with why."""
    for be in rc.GRID_BE:
        found, unreachable, absent = rc.grid_classes(be)
        names = [c[0] for c in found]
        assert len(set(names)) == len(names)
        shifts = [sh for sh in range(-17, 27) if 1 <= be - sh <= 254]
        expected = sum(len(rc.class_mantissas(sh)) for sh in shifts) + 3
        assert len(found) + len(unreachable) + len(absent) == expected
        print("be %3d: shifts %+d .. %+d, %d classes built, %d unreachable, %d do not exist" % (be, shifts[0], shifts[-1], len(found), len(unreachable), len(absent)))
        print("    unreachable (no float32 d has fl(d * d) in the class; root() searched every candidate's neighbours):", ", ".join(unreachable) or "none")
        print("    do not exist:", ", ".join(absent) or "none")
        for name in ("subnormal smallest", "subnormal middle", "subnormal largest"):
            assert name in names                                    # the subnormal squares are all reachable
        # a tie is reachable at every shift from 2 to 22, whatever the exponent (those of shifts 1, 23 and 24 at every other exponent only)
        for sh in shifts:
            if 2 <= sh <= 22:
                assert "sh %+d tie" % sh in names, (be, sh)
        by_name = {c[0]: c[1] for c in found}
        for parity in (0, 1):
            cases = rc.term_grid(be, parity)
            first, last, lane0, lane255 = set(), set(), set(), set()
            for c in cases:
                d = np.subtract(c.a, c.b, dtype=F32)
                for k, block in enumerate(c.claims["blocks"]):
                    at = {name: np.flatnonzero(d[k * rc.RB:(k + 1) * rc.RB] == by_name[name]) for name in block}
                    for name, idx in at.items():
                        first |= {name} if 0 in idx else set()
                        last |= {name} if rc.RB - 1 in idx else set()
                        lane0 |= {name} if (idx < 16).any() else set()
                        lane255 |= {name} if (idx >= rc.RB - 16).any() else set()
            assert first == last == lane0 == lane255 == set(names), (be, parity)
            assert all(bool(c.carry == rc.make(be, rc.ONE | parity)) for c in cases)
    for line in rc.UNREACHABLE_AT_ALL:
        print("unreachable:", line)


def literal(sq_block, start):
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate((np.array([start], dtype=F32), sq_block)), dtype=F32)[-1]


def check_increments(case, counts):
    """increments() == increment_by_definition() for all six candidates of every predicted block, and both are what the literal
    float32 chain does to sampled entry mantissas of either parity: 2^23, 2^23 + 1, two in the middle, the largest that still fits."""
    t = case.truth
    nb = len(t["expo"])
    sq = np.concatenate((t["sq"], np.zeros(nb * rc.RB - case.m, dtype=F32))).reshape(nb, rc.RB)
    for k in np.flatnonzero(t["expo"] > 0):
        for ci in range(3):
            E = int(t["expo"][k]) - 1 + ci
            for p in (0, 1):
                D = int(t["cand"][k, 2 * ci + p])
                assert D == rc.increment_by_definition(sq[k], E, p), (case, k, ci, p)
                counts["by definition"] += 1
                if D >= rc.ONE or not 1 <= E <= 254:
                    continue
                largest = rc.TOP - 1 - D
                largest -= (largest ^ p) & 1
                for M in {rc.ONE + p, rc.ONE + 2 + p, rc.ONE + 0x2AAAAA * 2 + p, largest}:
                    if rc.ONE <= M and M + D < rc.TOP:
                        assert rc.bits(literal(sq[k], rc.make(E, M))) == rc.bits(rc.make(E, M + D)), (case, k, ci, p, M)
                        counts["literal"] += 1
                if largest >= rc.ONE and D > 0:                     # ... and one mantissa further the chain leaves the binade
                    assert rc.exponent(literal(sq[k], rc.make(E, min(largest + 2, rc.TOP - 1)))) != E or largest + 2 >= rc.TOP


def test_increments_agree_with_the_literal_chain():
    counts = {"by definition": 0, "literal": 0}
    for c in small_cases():
        if c.family != "carries":
            check_increments(c, counts)
    for be, parity in PAIRS:
        cases = rc.term_grid(be, parity)
        for c in (cases[0], cases[len(cases) // 2], cases[-1]):
            check_increments(c, counts)
    print("increments compared:", counts)
    assert counts["literal"] > 2000


def test_predicted_exponents_are_away_from_the_knife_edge():
    worst = {}
    for c in small_cases() + list(rc.cases("long")) + [c for pair in PAIRS for c in rc.term_grid(*pair)] + list(rc.job_pool()):
        worst[c.family] = min(worst.get(c.family, rc.INF), c.truth["margin"])
        assert c.truth["margin"] >= rc.MARGIN, (c, c.truth["margin"])
    print("smallest relative distance of an exact prefix from a limit, where the order of additions can matter:", {k: "%.3g" % v for k, v in worst.items()})


def test_every_cell_is_applied_and_the_serial_blocks_are_the_stated_ones():
    cells, per_family = {}, {}
    every = small_cases() + list(rc.cases("long")) + [c for pair in PAIRS for c in rc.term_grid(*pair)]
    for c in every:
        t = c.truth
        nonzero = int((t["expo"] != -1).sum())
        fam = per_family.setdefault(c.family, [0, 0, 0])
        fam[0], fam[1], fam[2] = fam[0] + 1, fam[1] + nonzero, fam[2] + len(t["serial"])
        for k, ci, p, ties in t["applied"]:
            if ties:
                cells[(ci, p)] = cells.get((ci, p), 0) + 1
        if c.family not in ("hostile", "carries"):
            assert 4 * len(t["serial"]) <= nonzero, (c, t["serial"], nonzero)
        if c.family == "term_grid":
            assert t["serial"] == [3] and [a[0] for a in t["applied"]] == [0, 1, 2] and {a[1] for a in t["applied"]} == {1}, (c, t["serial"], t["applied"])
        elif c.family == "ahead":
            assert t["serial"] == [1], (c, t["serial"])          # the block in which the float32 sum reaches the next binade
            assert {(ci, p) for k, ci, p, ties in t["applied"] if ties and k >= 2} == {(2, 0), (2, 1)}, c
        elif c.family == "behind":
            assert t["serial"] == [], (c, t["serial"])
            assert {(ci, p) for k, ci, p, ties in t["applied"] if ties and k >= 2} == {(0, 0), (0, 1)}, c
        elif "landing" in c.claims:
            # (at 2^24 - 1 the fast path applies block 1 -- no mantissa is larger -- and the first term of block 2 leaves the binade)
            assert t["serial"] == ([2] if c.claims["landing"] < 0 else [1]), (c, t["serial"])
            assert rc.mantissa(t["entries"][1]) + int(t["cand"][1, 2 + (rc.mantissa(t["entries"][1]) & 1)]) == rc.TOP + c.claims["landing"], c
    for fam, (n, blocks, serial) in per_family.items():
        print("%-9s %4d cases, %5d non-zero blocks, %4d of them necessary serial" % (fam, n, blocks, serial))
    print("blocks with a tie that the walk applies, per (candidate, parity):", sorted(cells.items()))
    assert set(cells) == {(ci, p) for ci in range(3) for p in (0, 1)}
    top = {c.name.split(" into")[0]: c for c in rc.cases("hostile") if "into +inf" in c.name}
    assert set(top) == {"ahead", "behind"}
    assert np.isinf(top["ahead"].truth["final"]) and top["ahead"].truth["serial"] == [1, 2, 3, 4, 5]
    assert (top["behind"].truth["expo"][2:] == 0).all() and top["behind"].truth["serial"] == [2, 3, 4, 5]     # the prefix rounds to +inf
    edges = {c.name: c for c in rc.cases("edges")}
    assert (edges["a block of zeros between two others"].truth["expo"] == -1).tolist() == [False, True, False]
    for c in rc.cases("long"):                                       # every block non-zero, no two sums alike
        assert (c.truth["expo"] != -1).all() and len(set(c.truth["sums"])) == len(c.truth["sums"])
        assert len(set(c.truth["expo"].tolist())) > 60               # ... and the chain climbs through many binades
    hostile = {c.name: c.truth for c in rc.cases("hostile")}
    assert np.isnan(hostile["a NaN input"]["final"]) and np.isnan(hostile["inf - inf"]["final"])
    assert np.isinf(hostile["d * d overflows"]["final"]) and np.isinf(hostile["an infinite input"]["final"])
    assert np.isinf(hostile["the sum overflows in mid-chain"]["final"]) and not hostile["the sum overflows in mid-chain"]["nonfinite"].any()
    assert rc.exponent(hostile["subnormal to the end"]["final"]) == 0 and hostile["subnormal to the end"]["final"] > 0
    t = hostile["leaves the subnormals in mid-block"]
    assert rc.exponent(t["entries"][0]) == 0 and rc.exponent(t["entries"][1]) >= 1
    assert [rc.bits(c.carry) for c in rc.cases("carries")[:8]] == [0, 1, 0x7FFFFF, 0x800000, 0x3FFFFFFF, 0x7F7FFFFF, 0x7F800000, rc.bits(F32(rc.NAN))]


def test_jobs_differ():
    pool = rc.job_pool()
    assert len(pool) >= max(rc.JOB_COUNTS) and len({c.m for c in pool}) == 1
    assert len({rc.bits(c.carry) for c in pool}) == len(pool)         # no two jobs share their carry,
    keys = {(c.truth["expo"].tobytes(), c.truth["cand"].tobytes(), tuple(c.truth["sums"])) for c in pool}
    assert len(keys) == len(pool)                                     # ... nor their block sums, exponents and candidates
    for n in rc.JOB_COUNTS:
        batch = rc.jobs(n)
        assert len(batch) == n and len({id(c) for c in batch}) == n
    print("job pool:", len(pool), "cases of", pool[0].m, "elements; families in the batch of 64:", sorted({c.name.split("/")[0] for c in rc.jobs(64)}))


def test_strict_accumulation_matches_the_oracle_and_the_reference(oracle, golden):
    g = golden("rmse_cases.npz")
    cases = rc.golden_cases()
    assert [repr(c) for c in cases] == list(g["names"]) and [rc.digest(c) for c in cases] == list(g["digests"])
    for c, want in zip(cases, g["rmse1d"]):
        final = rc.reference_chain(c.truth["sq"], F32(0))[1]
        got, orc = rc.chain_diff(final, c.m), oracle.rmse1d(np.array(c.a), np.array(c.b))
        assert (got == orc == want) or (np.isnan(got) and np.isnan(orc) and np.isnan(want)), (c, got, orc, want)
    # from a carry: a plain loop over np.float32
    n = 0
    with np.errstate(all="ignore"):
        for c in small_cases() + [rc.term_grid(*pair)[0] for pair in PAIRS]:
            res = c.carry
            for v in c.truth["sq"].tolist():
                res = F32(res + F32(v))
            assert rc.bits(res) == rc.bits(c.truth["final"]) or (np.isnan(res) and np.isnan(c.truth["final"])), c
            n += 1
    print("rmse1d of the reference, the oracle and np.add.accumulate agree on", len(cases), "vectors; a plain float32 loop from the carry on", n)


@pytest.mark.parametrize("m", [4096, 65536])
@pytest.mark.parametrize("kind", ["ahead", "behind"])
def test_guard_band_is_sound(kind, m):
    """device.decide_converged (the mirror of em_band / em_classify) on the families that approach the (m - 1) * 2^-24 bound its band
    rests on: 1.0 and then m - 1 squares just above half a unit of 1.0's grid, each of which the float32 sum rounds UP to a whole unit
    (ahead), or just below half a unit, each of which it absorbs (behind).  With the threshold one float32 step on either side of the
    serial sum, and over a sweep of thresholds, a decided float64 sum never contradicts  chain_diff(serial) < tole."""
    from wgsassign_amd import device
    filler = rc.nearest_root(rc.ONE + (1 << 13), 103, 1) if kind == "ahead" else rc.nearest_root(rc.TOP - (1 << 14), 102, -1)
    a = np.full(m, filler, dtype=F32)
    a[0] = 1.0
    sq = rc.squares(a, np.zeros(m, dtype=F32))
    F = rc.reference_chain(sq, F32(0))[1]
    S = math.fsum(sq.astype(np.float64).tolist())
    rel = abs(S - float(F)) / float(F) / ((m - 1) * 2.0 ** -24)
    print("%s, m = %d: serial %r, exact %r: apart by %.4f of (m - 1) * 2^-24 * serial" % (kind, m, F, S, rel))
    assert 0.4 < rel < 1.0                                            # (ahead: every addition errs by almost half a unit one way)
    steps = [F]
    for _ in range(3):
        steps = [np.nextafter(steps[0], F32(0))] + steps + [np.nextafter(steps[-1], F32(rc.INF))]
    toles = [device.chain_diff(x, m) for x in steps]
    toles += [t * (1 + s * 2.0 ** -50) for t in list(toles) for s in (-1, 1)]
    toles += [device.chain_diff(F, m) * f for f in np.linspace(0.5, 1.5, 2001)]
    decided = 0
    for tole in toles:
        d = device.decide_converged(S, m, tole)
        if d:
            decided += 1
            assert (d > 0) == (device.chain_diff(F, m) < tole), (kind, m, tole, d)
    assert 0 < decided < len(toles)                                   # far thresholds are decided, the near ones go to the chain
