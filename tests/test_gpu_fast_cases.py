"""The float32 mode (MODE_FAST) of every scoring kernel of csrc/assign_kernels.hip on the enumerated terms of tests/score_cases.py, and
of the two float32-slab EM kernels of csrc/em_kernels.hip on the cells of tests/em_cases.py, held twice:
    BITWISE to the restatement of tests/fast_cases.py, fed with the device's own fast_log values (one call of wgs_debug_fast_values on
            the distinct sums of a case): NaN where NaN is predicted, the same bits elsewhere, on `finite` AND on `hostile`;
    BY BOUND to the real-arithmetic reference on the terms of `finite` whose real sum is positive (fast_cases.term_bound, derived, no
            other tolerance anywhere), with the oracle's class -- -inf or NaN -- on the rest.
Each test forces one kernel and asserts through Score.plan() and codes_info() what ran, as tests/test_gpu_score_cases.py does:
    assign_kernel<KB, FAST>           wgs_debug_assign_parts_f64 at P = m: every term on its own, K = 4, 7, 8, 13, `grid` and `ragged`
    loglike_site_kernel<FAST>         into zeros and into the non-zero start vectors of the exact test (its add is a float32 add)
    score_sweep_kernel<., ., FAST, .> WGSASSIGN_CODES=0; shared columns K = 1, 4 .. 10, 13, 20, 23; per-individual columns of their own;
                                      a row range that cuts a pair; `grid`, `block`, `ragged`; cell sums = math.fsum of the restated terms
    score_coded_kernel<., FAST, ., .> float and float64 tables, batches of 16, 8 and 4, parts 1, 5 and 16, SNPs left uncoded; each cell
                                      also equal to the float32 direct sweep
    em_sweep_kernel<FAST>             one fit per population (EMBatch.sweep_paths()), two step()s from the enumerated frequencies of
                                      tests/em_cases.py, em_cases.negative_zero_sums, step()'s float64 sums under the existing rule;
                                      with the codes on offer too: no coded EM kernel may sweep in float32 mode
    em_sweep_group_kernel<FAST>       3, 4 and 5 re-fits per slab with a left-out column (a lone one goes to em_sweep_kernel)
The EM kernels' restatement takes the device's fast_rcp; their bound (fast_cases.update_bound) holds the first update of `finite`.
What this file found in its parent: DESIGN section 4 (g2 formed in float32; v_log_f32 on subnormal sums of either sign)."""
import functools
import math

import numpy as np
import pytest

import fast_cases as fc
import score_cases as sc

pytestmark = pytest.mark.gpu
F32 = np.float32
KERNELS = ("assign_kernel", "loglike_site_kernel", "score_sweep_kernel", "score_sweep_kernel PER_IND", "score_coded_kernel", "em_sweep_kernel",
           "em_sweep_group_kernel")
compared = {}                     # kernel -> results compared (printed by the last test)
BATCHES = {1: 4, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 10, 13: 7, 20: 10, 23: 8}         # K -> register batch of the sweep
SITE0 = 12345


@pytest.fixture(scope="module")
def dev():
    from wgsassign_amd import device
    device.get_context()
    return device


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for var in ("WGSASSIGN_MODE", "WGSASSIGN_PARTS", "WGS_SCORE_CODED_PARTS", "WGS_SCORE_CODED_TABLE", "WGSASSIGN_CODES_TABLE"):
        monkeypatch.delenv(var, raising=False)


def device_log(x):
    """fast_log of the device for float32 arguments (wgs_debug_fast_values)."""
    from wgsassign_amd import _lib, device
    x = np.ascontiguousarray(x, dtype=F32)
    out = np.empty_like(x)
    _lib.check(_lib.load().wgs_debug_fast_values(device.get_context().handle, 0, _lib.f32p(x), _lib.f32p(out), x.shape[0]))
    return out


@functools.lru_cache(maxsize=None)
def restated(variant, shape="grid", extra=0, at_chosen=False):
    """(case, V (n, K_ALL, m) float32): the restated float32-mode terms with the device's fast_log.  Made once, shared, read-only."""
    if extra:
        case = sc.build(variant, shape, extra=extra, extra_at=sc.uncoded_sites(shape) if at_chosen else None)
        for a in (case["L"], case["A"]):
            a.setflags(write=False)
    else:
        case = sc.case_of(variant, shape)
    V, distinct = fc.fast_terms(case, device_log)
    V.setflags(write=False)
    print("%s/%s%s: %d terms, %d distinct sums through the device's fast_log" % (variant, shape, " + %d" % extra if extra else "", V.size, distinct))
    return case, V


def on_device(dev, case, K, site0=0):
    b = dev.DeviceBeagle.from_host(case["L"], case["labels"].astype(np.int32), len(case["sizes"]), site0=site0)
    return b, dev.AFSet.from_host(np.ascontiguousarray(case["A"][:, :K]))


def per_individual(dev, case, K):
    n = case["L"].shape[1] // 2
    wide = dev.AFSet.from_host(np.ascontiguousarray(case["A"]))
    dummy = dev.AFSet.from_host(np.full((case["A"].shape[0], K), np.nan, dtype=F32))
    pops = np.stack([sc.permutation(i, K) for i in range(n)])
    colptr = np.array([[wide.col_dev(int(c)) for c in row] for row in pops], dtype=np.uint64)
    return wide, dummy, colptr, pops


def gathered(V, pops):
    return np.stack([V[i, pops[i]] for i in range(len(pops))])


def fail(what, kernel, got, want, bad, where):
    g, w = got.ravel()[bad], want.ravel()[bad]
    u = np.uint32 if got.dtype == F32 else np.uint64
    n_bad = int(((np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u)) & ~(np.isnan(got) & np.isnan(want))).sum())
    raise AssertionError("%s, %s: %d of %d results differ from the restatement, first at flat index %d: device %r (0x%x), restated %r (0x%x)\n    %s" % (
        what, kernel, n_bad, want.size, bad, g, int(np.array(g).view(u)), w, int(np.array(w).view(u)), where(bad)))


def describe(case, i, k, site, pops=None):
    col = k if pops is None else int(np.asarray(pops)[i][k])
    g0, g1, a = case["L"][site, 2 * i], case["L"][site, 2 * i + 1], case["A"][site, col]
    return sc.describe(case, i, k, site, pops) + "; float32 mode: s = %r" % float(fc.fast_sum(g0, g1, a))


def equal_terms(got, want, case, what, kernel, pops=None, order="ikm"):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    compared[kernel] = compared.get(kernel, 0) + want.size
    bad = sc.first_difference_any(got, want)
    if bad is not None:
        def where(flat):
            a, b, c = (int(x) for x in np.unravel_index(flat, want.shape))
            i, k, site = (a, b, c) if order == "ikm" else (a, c, b)
            return describe(case, i, k, site, pops)
        fail(what, kernel, got, want, bad, where)


def equal_cells(got, want, case, V, what, kernel, pops=None, P=1):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    compared[kernel] = compared.get(kernel, 0) + want.size
    bad = sc.first_difference_any(got, want)
    if bad is not None:
        def where(flat):
            row, k = (int(x) for x in np.unravel_index(flat, want.shape))
            i, p = row // P, row % P
            v = V[i, k]
            odd = np.flatnonzero(~np.isfinite(v) | (v > 0))
            site = int(odd[0]) if odd.size else 0
            return "cell (individual %d, population %d, partition %d of %d), %s; its first term that is not finite and <= 0, or its first: %s" % (
                i, k, p, P, sc.CELL_KINDS[int(sc.cell_kinds(v))], describe(case, i, k, site, pops))
        fail(what, kernel, got, want, bad, where)


def within_bound(terms, oracle_V, shape, what, K=sc.K_ALL):
    """terms (n, K, m) of the `finite` case against the real-arithmetic reference: within term_bound where the real sum is positive
    and the bound finite (everywhere but for sums below the float32 subnormals), the oracle's class elsewhere."""
    r = fc.real_of(shape)
    log, bound, sign = (np.ascontiguousarray(r[k].transpose(1, 2, 0))[:, :K] for k in ("log", "bound", "sign"))
    cmp_ = (sign > 0) & np.isfinite(bound)
    dev_ = np.abs(terms.astype(np.float64) - log)
    share = np.where(cmp_, dev_ / np.where(cmp_, bound, 1.0), 0.0)
    worst = np.unravel_index(int(np.argmax(share)), share.shape)
    print("%s: %d terms within bound (largest share of a bound %.4f: deviation %.3e of %.3e), %d by class" % (
        what, int(cmp_.sum()), float(share.max()), float(dev_[worst]), float(bound[worst]), int((~cmp_).sum())))
    assert np.isfinite(terms[cmp_]).all() and (share <= 1.0).all(), (what, worst, float(terms[worst]), float(log[worst]), float(bound[worst]))
    rest, ref = ~cmp_, oracle_V[:, :K]
    assert (np.isnan(ref[rest]) | np.isneginf(ref[rest])).all()
    assert np.array_equal(np.isnan(terms[rest]), np.isnan(ref[rest])) and np.array_equal(np.isneginf(terms[rest]), np.isneginf(ref[rest])), what
    return int(cmp_.sum())


# ---- the restatement with the device's fast_log against the real terms: what holds the kernels that return sums only ------------------
@pytest.mark.parametrize("shape", ["grid", "block", sc.RAGGED])
def test_restated_terms_within_bound(dev, oracle, shape):
    case, V = restated("finite", shape)
    _, ref = sc.reference(oracle, "finite", shape)
    assert within_bound(V, ref, shape, "restatement with the device's fast_log, finite/%s" % shape) == V.size - fc.NOT_POSITIVE[shape][0] - fc.UNBOUNDED[shape]
    # the float64 sum of every finite cell is exact in any order
    kinds = sc.cell_kinds(V)
    for i, k in zip(*np.nonzero(kinds == 0)):
        total, limit = sc.exact_sum_margin(V[i, k])
        assert total * 2 < limit, (shape, i, k, total, limit)
    # ... and the named terms: the pair (0.001, 0.999) at a = 1 (the reference's NaN) and next to it; (0, 1) at a = 1e-40 (-91.4)
    g0, g1 = F32(0.001), F32(0.999)
    assert np.isnan(device_log(fc.fast_sum(g0, g1, F32(1)).reshape(1)))[0]
    near = fc.real_terms(g0, g1, F32(1 - 2.0 ** -24))
    assert abs(float(device_log(fc.fast_sum(g0, g1, F32(1 - 2.0 ** -24)).reshape(1))[0]) - float(near["log"])) <= float(near["bound"])
    tiny = fc.real_terms(F32(0), F32(1), F32(1e-40))
    got = float(device_log(fc.fast_sum(F32(0), F32(1), F32(1e-40)).reshape(1))[0])
    assert abs(got - float(tiny["log"])) <= float(tiny["bound"]) and abs(got + 91.4) < 0.05, got


# ---- assign_kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 7, 8, 13])
@pytest.mark.parametrize("shape", ["grid", sc.RAGGED])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_assign_kernel_fast_mode(dev, oracle, variant, shape, K):
    from wgsassign_amd._lib import MODE_FAST
    case, V = restated(variant, shape)
    n, m = case["n_grid"], case["L"].shape[0]
    b, afs = on_device(dev, case, K)
    with np.errstate(all="ignore"):
        out, parts = dev.assign(b, afs, None, P=m, mode=MODE_FAST)
    what = "%s/%s, K = %d, P = m" % (variant, shape, K)
    equal_terms(parts.reshape(n, m, K), V[:, :K].transpose(0, 2, 1).astype(np.float64), case, what, "assign_kernel", order="imk")
    equal_cells(out, sc.expected_sums(V[:, :K]), case, V, what + ", totals", "assign_kernel")
    if variant == "finite":
        _, ref = sc.reference(oracle, variant, shape)
        within_bound(np.ascontiguousarray(parts.reshape(n, m, K).transpose(0, 2, 1)), ref, shape, "assign_kernel, " + what, K)
    afs.close()
    b.close()
    if shape == "grid":
        b, afs = on_device(dev, case, K, site0=SITE0)
        with np.errstate(all="ignore"):
            out, parts = dev.assign(b, afs, None, P=3, mode=MODE_FAST)
        labels = (SITE0 + np.arange(m)) % 3
        want = np.stack([sc.expected_sums(V[:, :K][:, :, labels == p]) for p in range(3)], axis=1).reshape(n * 3, K)
        equal_cells(parts, want, case, V, "%s, K = %d, P = 3, site0 = %d" % (variant, K, SITE0), "assign_kernel", P=3)
        afs.close()
        b.close()


# ---- loglike_site_kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_loglike_site_kernel_fast_mode(dev, oracle, monkeypatch, variant):
    """wgs_loglike in float32 mode: vec[s] = vec[s] + term, a float32 add -- into zeros, and into ordinary, -inf, huge, NaN and +inf
    starts."""
    from wgsassign_amd import glassy_cy
    monkeypatch.setenv("WGSASSIGN_MODE", "fast")
    case, V = restated(variant)
    n, m = case["n_grid"], case["L"].shape[0]
    start = np.array(sc.GOLDEN_STARTS, dtype=np.float64).astype(F32)[np.arange(m) % len(sc.GOLDEN_STARTS)]
    L, A = case["L"].copy(), case["A"].copy()
    got0, got1, want1 = np.zeros_like(V), np.empty_like(V), np.empty_like(V)
    with np.errstate(all="ignore"):
        for i in range(n):
            for k in range(sc.K_ALL):
                glassy_cy.loglike(L, A, got0[i, k], 1, i, k)
                got1[i, k] = np.roll(start, i + k)
                want1[i, k] = np.roll(start, i + k) + V[i, k]
                glassy_cy.loglike(L, A, got1[i, k], 1, i, k)
        want0 = F32(0) + V                                                   # (+0 + -0 = +0; the restated terms hold no -0 anyway)
    assert want1.dtype == F32
    equal_terms(got0, want0, case, "%s, into zeros" % variant, "loglike_site_kernel")
    equal_terms(got1, want1, case, "%s, into a non-zero vector" % variant, "loglike_site_kernel")
    if variant == "finite":
        _, ref = sc.reference(oracle, variant)
        within_bound(got0, ref, "grid", "loglike_site_kernel, finite/grid")


# ---- score_sweep_kernel -------------------------------------------------------------------------------------------------------------------
def sweep(dev, b, afs, colptr=None, rows=None):
    from wgsassign_amd._lib import MODE_FAST
    s = dev.Score(b, afs, colptr, rows)
    with np.errstate(all="ignore"):
        out = s.sums(MODE_FAST)
    plan = s.plan()
    s.close()
    return out, plan


@pytest.mark.parametrize("shape,K", [("grid", K) for K in (1, 4, 5, 6, 7, 8, 9, 10, 13, 20, 23)] + [("block", 6), ("block", 23), (sc.RAGGED, 6), (sc.RAGGED, 23)])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_score_sweep_kernel_fast_mode_shared_columns(dev, monkeypatch, variant, shape, K):
    monkeypatch.setenv("WGSASSIGN_CODES", "0")
    case, V = restated(variant, shape)
    b, afs = on_device(dev, case, K)
    out, plan = sweep(dev, b, afs)
    kb = BATCHES[K]
    print(variant, shape, K, plan)
    assert plan["path"] == 0 and (plan["kb"], plan["pairs"]) == (kb, 2 if kb <= 6 else 1), plan
    want = sc.expected_sums(V[:, :K])
    equal_cells(out, want, case, V, "%s/%s, K = %d" % (variant, shape, K), "score_sweep_kernel")
    if shape == "grid" and K in (4, 7):
        for lo, hi in ((3, 38), (0, 1), (17, 18), (51, 52)):                # row ranges that cut a pair of the wave and a slab
            part, plan = sweep(dev, b, afs, rows=(lo, hi))
            assert plan["path"] == 0
            only = np.zeros_like(want)
            only[lo:hi] = want[lo:hi]
            equal_cells(part, only, case, V, "%s, K = %d, rows [%d, %d)" % (variant, K, lo, hi), "score_sweep_kernel")
    afs.close()
    b.close()


@pytest.mark.parametrize("shape,K", [("grid", 4), ("grid", 5), ("grid", 10), ("block", 4), (sc.RAGGED, 4)])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_score_sweep_kernel_fast_mode_per_individual_columns(dev, monkeypatch, variant, shape, K):
    """Every individual points at K columns of its own of a 23-column set; the AFSet handed to the score holds NaN only."""
    monkeypatch.setenv("WGSASSIGN_CODES", "0")
    case, V = restated(variant, shape)
    b, _ = on_device(dev, case, 1)
    wide, dummy, colptr, pops = per_individual(dev, case, K)
    assert len({tuple(r) for r in pops.tolist()}) == len(pops)
    out, plan = sweep(dev, b, dummy, colptr)
    print(variant, shape, K, plan)
    assert plan["path"] == 0 and (plan["kb"], plan["pairs"]) == (BATCHES[K], 2 if K <= 4 else 1), plan
    Vp = gathered(V, pops)
    equal_cells(out, sc.expected_sums(Vp), case, Vp, "%s/%s, K = %d, per-individual columns" % (variant, shape, K), "score_sweep_kernel PER_IND", pops)
    for x in (dummy, wide, b):
        x.close()


# ---- score_coded_kernel -------------------------------------------------------------------------------------------------------------------
def coded(dev, monkeypatch, case, V, K, what, table_slots=64, batch=16, elem=None, parts=None, force_table=None, rich=0):
    """One float32-mode sweep through the class codes, held to the plan it must take, to the restated sums and to the direct sweep's bits."""
    monkeypatch.setenv("WGSASSIGN_CODES", "1")
    monkeypatch.setenv("WGSASSIGN_CODES_TABLE", str(table_slots))
    if parts is not None:
        monkeypatch.setenv("WGS_SCORE_CODED_PARTS", str(parts))
    if force_table is not None:
        monkeypatch.setenv("WGS_SCORE_CODED_TABLE", force_table)
    b, afs = on_device(dev, case, K)
    out, plan = sweep(dev, b, afs)
    info = b.codes_info()
    print(what, K, plan, {k: info[k] for k in ("available", "max_classes", "rich_snp_share", "score_batch_snps", "hash_slots")})
    kb = BATCHES[K]
    assert info["available"] and plan["path"] == 1 and plan["kb"] == kb, (plan, info)
    assert plan["score_batch"] == info["score_batch_snps"] == batch, (plan, info)
    assert plan["elem_bytes"] == (elem if elem is not None else (4 if batch == 16 and kb in (4, 7, 8) else 8)), plan
    assert abs(info["rich_snp_share"] - rich / case["L"].shape[0]) < 1e-9, info
    if parts is not None:
        assert plan["parts"] == parts, plan
    equal_cells(out, sc.expected_sums(V[:, :K]), case, V, what, "score_coded_kernel")
    monkeypatch.setenv("WGSASSIGN_CODES", "0")
    direct, plan0 = sweep(dev, b, afs)
    assert plan0["path"] == 0 and sc.same_bits64(direct, out)
    afs.close()
    b.close()


@pytest.mark.parametrize("K,table", [(4, None), (7, None), (8, None), (5, None), (10, None), (4, "d")])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_score_coded_kernel_fast_mode_tables_of_sixteen_snps(dev, monkeypatch, variant, K, table):
    """float rows at K = 4, 7 and 8, float64 rows at 5 and 10 and, forced, at 4; at K = 5 and 7 also the `ragged` shape."""
    case, V = restated(variant)
    coded(dev, monkeypatch, case, V, K, "%s, 16 SNPs per table%s" % (variant, ", float64 forced" if table else ""), force_table=table, elem=8 if table else None)
    if K in (5, 7):
        case, V = restated(variant, sc.RAGGED)
        coded(dev, monkeypatch, case, V, K, "%s/ragged, 16 SNPs per table" % variant)


@pytest.mark.parametrize("parts", [1, 5, 16])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_score_coded_kernel_fast_mode_parts_of_a_block(dev, monkeypatch, variant, parts):
    case, V = restated(variant, "block")
    coded(dev, monkeypatch, case, V, 5, "%s/block, %d parts" % (variant, parts), parts=parts)
    if parts == 5:
        coded(dev, monkeypatch, case, V, 23, "%s/block, %d parts, K = 23" % (variant, parts), parts=parts)


@pytest.mark.parametrize("extra,batch", [(36, 8), (48, 4)])
def test_score_coded_kernel_fast_mode_smaller_tables(dev, monkeypatch, extra, batch):
    case, V = restated("hostile", "grid", extra)
    coded(dev, monkeypatch, case, V, 4, "hostile + %d individuals, %d SNPs per table" % (extra, batch), table_slots=128, batch=batch, elem=8)
    coded(dev, monkeypatch, case, V, 7, "hostile + %d individuals, %d SNPs per table" % (extra, batch), table_slots=128, batch=batch, elem=8)


@pytest.mark.parametrize("shape,K", [("grid", 7), ("grid", 23), ("block", 7), ("block", 10)])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_score_coded_kernel_fast_mode_uncoded_snps(dev, monkeypatch, variant, shape, K):
    """SNPs the encoder leaves uncoded: their terms come straight from the float32 slab, for both halves of both pairs of every quad."""
    case, V = restated(variant, shape, 48, True)
    rich, batch = len(sc.uncoded_sites(shape)), sc.table_snps(case["L"])
    assert batch == {("finite", "grid"): 8, ("hostile", "grid"): 4}.get((variant, shape), 16)
    coded(dev, monkeypatch, case, V, K, "%s/%s, %d SNPs left uncoded" % (variant, shape, rich), batch=batch, elem=8 if batch < 16 else None, rich=rich)


# ---- em_sweep_kernel<FAST>, em_sweep_group_kernel<FAST> ----------------------------------------------------------------------------------
EM_KERNELS = ("em_sweep_kernel", "em_sweep_group_kernel", "em_coded_kernel", "em_coded_group_kernel")


def device_rcp(x):
    """fast_rcp of the device for float32 arguments (wgs_debug_fast_values)."""
    from wgsassign_amd import _lib, device
    x = np.ascontiguousarray(x, dtype=F32)
    out = np.empty_like(x)
    _lib.check(_lib.load().wgs_debug_fast_values(device.get_context().handle, 1, _lib.f32p(x), _lib.f32p(out), x.shape[0]))
    return out


def em_force(monkeypatch, how="codes off"):
    """The environment of tests/test_gpu_em_cases.py that sends exact sweeps to the float32-slab kernels -- and, with the codes built
    and on offer, the one in which only the mode keeps a sweep from the coded kernels (em_api.hip: no coded kernel in MODE_FAST)."""
    if how == "codes off":
        monkeypatch.setenv("WGSASSIGN_CODES", "0")
    else:
        monkeypatch.setenv("WGSASSIGN_CODES", "1")
        monkeypatch.setenv("WGSASSIGN_EM_CODES_SWEEPS", "0")
        monkeypatch.setenv("WGSASSIGN_EM_CODES_MIN", "1")
    monkeypatch.setenv("WGSASSIGN_EM_FUSE", "1")
    monkeypatch.delenv("WGSASSIGN_EM_MODE", raising=False)


def em_swept(em, before, kernel):
    after = em.sweep_paths()
    delta = [a - b for a, b in zip(after, before)]
    i = EM_KERNELS.index(kernel)
    assert delta[i] == 1 and all(d == 0 for j, d in enumerate(delta) if j != i), "%s expected once, the sweeps went %r" % (kernel, dict(zip(EM_KERNELS, delta)))
    return after


def em_equal(got, want, grid, fits, what, kernel):
    import em_cases as ec
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    compared[kernel] = compared.get(kernel, 0) + want.size
    bad = ec.first_difference(got, want)
    if bad is not None:
        j, site = (int(x) for x in np.unravel_index(bad, want.shape))
        n_bad = int(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).sum())
        raise AssertionError("%s, %s: %d of %d results differ from the restatement, first at fit %d, site %d: device %r (0x%08x), restated %r (0x%08x)\n    %s" % (
            what, kernel, n_bad, want.size, j, site, got[j, site], got.view(np.uint32)[j, site], want[j, site], want.view(np.uint32)[j, site],
            ec.describe(grid, fits[j][0], site, fits[j][1]) if "cell" in grid else "population %d" % fits[j][0]))
    assert ec.same_nan(want, got), what


def em_sums_agree(ssq, f_new, f_old, what):
    """step()'s float64 sums under the rule of tests/test_gpu_em_cases.py: sums_agree."""
    import em_cases as ec
    for j in range(len(ssq)):
        sq = ec.squares(f_new[j], f_old[j])
        if not np.isfinite(sq).all():
            assert not math.isfinite(ssq[j]), (what, j, ssq[j])
        else:
            exact = math.fsum(sq.astype(np.float64))
            assert math.isfinite(ssq[j]) and abs(ssq[j] - exact) <= len(sq) * 2.0 ** -53 * exact, (what, j, ssq[j], exact)


def em_within_bound(got, fits, what):
    """The first update of `finite` against the real-arithmetic one, on the (fit, site) whose terms all have a positive real sum."""
    n = 0
    worst = 0.0
    for j, (k, skip) in enumerate(fits):
        F, bound, cmp_ = fc.em_real_of(k, skip)
        share = np.abs(got[j].astype(np.float64) - F)[cmp_] / bound[cmp_]
        assert np.isfinite(got[j][cmp_]).all() and (share <= 1.0).all(), (what, j, k, skip, float(share.max()))
        worst, n = max(worst, float(share.max())), n + int(cmp_.sum())
    print("%s: %d (fit, site) within bound, largest share of a bound %.4f" % (what, n, worst))
    return n


def em_run(dev, monkeypatch, grid, groups, skips, fits, olds, kernel, what, updates=2, finite=False):
    """`updates` step()s of a float32-mode batch from `olds`, each held to the restatement with the device's fast_rcp."""
    import em_cases as ec
    from wgsassign_amd._lib import MODE_FAST
    b = dev.DeviceBeagle.from_host(grid["L"], grid["labels"].astype(np.int32), len(grid["sizes"]))
    em = dev.EMBatch(b, np.array(groups, dtype=np.int32), None if skips is None else np.array(skips, dtype=np.int32), mode=MODE_FAST)
    for j in range(em.n_fits):
        em.set_f(j, olds[j])
    paths, prev = em.sweep_paths(), np.stack(olds)
    for u in range(updates):
        with np.errstate(all="ignore"):
            ssq = em.step()
        paths = em_swept(em, paths, kernel)
        got = np.stack([em.get_f(j) for j in range(em.n_fits)])
        want = np.stack([fc.fast_update(ec.columns(grid["L"], grid["members"][k]), prev[j], device_rcp, skip=skip) for j, (k, skip) in enumerate(fits)])
        em_equal(got, want, grid, fits, "%s, update %d" % (what, u + 1), kernel)
        em_sums_agree(ssq, want, prev, "%s, update %d" % (what, u + 1))
        if finite and u == 0:
            em_within_bound(got, fits, "%s, %s" % (kernel, what))
        prev = want
    em.close()
    b.close()


@pytest.mark.parametrize("how", ["codes off", "codes on offer"])
@pytest.mark.parametrize("variant", ["finite", "hostile"])
def test_em_sweep_kernel_fast_mode(dev, monkeypatch, variant, how):
    """One fit per population, two step()s from the enumerated frequencies.  With the class codes built and on offer it is still
    em_sweep_kernel that sweeps: no coded EM kernel runs in float32 mode."""
    import em_cases as ec
    grid = ec.grid_of(variant)
    K = len(grid["sizes"])
    em_force(monkeypatch, how)
    em_run(dev, monkeypatch, grid, np.arange(K), None, [(k, None) for k in range(K)], [grid["f_old"][k] for k in range(K)], "em_sweep_kernel",
           "%s, one fit per population, %s" % (variant, how), finite=variant == "finite")


@pytest.mark.parametrize("count", [1, 3, 4, 5])
@pytest.mark.parametrize("variant", ["finite", "hostile"])
def test_em_sweep_group_kernel_fast_mode(dev, monkeypatch, variant, count):
    """1, 3, 4 and 5 re-fits of each of the populations of 9, 17, 33 and 49, each with a left-out column: a lone re-fit goes to
    em_sweep_kernel (its checked buffer holds the left-out individual), 3 and 4 share a tile, 5 make two groups."""
    import em_cases as ec
    grid = ec.grid_of(variant)
    em_force(monkeypatch)
    groups, skips, fits, olds = [], [], [], []
    for k in [ec.SIZES.index(size) for size in ec.LOO_SIZES]:
        g, s, cols = ec.loo_fits(grid, k, count)
        groups += list(g)
        skips += list(s)
        fits += [(k, c) for c in cols]
        olds += [grid["f_old"][k]] * count
    em_run(dev, monkeypatch, grid, groups, skips, fits, olds, "em_sweep_kernel" if count == 1 else "em_sweep_group_kernel",
           "%s, %d re-fits per slab" % (variant, count), finite=variant == "finite")


def test_em_fast_mode_a_running_sum_of_negative_zero(dev, monkeypatch):
    """em_cases.negative_zero_sums in float32 mode: the restatement decides what the sign of each zero is, the kernel has its bits."""
    import em_cases as ec
    case = ec.negative_zero_sums()
    K = len(case["sizes"])
    em_force(monkeypatch)
    em_run(dev, monkeypatch, case, np.arange(K), None, [(k, None) for k in range(K)], [case["f_old"][k] for k in range(K)], "em_sweep_kernel",
           "negative zero sums", updates=1)


def test_every_fast_kernel_was_compared():
    """(Last in the file: how many results each kernel was held to.)"""
    print("compared results per float32-mode kernel: %r" % compared)
    if compared:                                           # (empty when this test is selected alone)
        assert set(KERNELS) <= set(compared) and all(compared[k] >= 2000 for k in KERNELS), compared
