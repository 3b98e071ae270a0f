"""Every kernel of csrc/assign_kernels.hip on the enumerated terms of tests/score_cases.py: likelihood sums that are +inf, negative, a
subnormal of either sign, finite above 1, zero or NaN, each at lanes 0 and 63, in the ragged tile, in both halves of a wave's pair, in
every column of a quad, at the ends of slabs of 1 to 16 columns, at the block edge and at the end of every part.  Every comparison is
of bits: NaN exactly where the reference has NaN, the same bits elsewhere, the sign of an infinity included; there is no tolerance and
no cell is left out.  The yardstick is the oracle (oracle/wgs_oracle.c), which tests/test_score_cases_cpu.py ties to the real
reference on these inputs (tests/golden/score_cases.npz) and which holds the builders to what they claim -- among it that the float64
sum of every finite cell is exact in any order, so that the expected sum is math.fsum of the oracle's float32 values.  The oracle's
values are computed once per variant and shape, shared and read-only.

Each test forces one kernel and asserts through Score.plan() and codes_info() that this kernel, with this register batch, these pairs
per wave, this table and these parts ran:
    parts_exact_kernel      P = m: every site its own partition, so every TERM is compared on its own (the anchor of site_ll_exact)
    assign_kernel           exact mode through wgs_debug_assign_parts_f64: P = m every term as float64; P = 3 at site0 = 12345
    score_sweep_kernel      WGSASSIGN_CODES=0; shared columns K = 1 .. 23 (batches 4 to 10, one and two pairs per wave, padded slots
                            that repeat a hostile population), a row range that cuts a pair, per-individual columns that differ;
                            the `ragged` shape, whose only terms that are not finite stand in the ragged tile (a sum is poisoned
                            by its first such term, and the other shapes have one in every tile)
    score_coded_kernel      float and float64 tables of 16 SNPs, tables of 8 and of 4, parts 1, 5 and 16, SNPs left uncoded
    chain_cand / chain_walk parts_exact(P) against np.add.at and the literal kernel, site0, carries, per-individual columns
    loglike_site_kernel     wgs_loglike into zeros and into non-zero vectors
The float32 mode (MODE_FAST) of the same kernels is held on the same inputs, bit for bit to a float32 restatement and by a derived bound
to the real-arithmetic term, by tests/test_gpu_fast_cases.py (tests/fast_cases.py)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import score_cases as sc

pytestmark = pytest.mark.gpu
F32 = np.float32
KERNELS = ("parts_exact_kernel", "assign_kernel", "score_sweep_kernel", "score_sweep_kernel PER_IND", "score_coded_kernel", "chain kernels",
           "loglike_site_kernel")
compared = {}                     # kernel -> results compared (printed by the last test)
# K -> (register batch of the sweep, of the chain kernel): the table of tests/test_gpu_assign_k.py
BATCHES = {1: (4, 4), 4: (4, 4), 5: (5, 5), 6: (6, 6), 7: (7, 7), 8: (8, 8), 9: (9, 5), 10: (10, 5), 13: (7, 7), 20: (10, 7), 23: (8, 8)}
SITE0 = 12345


@pytest.fixture(scope="module")
def dev():
    from wgsassign_amd import device
    device.get_context()
    return device


@pytest.fixture(autouse=True)
def _exact_mode(monkeypatch):
    for var in ("WGSASSIGN_MODE", "WGSASSIGN_PARTS", "WGS_SCORE_CODED_PARTS", "WGS_SCORE_CODED_TABLE", "WGSASSIGN_CODES_TABLE"):
        monkeypatch.delenv(var, raising=False)


def lib():
    return __import__("wgsassign_amd._lib", fromlist=["x"])


def on_device(dev, case, K, site0=0):
    b = dev.DeviceBeagle.from_host(case["L"], case["labels"].astype(np.int32), len(case["sizes"]), site0=site0)
    return b, dev.AFSet.from_host(np.ascontiguousarray(case["A"][:, :K]))


def per_individual(dev, case, K):
    """(wide AFSet of all 23 columns, a K-column AFSet of NaN that nothing may read, colptr (n, K), pops (n, K)): every individual points
    at K columns of its own of the wide set (score_cases.permutation)."""
    n = case["L"].shape[1] // 2
    wide = dev.AFSet.from_host(np.ascontiguousarray(case["A"]))
    dummy = dev.AFSet.from_host(np.full((case["A"].shape[0], K), np.nan, dtype=F32))
    pops = np.stack([sc.permutation(i, K) for i in range(n)])
    colptr = np.array([[wide.col_dev(int(c)) for c in row] for row in pops], dtype=np.uint64)
    assert len({tuple(r) for r in pops.tolist()}) == n           # no two individuals share their columns
    return wide, dummy, colptr, pops


def gathered(V, pops):
    """V (n, K_ALL, m) -> (n, K, m): individual i against the columns pops[i] (the oracle on A[:, pops[i]])."""
    return np.stack([V[i, pops[i]] for i in range(len(pops))])


def fail(what, kernel, got, want, bad, where):
    g, w = got.ravel()[bad], want.ravel()[bad]
    u = np.uint32 if got.dtype == F32 else np.uint64
    n_bad = int(((np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u)) & ~(np.isnan(got) & np.isnan(want))).sum())
    raise AssertionError("%s, %s: %d of %d results differ, first at flat index %d: device %r (0x%x), reference %r (0x%x)\n    %s" % (
        what, kernel, n_bad, want.size, bad, g, int(np.array(g).view(u)), w, int(np.array(w).view(u)), where(bad)))


def equal_terms(got, want, case, what, kernel, pops=None, order="ikm"):
    """got, want (n, K, m) (order ikm) or (n, m, K) (order imk) per-term values; names the first term that differs."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    compared[kernel] = compared.get(kernel, 0) + want.size
    bad = sc.first_difference_any(got, want)
    if bad is not None:
        def where(flat):
            a, b, c = (int(x) for x in np.unravel_index(flat, want.shape))
            i, k, site = (a, b, c) if order == "ikm" else (a, c, b)
            return sc.describe(case, i, k, site, pops)
        fail(what, kernel, got, want, bad, where)


def equal_cells(got, want, case, V, what, kernel, pops=None, P=1):
    """got, want (n * P, K) sums of cells; names the first cell that differs, its kind and its first term that is not an ordinary one."""
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
                i, k, p, P, sc.CELL_KINDS[int(sc.cell_kinds(v))], sc.describe(case, i, k, site, pops))
        fail(what, kernel, got, want, bad, where)


@functools.lru_cache(maxsize=None)
def extended(variant, extra, at_chosen, shape="grid"):
    """(case, V) of build(variant, shape, extra=..., extra_at=...): made once, shared, read-only."""
    from oracle import oracle as orc
    orc.build()
    case = sc.build(variant, shape, extra=extra, extra_at=sc.uncoded_sites(shape) if at_chosen else None)
    V = sc.per_site(orc, case["L"], case["A"])
    for a in (case["L"], case["A"], V):
        a.setflags(write=False)
    return case, V


# ---- parts_exact_kernel: every term on its own -----------------------------------------------------------------------------------------
CARRIES = (-1.5, 1e-3, -3e38, 3e38, 0.0, -math.inf, math.inf, -2.0 ** -140)


@pytest.mark.parametrize("carried", [False, True], ids=["from zero", "carry"])
@pytest.mark.parametrize("columns", ["shared", "per individual"])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_parts_exact_kernel_every_term(dev, oracle, variant, columns, carried):
    """P = m: partition p is site p alone, so parts[i * m + p, k] = carry + v(i, k, p) in float32 -- every term of every cell."""
    case, V = sc.reference(oracle, variant)
    n, m = case["n_grid"], case["L"].shape[0]
    L = lib()
    if columns == "shared":
        K, pops, want_v = sc.K_ALL, None, V
        b, afs = on_device(dev, case, K)
        keep, cp = None, None
    else:
        K = 10
        b, _ = on_device(dev, case, 1)
        keep, afs, colptr, pops = per_individual(dev, case, K)
        want_v = gathered(V, pops)
        cp = colptr.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p))
    carry = None
    if carried:
        carry = np.array(CARRIES, dtype=np.float64).astype(F32)[(np.arange(n * m * K) * 7 // 3) % len(CARRIES)].reshape(n * m, K)
    got = np.zeros((n * m, K), dtype=F32)
    L.check(L.load().wgs_debug_parts_exact_literal(b.handle, afs.handle, cp, m, L.f32p(carry) if carried else None, L.f32p(got)))
    want = np.ascontiguousarray(want_v.transpose(0, 2, 1))                   # (n, m, K)
    if carried:
        with np.errstate(all="ignore"):
            want = (carry.reshape(n, m, K) + want).astype(F32)
    equal_terms(got.reshape(n, m, K), want, case, "%s, %s columns, %s" % (variant, columns, "carry" if carried else "from zero"), "parts_exact_kernel",
                pops, order="imk")
    for x in (afs, keep, b):
        if x is not None:
            x.close()


# ---- assign_kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 7, 8, 13])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_assign_kernel_exact_mode(dev, oracle, variant, K):
    from wgsassign_amd._lib import MODE_EXACT
    case, V = sc.reference(oracle, variant)
    n, m = case["n_grid"], case["L"].shape[0]
    b, afs = on_device(dev, case, K)
    with np.errstate(all="ignore"):
        out, parts = dev.assign(b, afs, None, P=m, mode=MODE_EXACT)
    equal_terms(parts.reshape(n, m, K), V[:, :K].transpose(0, 2, 1).astype(np.float64), case, "%s, K = %d, P = m" % (variant, K), "assign_kernel", order="imk")
    equal_cells(out, sc.expected_sums(V[:, :K]), case, V, "%s, K = %d, totals at P = m" % (variant, K), "assign_kernel")
    afs.close()
    b.close()
    # P = 3 with global labels: the float64 partition sums (exact on the finite cells in any order)
    b, afs = on_device(dev, case, K, site0=SITE0)
    with np.errstate(all="ignore"):
        out, parts = dev.assign(b, afs, None, P=3, mode=MODE_EXACT)
    labels = (SITE0 + np.arange(m)) % 3
    want = np.stack([sc.expected_sums(V[:, :K][:, :, labels == p]) for p in range(3)], axis=1).reshape(n * 3, K)
    equal_cells(parts, want, case, V, "%s, K = %d, P = 3, site0 = %d" % (variant, K, SITE0), "assign_kernel", P=3)
    afs.close()
    b.close()


# ---- score_sweep_kernel -------------------------------------------------------------------------------------------------------------------
def sweep(dev, b, afs, colptr=None, rows=None):
    from wgsassign_amd._lib import MODE_EXACT
    s = dev.Score(b, afs, colptr, rows)
    with np.errstate(all="ignore"):
        out = s.sums(MODE_EXACT)
    plan = s.plan()
    s.close()
    return out, plan


@pytest.mark.parametrize("shape,K", [("grid", K) for K in (1, 4, 6, 7, 10, 13, 20, 23)] + [("block", 6), ("block", 23), (sc.RAGGED, 6), (sc.RAGGED, 23)])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_score_sweep_kernel_shared_columns(dev, oracle, monkeypatch, variant, shape, K):
    monkeypatch.setenv("WGSASSIGN_CODES", "0")
    case, V = sc.reference(oracle, variant, shape)
    if variant == "hostile" and K in (1, 13, 23):
        assert case["freq_family"][K - 1] in ("negs", "negh", "infnan")             # the population the padded slots repeat is a hostile one
    b, afs = on_device(dev, case, K)
    out, plan = sweep(dev, b, afs)
    kb = BATCHES[K][0]
    print(variant, shape, K, plan)
    assert plan["path"] == 0 and (plan["kb"], plan["pairs"]) == (kb, 2 if kb <= 6 else 1), plan
    want = sc.expected_sums(V[:, :K])
    equal_cells(out, want, case, V, "%s/%s, K = %d" % (variant, shape, K), "score_sweep_kernel")
    if shape == "grid" and K in (4, 7):
        # row ranges that cut a pair of the wave and a slab: only their individuals are scored, with the same bits
        for lo, hi in ((3, 38), (0, 1), (17, 18), (51, 52)):
            part, plan = sweep(dev, b, afs, rows=(lo, hi))
            assert plan["path"] == 0
            only = np.zeros_like(want)
            only[lo:hi] = want[lo:hi]
            equal_cells(part, only, case, V, "%s, K = %d, rows [%d, %d)" % (variant, K, lo, hi), "score_sweep_kernel")
    afs.close()
    b.close()


@pytest.mark.parametrize("shape,K", [("grid", 4), ("grid", 5), ("grid", 10), ("block", 4), (sc.RAGGED, 4)])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_score_sweep_kernel_per_individual_columns(dev, oracle, monkeypatch, variant, shape, K):
    """Every individual points at K columns of its own of a 23-column set; the AFSet handed to the score holds NaN only."""
    monkeypatch.setenv("WGSASSIGN_CODES", "0")
    case, V = sc.reference(oracle, variant, shape)
    b, _ = on_device(dev, case, 1)
    wide, dummy, colptr, pops = per_individual(dev, case, K)
    out, plan = sweep(dev, b, dummy, colptr)
    print(variant, shape, K, plan)
    assert plan["path"] == 0 and (plan["kb"], plan["pairs"]) == (BATCHES[K][0], 2 if K <= 4 else 1), plan
    Vp = gathered(V, pops)
    equal_cells(out, sc.expected_sums(Vp), case, Vp, "%s/%s, K = %d, per-individual columns" % (variant, shape, K), "score_sweep_kernel PER_IND", pops)
    for x in (dummy, wide, b):
        x.close()


# ---- score_coded_kernel -------------------------------------------------------------------------------------------------------------------
def coded(dev, monkeypatch, case, V, K, what, table_slots=64, batch=16, elem=None, parts=None, force_table=None, rich=0):
    """One sweep through the class codes, held to the plan it must take, to the expected sums and to the direct sweep's bits."""
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
    kb = BATCHES[K][0]
    assert info["available"] and plan["path"] == 1 and plan["kb"] == kb, (plan, info)
    assert plan["score_batch"] == info["score_batch_snps"] == batch, (plan, info)
    assert plan["elem_bytes"] == (elem if elem is not None else (4 if batch == 16 and kb in (4, 7, 8) else 8)), plan
    assert abs(info["rich_snp_share"] - rich / case["L"].shape[0]) < 1e-9, info
    if parts is not None:
        assert plan["parts"] == parts, plan
    want = sc.expected_sums(V[:, :K])
    equal_cells(out, want, case, V, what, "score_coded_kernel")
    monkeypatch.setenv("WGSASSIGN_CODES", "0")
    direct, plan0 = sweep(dev, b, afs)
    assert plan0["path"] == 0 and sc.same_bits64(direct, out)
    afs.close()
    b.close()


@pytest.mark.parametrize("K,table", [(4, None), (7, None), (8, None), (5, None), (6, None), (9, None), (10, None), (4, "d")])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_score_coded_kernel_tables_of_sixteen_snps(dev, oracle, monkeypatch, variant, K, table):
    """float rows at K = 4, 7 and 8, float64 rows at 5, 6, 9 and 10 and, forced, at 4."""
    case, V = sc.reference(oracle, variant)
    coded(dev, monkeypatch, case, V, K, "%s, 16 SNPs per table%s" % (variant, ", float64 forced" if table else ""), force_table=table, elem=8 if table else None)
    if K in (5, 7):
        # ... and where the ragged tile's five SNPs, a part's last batch, are the only ones with a term that is not finite
        case, V = sc.reference(oracle, variant, sc.RAGGED)
        coded(dev, monkeypatch, case, V, K, "%s/ragged, 16 SNPs per table" % variant)


@pytest.mark.parametrize("parts", [1, 5, 16])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_score_coded_kernel_parts_of_a_block(dev, oracle, monkeypatch, variant, parts):
    """4096 + 64 + 5 sites: a block shared by 1, 5 and 16 workgroups (runs of 64, 13 and 4 tiles), a second block of a tile and a
    ragged one, combine_parts_kernel and block_prefix_kernel behind them; terms at the end of every run."""
    case, V = sc.reference(oracle, variant, "block")
    coded(dev, monkeypatch, case, V, 5, "%s/block, %d parts" % (variant, parts), parts=parts)
    if parts == 5:
        coded(dev, monkeypatch, case, V, 23, "%s/block, %d parts, K = 23" % (variant, parts), parts=parts)


@pytest.mark.parametrize("extra,batch", [(36, 8), (48, 4)])
def test_score_coded_kernel_smaller_tables(dev, monkeypatch, extra, batch):
    """A slab of `extra` more individuals with an ordinary pair of their own each pushes the classes per SNP over 616 / 16 (and 616 / 8):
    tables of 8 and of 4 SNPs, float64 rows whatever the register batch."""
    case, V = extended("hostile", extra, False)
    cl = sc.classes_per_snp(case["L"])
    assert (cl.max() * 8 <= 616 < cl.min() * 16) if batch == 8 else (cl.min() * 8 > 616)
    coded(dev, monkeypatch, case, V, 4, "hostile + %d individuals, %d SNPs per table" % (extra, batch), table_slots=128, batch=batch, elem=8)
    coded(dev, monkeypatch, case, V, 7, "hostile + %d individuals, %d SNPs per table" % (extra, batch), table_slots=128, batch=batch, elem=8)


@pytest.mark.parametrize("shape,K", [("grid", 7), ("grid", 23), ("block", 7), ("block", 10)])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_score_coded_kernel_uncoded_snps(dev, monkeypatch, variant, shape, K):
    """At score_cases.uncoded_sites 48 more individuals have a pair of their own each: more classes than the encoder's 64-slot tables
    hold, so those SNPs stay uncoded (ncls = 0) and the coded sweep takes their terms -- one of every class among them -- from the
    float32 slab, for both halves of both pairs of every quad.  In the grid case they are 12 sites of 197, which also raises the 99th
    percentile of the classes per SNP: a table of 8 (`finite`) or 4 SNPs (`hostile`) and float64 rows; in the block case 11 of 4165 leave it alone: 16 SNPs,
    float rows at K = 7 (whose phase 2 skips an uncoded SNP by a branch) and float64 rows at K = 10 (which reads the row of zeros)."""
    case, V = extended(variant, 48, True, shape)
    rich, batch = len(sc.uncoded_sites(shape)), sc.table_snps(case["L"])
    assert batch == {("finite", "grid"): 8, ("hostile", "grid"): 4}.get((variant, shape), 16)
    coded(dev, monkeypatch, case, V, K, "%s/%s, %d SNPs left uncoded" % (variant, shape, rich), batch=batch, elem=8 if batch < 16 else None, rich=rich)


# ---- chain_cand_kernel + chain_walk_kernel ------------------------------------------------------------------------------------------------
def test_the_chains_meet_what_they_are_built_for(oracle):
    """In the block case of `hostile` (K = 13): finite cells with positive values (s > 1), chains with +inf and then -inf, a -inf at the
    first and at the last site of a partition."""
    case, V = sc.reference(oracle, "hostile", "block")
    V = V[:, :13]
    m = V.shape[-1]
    kinds = sc.cell_kinds(V)
    assert ((kinds == 0) & (V > 0).any(axis=-1)).sum() >= 8
    first_p, first_n = np.argmax(np.isposinf(V), axis=-1), np.argmax(np.isneginf(V), axis=-1)
    assert (np.isposinf(V).any(axis=-1) & np.isneginf(V).any(axis=-1) & ~np.isnan(V).any(axis=-1) & (first_p < first_n)).any()
    for P in (2, 3, 7, 64):
        assert np.isneginf(V[:, :, :P]).any() and np.isneginf(V[:, :, m - P:]).any()


@pytest.mark.parametrize("P", [1, 2, 3, 7, 64])
@pytest.mark.parametrize("columns,site0", [("shared", 0), ("shared", SITE0), ("per individual", SITE0)])
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_chain_kernels(dev, oracle, monkeypatch, variant, columns, site0, P):
    """parts_exact(P): the reference's serial float32 np.add.at sums, against NumPy on the oracle's values and against the literal
    kernel; then continued from a non-zero float32 carry (wgs_assign_parts_exact)."""
    monkeypatch.setenv("WGSASSIGN_CODES", "0")
    case, V = sc.reference(oracle, variant, "block")
    n = case["n_grid"]
    L = lib()
    if columns == "shared":
        K, pops, Vk = 13, None, V[:, :13]
        b, afs = on_device(dev, case, K, site0=site0)
        keep, colptr, cp = None, None, None
    else:
        K = 5
        b, _ = on_device(dev, case, 1, site0=site0)
        keep, afs, colptr, pops = per_individual(dev, case, K)
        Vk = gathered(V, pops)
        cp = colptr.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p))
    s = dev.Score(b, afs, colptr)
    with np.errstate(all="ignore"):
        got = s.parts_exact(P)
    plan, (redone, walked) = s.plan(), s.serial_blocks()
    s.close()
    ckb = BATCHES[K][1]
    print(variant, columns, site0, P, plan, "blocks redone serially %d of %d walked" % (redone, walked))
    assert plan["path"] == 0 and (plan["chain_kb"], plan["chain_pairs"]) == (ckb, 2 if ckb <= 4 and columns == "shared" else 1), plan
    if variant == "finite":
        assert walked - redone >= 1, (redone, walked)                       # a block on the parallel path
    want = sc.partition_sums(Vk, P, site0)
    what = "%s/block, %s columns, site0 = %d, P = %d" % (variant, columns, site0, P)
    equal_cells(got, want, case, Vk, what, "chain kernels", pops, P=P)
    lit = dev.partition_sums_exact(b, afs, colptr, P=P, literal=True)
    equal_cells(lit, want, case, Vk, what + ", literal", "parts_exact_kernel", pops, P=P)
    # from a carry, as the second of two SNP shards
    carry = -(np.random.default_rng(P).random((n * P, K)) * 3e3).astype(F32)
    carry[::5] = 0.0
    carry[3::11] = np.float32(2.5)
    cont = np.zeros_like(carry)
    L.check(L.load().wgs_assign_parts_exact(b.handle, afs.handle, cp, P, L.f32p(carry), L.f32p(cont)))
    equal_cells(cont, sc.partition_sums(Vk, P, site0, carry), case, Vk, what + ", from a carry", "chain kernels", pops, P=P)
    for x in (afs, keep, b):
        if x is not None:
            x.close()


# ---- loglike_site_kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_loglike_site_kernel(oracle, variant):
    """wgs_loglike (the thin mirror of glassy_cy.loglike): every term into zeros, and every term accumulated into a vector of ordinary,
    -inf, huge, NaN and +inf starts -- vec[s] = (float)((double)vec[s] + log((double)s))."""
    from wgsassign_amd import glassy_cy
    case, V = sc.reference(oracle, variant)
    n, m = case["n_grid"], case["L"].shape[0]
    start = np.array(sc.GOLDEN_STARTS, dtype=np.float64).astype(F32)[np.arange(m) % len(sc.GOLDEN_STARTS)]
    L, A = case["L"].copy(), case["A"].copy()                               # (the mirror takes writeable buffers, as Cython's memoryviews do)
    got0, got1, want1 = np.zeros_like(V), np.empty_like(V), np.empty_like(V)
    with np.errstate(all="ignore"):
        for i in range(n):
            for k in range(sc.K_ALL):
                glassy_cy.loglike(L, A, got0[i, k], 1, i, k)
                got1[i, k] = want1[i, k] = np.roll(start, i + k)
                glassy_cy.loglike(L, A, got1[i, k], 1, i, k)
                oracle.loglike(L, A, want1[i, k], 1, i, k)
    equal_terms(got0, V, case, "%s, into zeros" % variant, "loglike_site_kernel")
    equal_terms(got1, want1, case, "%s, into a non-zero vector" % variant, "loglike_site_kernel")


def test_every_kernel_was_compared():
    """(Last in the file: how many results each kernel was held to.)"""
    print("compared results per kernel: %r" % compared)
    if compared:                                           # (empty when this test is selected alone)
        assert set(KERNELS) <= set(compared) and all(compared[k] >= 2000 for k in KERNELS), compared
