"""What a scoring call decides before it enqueues anything (csrc/score_api.hip: score_plan_sums, read back with
wgs_debug_score_plan / Score.plan()): the sweep over the float32 slabs or through the class codes, the register batch and the
pairs per wave of the sweep and of the chain kernel, the coded sweep's table and how many workgroups share a block.  A test that
only compares "through the codes" with "direct" passes when both legs take the same kernel; here every case names the kernel it
expects AND holds the sums to the oracle.

Matrices: 4097 SNPs (two blocks, the second a single SNP) x 37 individuals in K population slabs.  The expected register batches
are the table in the docstring of tests/test_gpu_assign_k.py (the batch with the fewest passes over K, then the least padding; the
chain kernel stays at 8 or fewer), two pairs per wave where the sweep's batch is <= 6 (per-individual columns: <= 4; chain kernel:
<= 4 and shared columns only)."""
import functools

import numpy as np
import pytest

import synth
from test_gpu_parity import same, same_nan

pytestmark = pytest.mark.gpu

M, N = 4097, 37
# K: (register batch of the sweep, of the chain kernel)
SHAPES = {1: (4, 4), 4: (4, 4), 6: (6, 6), 7: (7, 7), 10: (10, 5), 13: (7, 7), 20: (10, 7), 23: (8, 8)}


@pytest.fixture(scope="module")
def dev():
    from wgsassign_amd import device
    device.get_context()
    return device


@functools.lru_cache(maxsize=None)
def case(K, m=M):
    """(L, group_of, frequencies (m, K), the oracle's float32 sums): made once per K and shared; nobody writes to them."""
    from oracle import oracle as orc
    orc.build()
    rng = np.random.default_rng(900 + K)
    labels = rng.integers(0, K, size=N)
    labels[:K] = np.arange(K)                                  # no empty population
    L, IDs = synth.make_beagle_for_labels(M, labels, K, seed=7)
    L = np.ascontiguousarray(L[:m])
    pops = np.unique(IDs[:, 1])
    group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
    A = (0.02 + 0.96 * rng.random((m, K))).astype(np.float32)
    with np.errstate(all="ignore"):
        ll = orc.assignLL(L, A.copy(), 4)
    return L, group_of, A, ll


def on_device(dev, K, m=M):
    L, group_of, A, ll = case(K, m)
    return dev.DeviceBeagle.from_host(L, group_of, K), dev.AFSet.from_host(A), ll


def sums_and_plan(dev, b, afs, colptr=None, chains=False):
    from wgsassign_amd._lib import MODE_EXACT
    sc = dev.Score(b, afs, colptr)
    out = sc.sums(MODE_EXACT)
    if chains:
        sc.parts_exact(3)                                      # wgs_score_chains_prepare(P = 3) and the walk
    plan = sc.plan()
    sc.close()
    return out, plan


def direct_sums(dev, b, afs, monkeypatch):
    with monkeypatch.context() as mp:
        mp.setenv("WGSASSIGN_CODES", "0")
        out, plan = sums_and_plan(dev, b, afs)
    assert plan["path"] == 0
    return out


@pytest.mark.parametrize("K", sorted(SHAPES))
def test_direct_sweep_shapes(dev, K, monkeypatch):
    monkeypatch.setenv("WGSASSIGN_CODES", "0")
    b, afs, ll = on_device(dev, K)
    out, plan = sums_and_plan(dev, b, afs, chains=True)
    print(K, plan)
    kb, chain_kb = SHAPES[K]
    assert plan["path"] == 0
    assert (plan["kb"], plan["pairs"]) == (kb, 2 if kb <= 6 else 1)
    assert (plan["chain_kb"], plan["chain_pairs"]) == (chain_kb, 2 if chain_kb <= 4 else 1)
    assert same_nan(out.astype(np.float32), ll)
    afs.close()
    b.close()


@pytest.mark.parametrize("K,pairs", [(4, 2), (5, 1), (10, 1)])
def test_per_individual_columns(dev, K, pairs, monkeypatch):
    """Every individual points at the shared columns: the per-site values are the shared-column sweep's and a block's float64
    partial sums are exact, so the float64 sums are the same bits."""
    monkeypatch.setenv("WGSASSIGN_CODES", "0")
    b, afs, ll = on_device(dev, K)
    shared, _ = sums_and_plan(dev, b, afs)
    colptr = np.empty((N, K), dtype=np.uint64)
    colptr[:] = [afs.col_dev(k) for k in range(K)]
    out, plan = sums_and_plan(dev, b, afs, colptr, chains=True)
    print(K, plan)
    assert plan["path"] == 0 and plan["pairs"] == pairs and plan["chain_pairs"] == 1
    assert same(out, shared) and same_nan(out.astype(np.float32), ll)
    afs.close()
    b.close()


def expected_elem_bytes(kb, batch):
    """float rows only in the 16-SNP table and only where they need at most one float of padding to 16 bytes"""
    return 4 if batch == 16 and kb in (4, 7, 8) else 8


@pytest.mark.parametrize("K", [4, 5, 6, 7, 8, 9, 10])
def test_coded_sweep_table(dev, K, monkeypatch):
    monkeypatch.setenv("WGSASSIGN_CODES", "1")
    monkeypatch.setenv("WGSASSIGN_CODES_TABLE", "64")          # (also codes matrices too small to be worth it)
    b, afs, ll = on_device(dev, K)
    out, plan = sums_and_plan(dev, b, afs)
    info = b.codes_info()
    print(K, plan, info["score_batch_snps"])
    assert plan["path"] == 1 and plan["kb"] == K
    assert info["available"] and plan["score_batch"] == info["score_batch_snps"] and plan["score_batch"] in (16, 8, 4)
    assert plan["elem_bytes"] == expected_elem_bytes(K, plan["score_batch"])
    assert 1 <= plan["parts"] <= 16
    assert same_nan(out.astype(np.float32), ll)
    assert same(out, direct_sums(dev, b, afs, monkeypatch))
    afs.close()
    b.close()


def test_one_block_is_split_sixteen_ways(dev, monkeypatch):
    """m <= 4096 and n <= 1024: one block and one group of quads, so every split fits in one round of workgroups and the cost is
    ceil(64 / parts) + 1 tiles, whose only minimum over the usable splits up to 16 is 16."""
    monkeypatch.setenv("WGSASSIGN_CODES", "1")
    monkeypatch.setenv("WGSASSIGN_CODES_TABLE", "64")
    b, afs, ll = on_device(dev, 4, 4096)
    out, plan = sums_and_plan(dev, b, afs)
    print(plan)
    assert plan["path"] == 1 and plan["parts"] == 16
    assert same_nan(out.astype(np.float32), ll)
    afs.close()
    b.close()


def test_forced_parts_and_table(dev, monkeypatch):
    """WGS_SCORE_CODED_PARTS and WGS_SCORE_CODED_TABLE are obeyed and reported, and change no bit of the float64 sums."""
    monkeypatch.setenv("WGSASSIGN_CODES", "1")
    monkeypatch.setenv("WGSASSIGN_CODES_TABLE", "64")
    K = 5
    b, afs, ll = on_device(dev, K)
    outs = []
    for parts in (1, 5, 16):
        monkeypatch.setenv("WGS_SCORE_CODED_PARTS", str(parts))
        out, plan = sums_and_plan(dev, b, afs)
        print(parts, plan)
        assert plan["path"] == 1 and plan["parts"] == parts
        outs.append(out)
    monkeypatch.delenv("WGS_SCORE_CODED_PARTS")
    for table, elem in (("f", 4), ("d", 8)):
        monkeypatch.setenv("WGS_SCORE_CODED_TABLE", table)
        out, plan = sums_and_plan(dev, b, afs)
        print(table, plan)
        assert plan["path"] == 1 and plan["kb"] == 5 and plan["score_batch"] == 16 and plan["elem_bytes"] == elem
        outs.append(out)
    monkeypatch.delenv("WGS_SCORE_CODED_TABLE")
    direct = direct_sums(dev, b, afs, monkeypatch)
    assert all(same(o, direct) for o in outs)
    assert same_nan(direct.astype(np.float32), ll)
    afs.close()
    b.close()


# The table's SNP count follows from the 99th percentile of the classes per SNP (codes.hip: wgs_beagle_codes_plan; ~67 here, and
# 16 x 67 rows exceed the table's 616), which the 400 individuals and the quality bins set, not m: the percentile is the same at
# 65, 130, 300 and 6000 SNPs.  So m is the smallest the sweep itself still has something to get wrong at: two tiles and a ragged
# third of 2 SNPs.
QUALITY_M = 130


def test_many_classes_take_a_smaller_table_of_float64(dev, oracle, monkeypatch):
    """The quality-dependent matrix of tests/test_gpu_codes.py::test_quality_dependent_likelihoods (400 individuals, 4 populations)
    has too many classes per SNP for 16 SNPs per table: 8 or 4, and those tables hold float64 whatever the register batch (4 here,
    which takes float rows in a 16-SNP table)."""
    monkeypatch.setenv("WGSASSIGN_CODES", "1")
    m, n, K = QUALITY_M, 400, 4
    L, IDs = synth.make_beagle_quality(m, n, K, seed=5, quals=synth.QUAL_BINS)
    pops = np.unique(IDs[:, 1])
    group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
    A = (0.02 + 0.96 * np.random.default_rng(6).random((m, K))).astype(np.float32)
    b = dev.DeviceBeagle.from_host(L, group_of, K)
    afs = dev.AFSet.from_host(A)
    out, plan = sums_and_plan(dev, b, afs)
    info = b.codes_info()
    print(plan, info["score_batch_snps"])
    assert plan["path"] == 1 and plan["kb"] == 4
    assert plan["score_batch"] == info["score_batch_snps"] and plan["score_batch"] in (8, 4)
    assert plan["elem_bytes"] == 8 and 1 <= plan["parts"] <= 16
    with np.errstate(all="ignore"):
        assert same_nan(out.astype(np.float32), oracle.assignLL(L, A.copy(), 4))
    afs.close()
    b.close()


def test_a_matrix_not_worth_coding_is_swept_directly(dev, oracle, monkeypatch):
    """Deep coverage -- as many classes per SNP as individuals (the matrix of test_matrices_not_worth_coding_take_the_direct_kernels):
    no codes, the float32 sweep, with the codes left switched on."""
    monkeypatch.delenv("WGSASSIGN_CODES", raising=False)
    m, n, K = 3000, 80, 2
    rng = np.random.default_rng(4)
    g = rng.dirichlet((0.7, 0.7, 0.7), size=(m, n))
    L = np.empty((m, 2 * n), dtype=np.float32)
    L[:, 0::2] = np.round(g[:, :, 0], 6)
    L[:, 1::2] = np.round(g[:, :, 1], 6)
    group_of = (np.arange(n) // (n // K)).astype(np.int32)
    A = (0.02 + 0.96 * rng.random((m, K))).astype(np.float32)
    b = dev.DeviceBeagle.from_host(L, group_of, K)
    afs = dev.AFSet.from_host(A)
    out, plan = sums_and_plan(dev, b, afs)
    print(plan)
    assert not b.codes_info()["available"]
    assert plan["path"] == 0 and (plan["kb"], plan["pairs"]) == (4, 2)
    assert same_nan(out.astype(np.float32), oracle.assignLL(L, A.copy(), 4))
    afs.close()
    b.close()
