"""The class encoder (csrc/codes_kernels.hip: class_encode_kernel) held to its contract on the enumerated key sets of
tests/codes_cases.py: what it WRITES -- codes, dictionaries, ncls, the slabs' own numbering, tile_rows -- is read back
(wgs_debug_codes_download) and compared bit for bit with the matrix, for every geometry of its hash tables; then the sweeps that
consume the codes are compared with the direct kernels and the oracle on the same matrices.  No tolerance appears anywhere: the
statistics are quotients of integers and are compared with the same quotient."""
import numpy as np
import pytest

import codes_cases as cc
from test_codes_cases_cpu import MATRIX_NAMES
from test_gpu_codes import codes, quiet
from test_gpu_parity import same, same_nan

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dev():
    from wgsassign_amd import device
    device.get_context()
    return device


def matrix(T, name):
    return cc.build(T)[MATRIX_NAMES.index(name)]


def force(monkeypatch, T, rows):
    monkeypatch.setenv("WGSASSIGN_CODES_TABLE", str(T))
    monkeypatch.setenv("WGSASSIGN_EM_TABLE_ROWS", str(rows))
    monkeypatch.setenv("WGSASSIGN_EM_CODES_SWEEPS", "0")
    monkeypatch.setenv("WGSASSIGN_EM_CODES_MIN", "1")


def key64(a):
    """(..., 2) uint32 (g0, g1) -> one uint64"""
    return a[..., 0].astype(np.uint64) | (a[..., 1].astype(np.uint64) << np.uint64(32))


def distinct_per_row(a):
    s = np.sort(a, axis=1)
    return 1 + (s[:, 1:] != s[:, :-1]).sum(axis=1)


def test_download_refuses_a_matrix_without_codes(dev):
    M = matrix(64, "edges_1")
    b = dev.DeviceBeagle.from_host(M.L, M.labels, len(M.G.slab_sizes))
    with pytest.raises(ValueError, match="no class codes"):
        b.codes_download()
    with codes(False):
        assert not b.codes_info()["available"]
        with pytest.raises(ValueError, match="no class codes"):
            b.codes_download()
    b.close()


@pytest.mark.parametrize("name", MATRIX_NAMES)
@pytest.mark.parametrize("T,rows", [(64, 8), (64, 24), (128, 8), (128, 24), (256, 8), (256, 24)])
def test_what_the_encoder_writes(dev, T, rows, name, monkeypatch):
    """Round trip of codes and dictionary, class counts, the slabs' own numbering, tile_rows, the verdicts and the statistics."""
    force(monkeypatch, T, rows)
    M, G = matrix(T, name), cc.Geometry(T)
    b = dev.DeviceBeagle.from_host(M.L, M.labels, len(G.slab_sizes))
    assert np.array_equal(b.download_rows(0, M.m).view(np.uint32), M.L.view(np.uint32))            # the upload keeps every bit: signed zeros, NaN payloads
    with codes(True):
        info = b.codes_info()
        assert info["available"]
        d = b.codes_download()
    b.close()
    check_download(M, G, rows, d, info)


def check_download(M, G, rows, d, info):
    T, name, m, n = G.T, M.name, M.m, M.n
    bitsL = M.L.view(np.uint32)
    want = np.stack([bitsL[:, 0::2], bitsL[:, 1::2]], axis=2)                       # (m, n, 2)
    # ---- geometry
    assert d["hash_slots"] == info["hash_slots"] == T and d["em_table_rows"] == info["em_table_rows"] == rows and d["slab_numbering"]
    assert d["batch_rows_cap"] == cc.BATCH_ROWS_CAP and d["tile_rows_bytes"] * (cc.ENC_SLOTS // 256) == 64
    drows = d["dict_rows"]
    if name == "groups":
        assert d["score_batch_snps"] == G.score_batch and drows >= M.counts.max()
    else:
        assert drows == G.drows        # so the rows of drows and drows + 1 classes are among the cases, and `rich` means what the cases say
        assert {"count_%d" % drows, "count_%d" % (drows + 1)} <= {case for other in cc.build(T) for case in other.names}
    ncls = d["ncls"].astype(np.int64)
    coded = ncls > 0
    # ---- verdicts
    went_rich = {}
    for case in sorted(set(M.names[M.expect == "either"])):
        at = (M.names == case) & (M.expect == "either")
        went_rich[case] = (int((~coded[at]).sum()), int(at.sum()))
    print("either rows the encoder declared rich, T=%d lrows=%d %s: %s" % (T, rows, name, went_rich))
    bad = np.flatnonzero(((M.expect == "coded") & ~coded) | ((M.expect == "rich") & coded))
    assert not len(bad), [(int(i), str(M.names[i]), str(M.expect[i]), int(ncls[i])) for i in bad[:20]]
    chain = np.array([f.get("chain", 0) for f in M.facts])
    assert not coded[chain == 40].any() and coded[(chain > 0) & (chain <= cc.ENC_RMAX)].all() and coded[M.names == "plain"].all()
    # ---- round trip: dict[snp][codes[snp][i]] is individual i's (g0, g1); ncls = distinct bit patterns; the dictionary's rows are distinct
    code = np.concatenate([s["codes"] for s in d["slabs"]], axis=1).astype(np.int64)
    assert code.shape == (m, n)
    snp = np.arange(m)[:, None]
    got = d["dict"][snp, np.minimum(code, drows - 1)]
    ok = (code < ncls[:, None]) & (got == want).all(axis=2)
    bad = np.flatnonzero(coded & ~ok.all(axis=1))
    assert not len(bad), [(int(i), str(M.names[i]), int(ncls[i])) for i in bad[:20]]
    bad = np.flatnonzero(coded & (ncls != M.counts))
    assert not len(bad), [(int(i), str(M.names[i]), int(ncls[i]), int(M.counts[i])) for i in bad[:20]]
    dk = key64(d["dict"])
    for i in np.flatnonzero(coded):
        assert len(np.unique(dk[i, :ncls[i]])) == ncls[i], (i, M.names[i])
    # ---- the slabs' own numbering
    tiles = (m + 63) // 64
    rich_tile = np.concatenate([~coded, np.zeros(tiles * 64 - m, dtype=bool)]).reshape(tiles, 64).any(axis=1)
    n_direct = 0
    for g, size in enumerate(G.slab_sizes):
        s = d["slabs"][g]
        if size == 0:
            continue
        a, e = cc.slab_range(G, g)
        loc = np.concatenate([M.slab_counts[:, g], np.ones(tiles * 64 - m, dtype=np.int64)])     # (SNPs beyond the last: zeros, one class)
        tr = s["tile_rows"].astype(np.int64)
        per_byte = loc.reshape(tiles, d["tile_rows_bytes"], -1).max(axis=2)
        expect_tile = np.where(rich_tile, 255, loc.reshape(tiles, 64).max(axis=1))
        assert (tr >= np.where(rich_tile[:, None], 0, per_byte)).all(), (g, "tile_rows below the classes of its SNPs")
        bad = np.flatnonzero(tr.max(axis=1) != expect_tile)
        assert not len(bad), (g, [(int(t), int(tr[t].max()), int(expect_tile[t])) for t in bad[:10]])
        direct = tr.max(axis=1) > rows
        n_direct += int(direct.sum())
        keep = np.flatnonzero(~np.repeat(direct, 64)[:m])
        lc = s["lcodes"].astype(np.int64)[keep]
        lgot = s["ldict"][keep[:, None], np.minimum(lc, rows - 1)]
        lok = (lc < loc[keep, None]) & (lgot == want[keep, a:e]).all(axis=2)
        assert lok.all(), (g, [(int(keep[i]), str(M.names[keep[i]])) for i in np.flatnonzero(~lok.all(axis=1))[:10]])
        assert np.array_equal(distinct_per_row(lc), loc[keep]), g
    slabs_used = sum(1 for size in G.slab_sizes if size)
    assert 0 < n_direct < slabs_used * tiles                       # both sides of lrows are there
    # ---- the statistics agree with what was read back
    assert round(info["rich_snp_share"] * m) == int((~coded).sum()) and info["rich_snp_share"] == int((~coded).sum()) / m
    assert info["max_classes"] == ncls.max() and info["mean_classes"] == int(ncls.sum()) / int(coded.sum())
    assert info["em_direct_tile_share"] == n_direct / (slabs_used * tiles)
    # ---- the test is not blind: the chains cost the probe rounds their construction implies (c keys with one home slot in one
    # buffer: c - 1 rounds beyond the first, counted once per wavefront and buffer, given up after ENC_RMAX)
    if name.startswith("chains"):
        buffers = tiles * (64 // G.snps) * sum(-(-((size + 3) // 4) // (G.cols * cc.ENC_UQ)) for size in G.slab_sizes if size)
        implied = np.array([min(min(f["chain"], G.buffer) - 1, cc.ENC_RMAX) if f.get("spread") == "buffer" else 0 for f in M.facts])
        implied = np.concatenate([implied, np.zeros(tiles * 64 - m, dtype=np.int64)]).reshape(-1, G.snps).max(axis=1).sum()
        # (the statistic is rounds / buffers in a double: its product with the buffers, rounded, is the whole number of rounds again)
        assert implied > 0 and round(info["probe_rounds_per_buffer"] * buffers) >= implied, (info["probe_rounds_per_buffer"] * buffers, implied)


@pytest.mark.parametrize("T", cc.GEOMETRIES)
def test_classes_are_numbered_in_order_of_appearance(dev, T, monkeypatch):
    """The order of the classes is asserted where it is well defined: in cc.order_matrix every slab is one quad, so all of a SNP's
    individuals fall in one lane's walk.  codes = the first-appearance rank of each individual's bit pattern, the dictionary's rows
    stand in that order, and a slab's own code is the rank of the class among those the slab holds."""
    force(monkeypatch, T, 8)
    M = cc.order_matrix(T)
    G, m = M.G, M.m
    b = dev.DeviceBeagle.from_host(M.L, M.labels, len(G.slab_sizes))
    with codes(True):
        assert b.codes_info()["available"]
        d = b.codes_download()
    b.close()
    assert d["hash_slots"] == T and d["em_table_rows"] == 8 and d["slab_numbering"] and d["dict_rows"] >= M.counts.max()
    assert np.array_equal(d["ncls"], M.counts)
    code = np.concatenate([s["codes"] for s in d["slabs"]], axis=1).astype(np.int64)
    bad = np.flatnonzero((code != M.rank).any(axis=1))
    assert not len(bad), [(int(i), str(M.names[i]), code[i].tolist(), M.rank[i].tolist()) for i in bad[:5]]
    bitsL = M.L.view(np.uint32)
    want = np.stack([bitsL[:, 0::2], bitsL[:, 1::2]], axis=2)
    assert np.array_equal(d["dict"][np.arange(m)[:, None], M.rank], want)          # row k: the k-th pattern to appear
    for g, size in enumerate(G.slab_sizes):
        if size == 0:
            continue
        a, e = cc.slab_range(G, g)
        s = d["slabs"][g]
        local = np.array([np.searchsorted(np.unique(r), r) for r in M.rank[:, a:e]])
        assert np.array_equal(s["lcodes"], local), g
        assert np.array_equal(s["ldict"][np.arange(m)[:, None], local], want[:, a:e]), g
        loc = np.concatenate([M.slab_counts[:, g], np.ones(-m % 64, dtype=np.int64)])
        assert np.array_equal(s["tile_rows"].max(axis=1), loc.reshape(-1, 64).max(axis=1)), g


@pytest.mark.parametrize("T", cc.GEOMETRIES)
def test_the_longest_chains_that_must_be_coded(dev, T, monkeypatch):
    """cc.sparse_chain_matrix: chains of ENC_RMAX keys and chains that wrap past the last slot, in so few SNPs that the matrix is coded
    whatever the sample pass makes of them -- an encoder that gives up too early fails HERE, on their verdicts, not by declining the
    matrix.  Every SNP is coded with its number of classes, and codes and dictionary round-trip."""
    force(monkeypatch, T, 24)
    M = cc.sparse_chain_matrix(T)
    b = dev.DeviceBeagle.from_host(M.L, M.labels, len(M.G.slab_sizes))
    with codes(True):
        info = b.codes_info()
        assert info["available"]
        d = b.codes_download()
    b.close()
    assert d["hash_slots"] == T and d["dict_rows"] >= cc.ENC_RMAX
    bad = np.flatnonzero(d["ncls"] != M.counts)
    assert not len(bad), [(int(i), str(M.names[i]), int(d["ncls"][i]), int(M.counts[i])) for i in bad]
    assert info["rich_snp_share"] == 0 and info["max_classes"] == cc.ENC_RMAX
    code = np.concatenate([s["codes"] for s in d["slabs"]], axis=1).astype(np.int64)
    bitsL = M.L.view(np.uint32)
    want = np.stack([bitsL[:, 0::2], bitsL[:, 1::2]], axis=2)
    assert (code < M.counts[:, None]).all() and np.array_equal(d["dict"][np.arange(M.m)[:, None], code], want)


def fit_and_score(dev, b, groups, counts, mode=None):
    K = len(groups)
    em = dev.EMBatch(b, np.asarray(groups, dtype=np.int32))
    iters = em.run(200, 1e-4)
    paths = em.sweep_paths()
    cols = []
    afs = dev.AFSet(b.m, K, ctx=b.ctx)
    for k in range(K):
        em.clamp(k, int(counts[k]))
        cols.append(em.get_f(k))
        afs.set_column_from_em(k, em, k)
    out, _ = dev.assign(b, afs, mode=mode)
    em.close()
    afs.close()
    return [int(x) for x in iters], np.stack(cols, axis=1), out, paths


@pytest.mark.parametrize("name", MATRIX_NAMES)
@pytest.mark.parametrize("T", cc.GEOMETRIES)
def test_the_sweeps_that_read_the_codes(dev, oracle, T, name, monkeypatch):
    """The EM fit of every population to convergence and the n x K sums, through the codes and directly, exact and fast: identical
    iterations, frequencies and sums, and the oracle's in the exact mode.  16 table rows: the limit cases fall on both sides, and
    both the table path and the direct-tile path of the coded EM sweep run."""
    from wgsassign_amd._lib import MODE_FAST
    force(monkeypatch, T, 16)
    M, G = matrix(T, name), cc.Geometry(T)
    groups = [g for g, size in enumerate(G.slab_sizes) if size]
    counts = [G.slab_sizes[g] for g in groups]
    eq = same_nan if np.isnan(M.L).any() else same
    b = dev.DeviceBeagle.from_host(M.L, M.labels, len(G.slab_sizes))
    with codes(False):
        it0, af0, out0, paths0 = fit_and_score(dev, b, groups, counts)
        _, _, fast0, _ = fit_and_score(dev, b, groups, counts, mode=MODE_FAST)
        assert b.codes_state() == 0 and paths0[2] == 0 and paths0[3] == 0
    with codes(True):
        info = b.codes_info()
        assert info["available"] and info["em_table_rows"] == 16 and 0 < info["em_direct_tile_share"] < 1
        it1, af1, out1, paths1 = fit_and_score(dev, b, groups, counts)
        _, _, fast1, _ = fit_and_score(dev, b, groups, counts, mode=MODE_FAST)
        assert paths1[2] > 0                                       # through em_coded_kernel: its table path and its direct tiles
    b.close()
    assert it1 == it0 and eq(af1, af0) and same_nan(out1, out0) and same_nan(fast1, fast0)
    IDs = np.array([["Ind%d" % i, "pop%02d" % g] for i, g in enumerate(M.labels)], dtype=str)
    L = np.array(M.L)
    with quiet():
        _, af_o, _, it_o = oracle.fit_reference_af(L, IDs, t=4)
    assert it1 == [int(x) for x in it_o] and eq(af1, af_o)
    with np.errstate(all="ignore"):
        assert same_nan(out1.astype(np.float32), oracle.assignLL(L, af_o.copy(), 4))


@pytest.mark.parametrize("name", MATRIX_NAMES)
@pytest.mark.parametrize("T", cc.GEOMETRIES)
def test_leave_one_out_refits_of_one_population(dev, oracle, T, name, monkeypatch):
    """The re-fits of the population one above a buffer, each without one of its individuals, through em_coded_group_kernel
    (WGSASSIGN_LOO_CODES=1) and through the float32 group kernel (0): identical; the first and the last re-fit are the oracle's."""
    force(monkeypatch, T, 16)
    M, G = matrix(T, name), cc.Geometry(T)
    pop = 5
    a, e = cc.slab_range(G, pop)
    skips = np.arange(a, e, dtype=np.int32)
    eq = same_nan if np.isnan(M.L).any() else same
    res = {}
    for on in ("0", "1"):
        monkeypatch.setenv("WGSASSIGN_LOO_CODES", on)
        b = dev.DeviceBeagle.from_host(M.L, M.labels, len(G.slab_sizes))
        em = dev.EMBatch(b, np.full(len(skips), pop, dtype=np.int32), skips=skips)
        its = [int(x) for x in em.run(200, 1e-4)]
        paths = em.sweep_paths()
        res[on] = (its, np.stack([em.get_f(k) for k in range(len(skips))], axis=1))
        # (the last fit left of a batch has its slab to itself and is planned like a population's own fit, whatever WGSASSIGN_LOO_CODES says)
        assert (paths[3] > 0 and b.codes_state() == 1) if on == "1" else (paths[1] > 0 and paths[3] == 0)
        if on == "1":
            assert 0 < b.codes_info()["em_direct_tile_share"] < 1
        em.close()
        b.close()
    assert res["1"][0] == res["0"][0] and eq(res["1"][1], res["0"][1])
    L = np.array(M.L)
    for j in (0, len(skips) - 1):
        f, it = oracle.emMAF(oracle.gather(L, np.delete(skips, j), t=4), 200, 1e-4, t=4)
        assert res["1"][0][j] == int(it) and eq(res["1"][1][:, j], f)
