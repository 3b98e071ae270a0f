"""CPU-only: sites deeper than 21 reads.  tests/zscore_cpu.py, unmodified, reproduces bit for bit what the real reference returned
on such data (tests/golden/zscore_deep.npz, made by tests/golden/make_golden_zscore_deep.py) in both regimes -- deep depths that
are incomplete and dropped, and the depths 22 and 23 kept with an index of (24, 24); the product's host side of the deep tier
(dictionary of the listed sites, merge of the two tiers, deep tables) is held to the same records -- the tables also by reading
them the way the mask and statistic kernels do, which must give the recorded L_keep, W_l and var_W_l."""
import ast
import os

import numpy as np
import pytest

import synth_deep
import synth_depth
import zscore_cpu
from conftest import GOLDEN
from test_zscore_cpu import compare_individual, runs, same


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "zscore_deep.npz"), allow_pickle=False)


_inputs = []


def deep_inputs(gold):
    if not _inputs:
        L, AD, IDs, A, deep = synth_deep.make_deep(**ast.literal_eval(str(gold["case_deep_gen"])))
        assert synth_depth.digest(L, AD, A) == str(gold["case_deep_digest"]), "the generator no longer reproduces the recorded inputs"
        _inputs.append((L, AD, IDs, A, deep))
    return _inputs[0]


def test_restatement_reproduces_every_recorded_array(gold, oracle):
    L, AD, IDs, A, _ = deep_inputs(gold)
    pops = np.unique(IDs[:, 1])
    seen = 0
    for r, spec in runs(gold):
        if spec["flavour"] == "assignment":
            res = zscore_cpu.assignment(L, AD, IDs, pops, A, spec["thr"], spec["srt"], spec["ind_start"], spec["ind_end"])
        else:
            res = zscore_cpu.reference(L, AD, IDs, lambda Lp, it, tol: oracle.emMAF(Lp, it, tol, 2), 200, 1e-4, spec["thr"], spec["srt"],
                                       spec["ind_start"], spec["ind_end"])
        lo = spec["ind_start"] or 0
        lines = []
        for j, one in enumerate(res):
            compare_individual(gold, r, lo + j, one, one["extra"] if spec["flavour"] == "reference" else None)
            lines += zscore_cpu.stdout_lines(lo + j, one)
            seen += 1
        assert lines == str(gold["run%d_stdout" % r]).splitlines()[:-1], "stdout lines of run %d" % r
        assert zscore_cpu.file_text([one["z"] for one in res]) == str(gold["run%d_file" % r])
    assert seen == 11


def test_recorded_case_covers_both_regimes(gold):
    """Individuals 1, 3, 4 have deep classes in the dictionary and none in AD_array (dropped); individual 2 keeps the depths 22 and 23
    whole, its index is (24, 24), and most of its deep sites are in L_keep."""
    L, AD, IDs, A, deep = deep_inputs(gold)
    for r in (0, 1):
        for i in (1, 3, 4):
            keys = gold["run%d_i%d_keys" % (r, i)]
            assert (keys.sum(axis=1) > 21).sum() >= 3 and gold["run%d_i%d_AD_array" % (r, i)][:, 2].max() <= 21
            assert not np.isin(deep[i], gold["run%d_i%d_keep" % (r, i)]).any()
        assert (255, 255) in {tuple(k) for k in gold["run%d_i3_keys" % r]}
        arr = gold["run%d_i2_AD_array" % r]
        assert {22, 23} <= set(arr[:, 2]) and (arr[:, 2] == 22).sum() == 23 and (arr[:, 2] == 23).sum() == 24
        assert gold["run%d_i2_index" % r].shape == (24, 24)
        kept = np.isin(deep[2], gold["run%d_i2_keep" % r]).sum()
        assert len(deep[2]) // 2 <= kept < len(deep[2])
        assert (gold["run%d_i0_keys" % r].sum(axis=1) <= 21).all()


def listed(L, AD, i):
    """What wgs_zscore_deep_sites returns for individual i, and the dense tier as wgs_zscore_classes returns it."""
    from wgsassign_amd import zscore
    dl = AD[:, 2 * i] + AD[:, 2 * i + 1]
    at = np.flatnonzero(dl > zscore.MAX_DENSE)
    deep = (at.astype(np.int32), np.ascontiguousarray(AD[at][:, 2 * i:2 * i + 2]), np.ascontiguousarray(L[at][:, 2 * i:2 * i + 2]))
    shallow = dl <= zscore.MAX_DENSE
    site = np.flatnonzero(shallow)
    keys, counts, _, sums = zscore_cpu.depth_classes(L[shallow], AD[shallow], i)
    first = np.array([site[np.flatnonzero((AD[shallow, 2 * i] == a) & (AD[shallow, 2 * i + 1] == b))[0]] for a, b in keys], dtype=np.int32)
    return (keys, counts, first, sums), deep


def test_host_dictionary_and_deep_tables(gold):
    """zscore.deep_classes / merge_tiers / key_filter / get_factorials / deep_tables against the records."""
    from wgsassign_amd import zscore
    L, AD, IDs, A, _ = deep_inputs(gold)
    summaries = []
    for i in range(6):
        g = lambda k: gold["run0_i%d_%s" % (i, k)]
        dense, deep = listed(L, AD, i)
        empty = (np.empty((0, 2), dtype=np.int64), np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int32), np.empty((0, 3), dtype=np.float32))
        keys, counts, means = zscore.merge_tiers(dense, zscore.deep_classes(*deep) if len(deep[0]) else empty)
        same(keys, g("keys"), "keys")
        same(counts, g("counts"), "counts")
        same(means, g("means"), "means")
        arr = zscore.key_filter(keys, counts, 0, False)
        same(arr, g("AD_array"), "AD_array")
        fac, like, index = zscore.get_factorials(arr, keys, means, 0.01)
        same(fac, g("fac"), "AD_factorial")
        same(like, g("like"), "AD_like")
        same(index, g("index"), "AD_index")
        summaries.append(dict(keys=keys, counts=counts, means=means, AD_array=arr))
    dmap, rows = zscore.deep_tables(summaries)
    assert dmap.shape == (6, 511) and rows.shape == (23 + 24, 8) and rows.dtype == np.float32
    assert sorted(np.flatnonzero(dmap[2] >= 0)) == [22, 23] and (np.delete(dmap, 2, axis=0) == -1).all()
    g = lambda k: gold["run0_i2_" + k]
    where = {tuple(k): r for r, k in enumerate(g("keys"))}
    for d in (22, 23):
        for a in range(d + 1):
            row = rows[dmap[2, d] + a]
            mean = g("means")[where[(d - a, a)]]
            assert row[0] == np.argmax(mean) and row[1] == mean.max()
            r = g("index")[a, d - a]
            same(row[2:5], g("like")[r], "AD_like at the transposed index")
            same(row[5:8], g("fac")[r], "AD_factorial at the transposed index")
    assert zscore.deep_tables(summaries[:2]) == (None, None)
    tabs, _ = zscore.stat_tables(summaries)
    assert tabs.shape == (6, 253, 6)


def test_tables_read_as_the_kernels_read_them(gold):
    """NumPy in the place of zmask_kernel / zstat_kernel over the product's own tables (mask_tables, stat_tables, deep_tables): a
    dense class through its class index, a deep class through map[depth] + Aa; the loops' row a through the class index of
    (depth - a, a) or row map[depth] + a.  Pins the layout the kernels are written against to the reference's outputs."""
    from wgsassign_amd import zscore
    F32 = np.float32
    L, AD, IDs, A, deep = deep_inputs(gold)
    pops = np.unique(IDs[:, 1])
    summaries = [dict(keys=gold["run0_i%d_keys" % i], counts=gold["run0_i%d_counts" % i], means=gold["run0_i%d_means" % i],
                      AD_array=gold["run0_i%d_AD_array" % i]) for i in range(6)]
    key_mean, key_comp = zscore.mask_tables(summaries)
    tabs, _ = zscore.stat_tables(summaries)
    dmap, rows = zscore.deep_tables(summaries)
    for i in range(6):
        Ar, Aa = AD[:, 2 * i].astype(np.int64), AD[:, 2 * i + 1].astype(np.int64)
        dl = Ar + Aa
        T = np.stack(zscore_cpu.triple(L, i), axis=1)
        dense = dl <= 21
        k = np.where(dense, dl * (dl + 1) // 2 + Aa, 0)
        r = np.where(dense, -1, dmap[i, dl])
        at = np.where(r >= 0, r + Aa, 0)
        comp = np.where(dense, key_comp[i, k], np.where(r >= 0, rows[at, 0].astype(np.int64), -1))
        mean = np.where(dense, key_mean[i, k], rows[at, 1])
        v = T[np.arange(len(dl)), np.maximum(comp, 0)]
        keep = np.flatnonzero((comp >= 0) & ~(np.abs(mean - v) > F32(0.01))).astype(np.int32)
        same(keep, gold["run0_i%d_keep" % i], "L_keep of individual %d" % i)
        Af = gold["run0_i%d_A" % i]
        Ad = Af.astype(np.float64)
        P0, P1, P2 = ((1.0 - Ad) * (1.0 - Ad)).astype(F32), ((2.0 * (1.0 - Ad)) * Ad).astype(F32), Af * Af
        wl, var = np.zeros(len(keep), dtype=F32), np.zeros(len(keep), dtype=F32)
        for q, s in enumerate(keep):
            d = int(dl[s])
            tab = tabs[i, d * (d + 1) // 2:d * (d + 1) // 2 + d + 1] if d <= 21 else rows[dmap[i, d]:dmap[i, d] + d + 1, 2:]
            lg = zscore_cpu._logf((tab[:, 0] * P0[q] + tab[:, 1] * P1[q]) + tab[:, 2] * P2[q])
            w = F32(0)
            for a in range(d + 1):
                for c, P in enumerate((P0[q], P1[q], P2[q])):
                    w = w + (lg[a] * P) * tab[a, 3 + c]
            u = F32(0)
            for a in range(d + 1):
                dd = w - lg[a]
                for c, P in enumerate((P0[q], P1[q], P2[q])):
                    u = u + ((dd * dd) * P) * tab[a, 3 + c]
            wl[q], var[q] = w, u
        same(wl, gold["run0_i%d_wl" % i], "W_l of individual %d" % i)
        same(var, gold["run0_i%d_var" % i], "var_W_l of individual %d" % i)
