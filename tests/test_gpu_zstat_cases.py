"""GPU: the per-site z-score statistic (csrc/zscore_kernels.hip: zstat_kernel, zs_loops out of the LDS table and out of the deep rows,
zs_logf) and the deep branch of the mask sweep on the enumerated terms of tests/zstat_cases.py, which tests/test_zstat_cases_cpu.py
holds to their claims and, through the restatement (tests/zscore_cpu.py), to the record of the real reference
(tests/golden/zstat_cases.npz).  Every comparison is an equality of bits over every kept site, NaN exactly where the restatement
has NaN (sign and payload of a NaN are not compared); nothing is left out and nothing has a tolerance."""
import ctypes
import os

import numpy as np
import pytest

import zscore_cpu
import zstat_cases as zs
from conftest import GOLDEN
from test_gpu_zscore import device_run
from test_zscore_cpu import same

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = -7
_want = {}


def restatement():
    """(W_l_obs, W_l, var_W_l) (n, 321) of the whole grid: computed once, shared, read-only."""
    if "grid" not in _want:
        g = zs.shared_grid()
        out = tuple(a.reshape(len(g["variant"]), -1) for a in zs.restatement(g))
        for a in out:
            a.setflags(write=False)
        _want["grid"] = out
    return _want["grid"]


@pytest.fixture(scope="module")
def device_grid():
    """The grid on the device: matrix in zs.N_SLABS population slabs, depth table, one frequency column per individual."""
    from wgsassign_amd import zscore
    from wgsassign_amd.device import AFSet, DeviceBeagle
    g = zs.shared_grid()
    b = DeviceBeagle.from_host(g["L"].copy(), g["group_of"].copy(), zs.N_SLABS)
    depth = zscore.DepthTable(b, g["AD"].copy(), chunk_rows=1000)
    afs = AFSet.from_host(g["A"].copy())
    yield g, depth, afs
    afs.close()
    depth.close()
    b.close()


def batches(n, size):
    return [(i0, min(size, n - i0)) for i0 in range(0, n, size)]


# ---------------------------------------------------------------- a. the statistic
@pytest.mark.parametrize("size, deep", [(None, True), (3, True), (2, True), (3, False)],
                         ids=["one batch", "batches of 3", "batches of 2", "dense, batches of 3"])
def test_statistic_on_every_term(device_grid, size, deep):
    """wgs_zkeep_create_deep (deep=False: plain wgs_zkeep_create, the DEEP = false instantiation, which drops the deep depths' sites)
    and wgs_zscore_stats on the whole grid: kept and the site lists are exactly the term sites; W_l_obs, W_l and var_W_l of every kept
    site of every individual are the restatement's bits; the element behind each output is untouched.  Batches of 3 and 2: obase is
    not zero, and batch boundaries fall between the table variants."""
    from wgsassign_amd import _lib, zscore
    from wgsassign_amd._lib import check, f32p, i32p
    g, depth, afs = device_grid
    lib = _lib.load()
    n = len(g["variant"])
    want = restatement()
    dense = np.array(zs.DEPTHS)[g["t_depth"]] <= zs.MAX_DENSE
    bad, compared = [], 0
    for i0, count in batches(n, size or n):
        keep = zscore.KeepSet(depth, i0, *(np.ascontiguousarray(t) for t in zs.batch_tables(g, i0, count, deep)))
        try:
            slots = [np.flatnonzero(dense[i0 + j]) if not deep else np.arange(len(g["sites"])) for j in range(count)]
            assert list(keep.kept) == [len(s) for s in slots], ("kept", i0, count, list(keep.kept))
            for j in range(count):
                out = np.full(len(slots[j]) + 1, GUARD, dtype=np.int32)
                check(lib.wgs_zkeep_sites(keep.handle, j, i32p(out)))
                assert out[-1] == GUARD
                same(out[:-1], g["sites"][slots[j]].astype(np.int32), "the kept sites of individual %d are the term sites" % (i0 + j))
            total = int(keep.kept.sum())
            got = [np.full(total + 1, GUARD, dtype=F32) for _ in range(3)]
            ptrs = (ctypes.c_void_p * count)(*[int(afs.col_dev(i0 + j)) for j in range(count)])
            tabs = np.ascontiguousarray(g["tabs"][i0:i0 + count])
            check(lib.wgs_zscore_stats(keep.handle, f32p(tabs), ptrs, f32p(got[0]), f32p(got[1]), f32p(got[2])))
            assert all(x[-1] == GUARD for x in got), "the element behind an output was written"
            ind = np.concatenate([np.full(len(s), i0 + j) for j, s in enumerate(slots)])
            flat = np.concatenate(slots)
            for name, x, w in zip(("W_l_obs", "W_l", "var_W_l"), got, want):
                expect = w[ind, flat]
                compared += len(expect)
                for k in zs.differences(x[:-1], expect):
                    bad.append("%s of %s: device %r (0x%08x), expected %r (0x%08x)" % (name, zs.describe(g, ind[k], flat[k]), x[k], zs.bits(x[k:k + 1])[0],
                                                                                      expect[k], zs.bits(expect[k:k + 1])[0]))
        finally:
            keep.close()
    assert compared == 3 * (n * len(g["sites"]) if deep else int(dense.sum()))
    assert not bad, "%d of %d values differ:\n%s" % (len(bad), compared, "\n".join(bad[:8]))


# ---------------------------------------------------------------- b. the deep mask at its edge
def kept_sites(L, AD, key_mean, key_comp, deep_map, deep_rows, launches):
    """[(first individual, slot, kept, sites)] of KeepSets over the individuals `launches` = [(i0, count)]."""
    from wgsassign_amd import zscore
    from wgsassign_amd.device import DeviceBeagle
    b = DeviceBeagle.from_host(L)
    depth = zscore.DepthTable(b, AD)
    out = []
    try:
        for i0, count in launches:
            rows = slice(i0, i0 + count)
            keep = zscore.KeepSet(depth, i0, key_mean[rows], key_comp[rows], deep_map[rows], deep_rows)
            for slot in range(count):
                out.append((i0, slot, int(keep.kept[slot]), keep.sites(slot)))
            keep.close()
    finally:
        depth.close()
        b.close()
    return out


def test_deep_mask_at_its_edge():
    """threshold_sites' groups of seven under classes of a deep depth -- means and components in the deep rows -- and a deep depth
    without rows: the kept sites are NumPy's ~(abs(mean - v) > float32(0.01)), ascending."""
    t = zs.deep_threshold_sites()
    for i0, slot, kept, got in kept_sites(t["L"], t["AD"], t["key_mean"], t["key_comp"], t["deep_map"], t["deep_rows"], [(0, 2), (1, 1)]):
        i = i0 + slot
        want = np.flatnonzero(zs.expected_keep(t["L"], t["AD"], i, t["key_mean"][i], t["key_comp"][i], t["deep_map"][i], t["deep_rows"])).astype(np.int32)
        assert np.array_equal(want, np.flatnonzero(t["expect"][:, i]))
        assert kept == len(want) == 24 * 4 + 7
        missing, extra = np.setdiff1d(want, got), np.setdiff1d(got, want)
        assert not len(missing) and not len(extra), ("individual %d" % i, "not kept", missing, "kept", extra)
        same(got, want, "sites in ascending order")
        assert not np.isin(t["dropped_sites"], got).any()


def test_special_values_at_the_mask():
    """NaN, +/-inf, -0.0 and subnormals at the tested component, under finite, infinite and zero means, dense and deep."""
    s = zs.special_mask_values()
    want = np.flatnonzero(zs.expected_keep(s["L"], s["AD"], 0, s["key_mean"][0], s["key_comp"][0], s["deep_map"][0], s["deep_rows"])).astype(np.int32)
    (_, _, kept, got), = kept_sites(s["L"], s["AD"], s["key_mean"], s["key_comp"], s["deep_map"], s["deep_rows"], [(0, 1)])
    wrong = np.setxor1d(want, got)
    assert not len(wrong), [c for c in s["cells"] if c[0] in wrong]
    assert kept == len(want) == 48
    same(got, want, "sites in ascending order")


# ---------------------------------------------------------------- c. the pipeline on frequencies of exactly 0 and 1
def same_values(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype.kind == "f":
        assert got.dtype == want.dtype and zs.same_nan(got, want), what
    else:
        same(got, want, what)


@pytest.mark.parametrize("batch, site0", [(3, 0), (2, 12345)])
def test_pipeline_on_boundary_frequencies(batch, site0):
    """zstat_cases.boundary_frequencies through the assignment flavour: every `details` array, the sums and z against the restatement
    and against the record of the real reference; the printed lines and the file text."""
    gold = np.load(os.path.join(GOLDEN, "zstat_cases.npz"), allow_pickle=False)
    if "pipeline" not in _want:
        L, AD, IDs, A = zs.boundary_frequencies()
        with np.errstate(all="ignore"):
            _want["pipeline"] = (L, AD, IDs, A, zscore_cpu.assignment(L, AD, IDs, np.unique(IDs[:, 1]), A))
    L, AD, IDs, A, want = _want["pipeline"]
    with np.errstate(all="ignore"):
        z, details, lines = device_run(L, AD, IDs, A, "assignment", 0, False, None, None, batch, site0)
    assert len(details) == len(want) == 4
    for i, (d, w) in enumerate(zip(details, want)):
        tag = "individual %d " % i
        for k in ("keys", "counts", "means", "AD_array", "keep", "fac", "like", "index", "A", "wobs", "wl", "var"):
            same_values(d[k], w[k], tag + k)
        sums = np.array([d[k] for k in ("W_l_obs", "z_mu", "z_var", "z")], dtype=F32)
        same_values(sums, np.array([w[k] for k in ("W_l_obs", "z_mu", "z_var", "z")], dtype=F32), tag + "sums and z")
        for k in ("wobs", "wl", "var"):
            same_values(d[k], gold["pipeline_i%d_%s" % (i, k)], tag + k + " against the record")
        same_values(sums, gold["pipeline_i%d_sums" % i], tag + "sums and z against the record")
    assert lines == [ln for i, w in enumerate(want) for ln in zscore_cpu.stdout_lines(i, w)]
    assert lines == str(gold["pipeline_stdout"]).splitlines()[:-1]
    assert zscore_cpu.file_text(z[:, 0]) == zscore_cpu.file_text([w["z"] for w in want]) == str(gold["pipeline_file"])
