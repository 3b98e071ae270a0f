"""GPU: the z-score sweeps (csrc/zscore_kernels.hip) on the enumerated inputs of tests/zscore_cases.py, which
tests/test_zscore_cases_cpu.py holds to their claims -- every depth class up to 21 reads (the classes 64 .. 252 that three of the
class sweep's four wavefronts own, the statistic's loops at depths 8 .. 21 out of the LDS table), the last dense classes next to
the first deep ones, the 0.01 site filter exactly at its edge, the prefix scan's partitions of its 256 threads, and the sweep's
own copy of the table logarithm against the original.  Everything is compared with no tolerance: with the CPU restatement
(tests/zscore_cpu.py), with the record of the real reference at these depths (tests/golden/zscore_classes.npz), with NumPy."""
import ctypes
import os

import numpy as np
import pytest

import zscore_cases as zc
import zscore_cpu
from conftest import GOLDEN
from test_gpu_log import values as original_log_values
from test_gpu_zscore import device_run
from test_gpu_zscore_deep import compare
from test_zscore_cases_cpu import recorded_inputs
from test_zscore_cpu import compare_individual, runs, same

pytestmark = pytest.mark.gpu

F32 = np.float32
_inputs, _want = {}, {}


def case(name):
    if name not in _inputs:
        _inputs[name] = getattr(zc, name)()
    return _inputs[name]


def restatement(name, flavour, oracle):
    """Computed once per (case, flavour) and shared; never changed."""
    if (name, flavour) not in _want:
        L, AD, IDs, A = case(name)[:4]
        if flavour == "assignment":
            _want[name, flavour] = zscore_cpu.assignment(L, AD, IDs, np.unique(IDs[:, 1]), A)
        else:
            _want[name, flavour] = zscore_cpu.reference(L, AD, IDs, lambda Lp, it, tol: oracle.emMAF(Lp, it, tol, 8), 200, 1e-4)
    return _want[name, flavour]


# ---------------------------------------------------------------- a. the pipeline on every class
@pytest.mark.parametrize("flavour", ["assignment", "reference"])
@pytest.mark.parametrize("name", ["every_class", "incomplete_21"])
def test_pipeline_on_every_class(name, flavour, oracle):
    """Batches of 3 (the full individuals 1 and 2 share a launch with a shallow one), then batches of 2 (a batch boundary between
    them) with site0 = 12345: every `details` array, the sums, z, the subset fits' iterations, the printed lines and the file text."""
    L, AD, IDs, A = case(name)[:4]
    want = restatement(name, flavour, oracle)
    assert len(want) == 4 and 21 in want[2]["AD_array"][:, 2] and (21 in want[1]["AD_array"][:, 2]) == (name == "every_class")
    printed = [ln for i, w in enumerate(want) for ln in zscore_cpu.stdout_lines(i, w)]
    for batch, site0 in ((3, 0), (2, 12345)):
        z, details, lines = device_run(L, AD, IDs, A, flavour, 0, False, None, None, batch, site0)
        compare(details, want, flavour)
        assert lines == printed
        assert zscore_cpu.file_text(z[:, 0]) == zscore_cpu.file_text([w["z"] for w in want])


@pytest.mark.parametrize("batch", [3, 2])
def test_recorded_classes_case_against_the_reference_itself(batch):
    """The reduced case the real reference was run on: every recorded array, the stdout lines and the file text."""
    gold = np.load(os.path.join(GOLDEN, "zscore_classes.npz"), allow_pickle=False)
    L, AD, IDs, A = recorded_inputs(gold)
    seen = 0
    for r, spec in runs(gold):
        z, details, lines = device_run(L, AD, IDs, A, spec["flavour"], spec["thr"], spec["srt"], spec["ind_start"], spec["ind_end"], batch)
        for j, d in enumerate(details):
            compare_individual(gold, r, j, d, d.get("it"))
            seen += 1
        assert lines == str(gold["run%d_stdout" % r]).splitlines()[:-1]
        assert zscore_cpu.file_text(z[:, 0]) == str(gold["run%d_file" % r])
    assert seen == 8


# ---------------------------------------------------------------- b. the dictionary alone
def dense_dictionary(L, AD, i):
    """What wgs_zscore_classes must return for individual i: counts, first sites, float32 sums per class, and `over`."""
    dl = AD[:, 2 * i] + AD[:, 2 * i + 1]
    dense = np.flatnonzero(dl <= zc.MAX_DENSE)
    keys, counts, _, sums = zscore_cpu.depth_classes(L[dense], AD[dense], i)
    k_of_site = zc.class_index(AD[dense, 2 * i].astype(np.int64), AD[dense, 2 * i + 1].astype(np.int64))
    cnt = np.zeros(zc.N_CLASSES, dtype=np.int32)
    first = np.full(zc.N_CLASSES, -1, dtype=np.int32)
    s = np.zeros((zc.N_CLASSES, 3), dtype=F32)                     # +0.0 where a class has no site
    for (a, b), c, row in zip(keys, counts, sums):
        k = int(zc.class_index(a, b))
        cnt[k], s[k], first[k] = c, row, dense[np.flatnonzero(k_of_site == k)[0]]
    return cnt, first, s, int((dl > zc.MAX_DENSE).sum())


@pytest.mark.parametrize("name", ["every_class", "edge_of_dense"])
def test_dictionary_of_all_253_classes(name):
    from wgsassign_amd import _lib, zscore
    from wgsassign_amd._lib import check, f32p, i32p
    from wgsassign_amd.device import DeviceBeagle
    L, AD = case(name)[:2]
    want = [dense_dictionary(L, AD, i) for i in range(4)]
    if name == "edge_of_dense":
        claims = case(name)[4]
        assert want[zc.EDGE_IND][3] == claims["over"] and all(want[zc.EDGE_IND][0][k] == n for k, n in claims["counts"].items())
    else:
        assert all((want[i][0] >= 6).all() for i in zc.FULL) and (want[0][0] == 0).sum() > 190
    b = DeviceBeagle.from_host(L)
    depth = zscore.DepthTable(b, AD, chunk_rows=1000)
    lib = _lib.load()
    try:
        for i0, count in ((0, 4), (1, 2), (2, 1)):
            cnt = np.full((count + 1, zc.N_CLASSES), -7, dtype=np.int32)
            first = np.full((count + 1, zc.N_CLASSES), -7, dtype=np.int32)
            sums = np.full((count + 1, zc.N_CLASSES, 3), -7, dtype=F32)
            over = np.full(count + 1, -7, dtype=np.int32)
            check(lib.wgs_zscore_classes(depth.handle, i0, count, i32p(cnt), f32p(sums), i32p(first), i32p(over)))
            assert (cnt[-1] == -7).all() and (first[-1] == -7).all() and (sums[-1] == -7).all() and over[-1] == -7
            for j in range(count):
                tag = "%s, individual %d of [%d, %d): " % (name, i0 + j, i0, i0 + count)
                w_cnt, w_first, w_sums, w_over = want[i0 + j]
                same(cnt[j], w_cnt, tag + "counts")
                same(first[j], w_first, tag + "first sites")
                same(sums[j], w_sums, tag + "float32 sums")                     # bytes: an empty class holds +0.0, not -0.0
                assert over[j] == w_over, tag + "sites beyond the dense tier"
    finally:
        depth.close()
        b.close()


# ---------------------------------------------------------------- c. the site filter at its edge
def test_site_filter_at_its_edge():
    from wgsassign_amd import zscore
    from wgsassign_amd.device import DeviceBeagle
    t = zc.threshold_sites()
    b = DeviceBeagle.from_host(t["L"])
    depth = zscore.DepthTable(b, t["AD"])
    try:
        for i0, rows in ((0, slice(0, 2)), (1, slice(1, 2))):
            keep = zscore.KeepSet(depth, i0, t["key_mean"][rows], t["key_comp"][rows])
            for slot in range(keep.count):
                want = np.flatnonzero(t["expect"][:, i0 + slot]).astype(np.int32)
                assert keep.kept[slot] == len(want) == 24 * 4 + 7               # four of every group of seven, and the class whose mean is NaN
                got = keep.sites(slot)
                missing, extra = np.setdiff1d(want, got), np.setdiff1d(got, want)
                assert not len(missing) and not len(extra), ("individual %d" % (i0 + slot), "not kept", missing, "kept", extra)
                same(got, want, "sites in ascending order")
            keep.close()
    finally:
        depth.close()
        b.close()


# ---------------------------------------------------------------- d. scan and compaction
@pytest.mark.parametrize("shape", range(len(zc.SCAN_SITES)))
def test_scan_and_compaction(shape):
    """kept, the site lists and the three compacted arrays across three individuals with different keep patterns; nothing is written
    behind the exact sizes."""
    from wgsassign_amd import _lib, zscore
    from wgsassign_amd._lib import check, f32p, i32p
    from wgsassign_amd.device import AFSet, DeviceBeagle
    m, names, keep_want = zc.scan_shapes()[shape]
    L, AD, key_mean, key_comp = zc.scan_inputs(m, keep_want)
    b = DeviceBeagle.from_host(L)
    depth = zscore.DepthTable(b)                                   # a fresh table: depth (0, 0) everywhere
    afs = AFSet.from_host(np.zeros((m, 1), dtype=F32))
    lib = _lib.load()
    try:
        keep = zscore.KeepSet(depth, 0, key_mean, key_comp)
        sites = [np.flatnonzero(keep_want[:, j]).astype(np.int32) for j in range(3)]
        assert list(keep.kept) == [len(s) for s in sites], (m, names)
        for j in range(3):
            out = np.full(len(sites[j]) + 1, -7, dtype=np.int32)
            check(lib.wgs_zkeep_sites(keep.handle, j, i32p(out)))
            assert out[-1] == -7
            same(out[:-1], sites[j], "sites of pattern %s at %d sites" % (names[j], m))
        total = int(keep.kept.sum())
        got = [np.full(total + 1, -7, dtype=F32) for _ in range(3)]
        ptrs = (ctypes.c_void_p * 3)(*[int(afs.col_dev(0))] * 3)
        tabs = zc.log_tables(3)
        check(lib.wgs_zscore_stats(keep.handle, f32p(tabs), ptrs, f32p(got[0]), f32p(got[1]), f32p(got[2])))
        assert all(g[-1] == -7 for g in got)
        wobs = np.concatenate([zscore_cpu._logf(L[sites[j], 2 * j]) for j in range(3)])
        assert len(np.unique(wobs)) == len(wobs) == total                        # a distinct value per kept site: the order shows
        same(got[0][:-1], wobs, "W_l_obs in site order, individual after individual")
        same(got[1][:-1], np.zeros(total, dtype=F32), "W_l")
        same(got[2][:-1], np.zeros(total, dtype=F32), "var_W_l")
        keep.close()
    finally:
        afs.close()
        depth.close()
        b.close()


# ---------------------------------------------------------------- e. the sweep's own logarithm
def sweep_log(x):
    """W_l_obs of one individual whose site s has depth (0, 0), g0 = x[s], g1 = 0 at frequency 0: zs_logf(x[s])."""
    from wgsassign_amd import zscore
    from wgsassign_amd.device import AFSet, DeviceBeagle
    L, AD, key_mean, key_comp = zc.log_inputs(x)
    b = DeviceBeagle.from_host(L)
    depth = zscore.DepthTable(b)
    afs = AFSet.from_host(np.zeros((len(x), 1), dtype=F32))
    try:
        keep = zscore.KeepSet(depth, 0, key_mean, key_comp)
        assert keep.kept[0] == len(x)
        wobs, wl, var = keep.stats(zc.log_tables(1), [afs.col_dev(0)])
        keep.close()
    finally:
        afs.close()
        depth.close()
        b.close()
    assert not wl[0].any() and not var[0].any()                    # log(1) = 0 in both loops
    return wobs[0]


_glibc_mismatches = {}


@pytest.mark.parametrize("part", ["quarter", "half", "one", "rest"])
def test_sweep_log_is_the_original(part, oracle):
    """Every argument of log_arguments(): zs_logf gives the bits of log_f32arg (wgs_debug_log_values), which tests/test_gpu_log.py
    holds to glibc exhaustively; against glibc itself no more arguments differ, over all parts, than the 16 allowed there."""
    from wgsassign_amd import _lib, device
    dev = (_lib.load(), device.get_context(), _lib)
    parts = zc.log_arguments()
    if part == "rest":
        bits = np.unique(np.concatenate((parts["stride"], parts["edges"], parts["specials"])))
        x = bits.view(F32)
        bits = bits[(x < F32(0.25)) | (x >= F32(2))]               # the three binades have launches of their own
        assert bits[0] == 0 and len(bits) > 250000
    else:
        bits = parts[part]
    x = np.ascontiguousarray(bits.view(F32))
    mine = sweep_log(x)
    original = original_log_values(dev, x)
    bad = np.flatnonzero(mine.view(np.uint32) != original.view(np.uint32))
    assert not len(bad), (len(bad), [hex(int(v)) for v in bits[bad[:4]]], mine[bad[:4]], original[bad[:4]])
    if part == "rest":
        assert mine[0] == -np.inf and np.isfinite(mine[1:]).all()
    ref = oracle.log_f32(x, min(len(os.sched_getaffinity(0)), 16))
    _glibc_mismatches[part] = int((mine.view(np.uint32) != ref.view(np.uint32)).sum())
    print("sweep log vs glibc, %s: %d of %d differ" % (part, _glibc_mismatches[part], len(x)))
    assert sum(_glibc_mismatches.values()) <= 16, _glibc_mismatches
