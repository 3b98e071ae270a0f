"""--get_assignment_z_score in site windows, the parts that need no GPU: the byte count per site and the plan it gives, the command
line's routing and messages (a candidate and a variable of its own, the older routes answering as before), the merge of the class
sweep's per-window results into global numbers, the concatenation of the deep-site lists across windows, and the new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _args(*argv):
    from wgsassign_amd import WGSassign
    return WGSassign.parser.parse_args(list(argv))


BASE = ("--beagle", "x.beagle.gz", "--pop_af_file", "a.npy", "--pop_af_IDs", "ids.txt", "--pop_names", "p.txt", "--ind_ad_file", "ad.txt",
        "--get_assignment_z_score")
OTHERS = (("--get_pop_like",), ("--get_reference_af",), ("--get_reference_z_score",), ("--get_reference_af", "--loo"),
          ("--get_reference_af", "--ne_obs"))


# ---------------------------------------------------------------- the plan
def test_site_bytes():
    from wgsassign_amd import windows
    # matrix 16 per pair, depths 2 per individual, frequencies 4 per column, mask words 12 per (individual, 64 sites), statistics 12 per individual
    assert windows.z_site_bytes(200, 5, 200) == 16 * 100 + 2 * 200 + 4 * 5 + (12 * 200 + 63) // 64 + 12 * 200
    assert windows.z_site_bytes(7, 3, 1) == 16 * 4 + 14 + 12 + 1 + 12
    assert windows.z_site_bytes(200, 5, 64) < windows.z_site_bytes(200, 5, 200)
    assert windows.z_state_bytes(1) == 3 * 8192 * 4 + 12 + 256 * 12 + 144 and windows.z_state_bytes(10) == 10 * windows.z_state_bytes(1)
    assert windows.ENV_Z == "WGSASSIGN_Z_WINDOW_SITES" and windows.ENV_Z not in (windows.ENV, windows.ENV_LOO, windows.ENV_NE)


def test_plan_z():
    from wgsassign_amd import windows
    free = 100 << 30
    budget = windows.budget(free)
    n, K, count = 200, 5, 200
    resident = windows.z_site_bytes(n, K, 64)
    m_fits = budget // resident
    assert windows.plan_z(m_fits, n, K, count, free, environ={}) is None and windows.fits_resident_z(m_fits, n, K, count, free)
    W, batch = windows.plan_z(m_fits + 1, n, K, count, free, environ={})
    per_site = windows.z_site_bytes(n, K, count) + 16 * 100                    # one window's objects and the second matrix
    assert batch == count and W % 8192 == 0
    assert W == (budget - windows.z_state_bytes(count)) // per_site // 8192 * 8192
    assert windows.z_state_bytes(count) + W * per_site <= budget < windows.z_state_bytes(count) + (W + 8192) * per_site
    # the variable forces windows whatever fits, and only its own variable does
    assert windows.plan_z(1000, n, K, count, free, environ={"WGSASSIGN_Z_WINDOW_SITES": "20000"}) == (16384, count)
    for other in ("WGSASSIGN_WINDOW_SITES", "WGSASSIGN_LOO_WINDOW_SITES", "WGSASSIGN_NE_WINDOW_SITES"):
        assert windows.plan_z(1000, n, K, count, free, environ={other: "20000"}) is None
    with pytest.raises(ValueError, match="WGSASSIGN_Z_WINDOW_SITES=100 is below 8192"):
        windows.plan_z(1000, n, K, count, free, environ={"WGSASSIGN_Z_WINDOW_SITES": "100"})
    # rounds of individuals: in 1 GiB the state of 2000 individuals (203 MB) and their statistics leave no room for a window of 8192 sites
    small = 1 << 30
    W, batch = windows.plan_z(10 ** 7, 2000, 5, 2000, small, environ={})
    assert batch == 1000 and W >= 8192
    assert windows.z_state_bytes(batch) + W * (windows.z_site_bytes(2000, 5, batch) + 16 * 1000) <= windows.budget(small)
    assert windows.z_state_bytes(2 * batch) + 8192 * (windows.z_site_bytes(2000, 5, 2 * batch) + 16 * 1000) > windows.budget(small)
    assert windows.z_batch(8192, 2000, 5, 2000, small) == batch and windows.z_batch(8192, 6, 3, 6, free) == 6
    with pytest.raises(MemoryError, match="windowed z-scores need two windows of 8192 sites"):
        windows.plan_z(10 ** 7, 200000, 5, 10, 1 << 30, environ={})


# ---------------------------------------------------------------- the command line
def test_command_line_routing():
    from wgsassign_amd.WGSassign import windowed_z_candidate
    assert windowed_z_candidate(_args(*BASE), 1)
    assert windowed_z_candidate(_args(*BASE, "--single_read_threshold", "--ind_start", "2", "--ind_end", "5", "--threads", "8"), 1)
    assert windowed_z_candidate(_args(*BASE[:-3], "--ind_counts_file", "c.gz", "--ind_majmin_file", "m.txt", BASE[-1]), 1)
    assert not windowed_z_candidate(_args(*BASE), 2) and not windowed_z_candidate(_args(*BASE), 8)      # a rank of several holds a shard
    assert not windowed_z_candidate(_args(*BASE[:-1]), 1)
    assert not windowed_z_candidate(_args(*BASE[:-1], "--get_reference_z_score"), 1)                     # needs masked re-fits over the whole file
    for other in OTHERS:
        assert not windowed_z_candidate(_args(*BASE, *other), 1), other


def test_the_older_routes_answer_as_before():
    from wgsassign_amd import WGSassign
    args = _args(*BASE)
    for candidate in (WGSassign.windowed_candidate, WGSassign.windowed_fit_candidate, WGSassign.windowed_loo_candidate,
                      WGSassign.windowed_ne_candidate):
        assert not candidate(args, 1)
    assert WGSassign.windowed_candidate(_args("--beagle", "x.beagle.gz", "--get_pop_like", "--pop_af_file", "a.npy"), 1)
    assert WGSassign.WINDOWS_ONLY == "windowed scoring (WGSASSIGN_WINDOW_SITES) covers --get_pop_like on one rank only"


class OneRank:
    world = 1


class TwoRanks:
    world = 2


class Ctx:
    def mem_info(self):
        return 100 << 30, 100 << 30


def test_only_its_own_variable_routes_the_run(monkeypatch, tmp_path):
    from wgsassign_amd import WGSassign
    af = tmp_path / "a.npy"
    np.save(af, np.zeros((4, 2), dtype=np.float32))
    argv = ("--beagle", "x.gz", "--pop_af_file", str(af), "--get_assignment_z_score")
    monkeypatch.delenv("WGSASSIGN_Z_WINDOW_SITES", raising=False)
    for name in ("WGSASSIGN_WINDOW_SITES", "WGSASSIGN_LOO_WINDOW_SITES", "WGSASSIGN_NE_WINDOW_SITES"):
        monkeypatch.setenv(name, "20000")
    monkeypatch.setattr(WGSassign.os.path, "getsize", lambda p: 1)                  # (the first look: a file that surely fits)
    assert WGSassign._z_window_sites(_args(*argv), OneRank(), Ctx()) is None         # the older variables route no z-score run
    assert WGSassign._window_sites(_args(*argv), OneRank(), None) is None            # ... and the z-scores are none of their candidates
    monkeypatch.setenv("WGSASSIGN_Z_WINDOW_SITES", "20000")
    assert WGSassign._z_window_sites(_args(*argv), OneRank(), None) == (16384, None)
    assert WGSassign._z_window_sites(_args(*argv), TwoRanks(), None) is None
    assert WGSassign._z_window_sites(_args(*argv[:-1], "--get_reference_z_score"), OneRank(), None) is None
    assert WGSassign._z_window_sites(_args(*argv, "--get_reference_z_score"), OneRank(), None) is None
    assert WGSassign._z_window_sites(_args(*argv, "--get_pop_like"), OneRank(), None) is None
    assert WGSassign._z_window_sites(_args("--beagle", "x.gz", "--pop_af_file", str(tmp_path / "no.npy"), argv[-1]), OneRank(), None) is None
    monkeypatch.setenv("WGSASSIGN_Z_WINDOW_SITES", "eight")
    with pytest.raises(SystemExit, match="WGSASSIGN_Z_WINDOW_SITES must be a number of sites"):
        WGSassign._z_window_sites(_args(*argv), OneRank(), None)
    # its variable routes nothing else
    monkeypatch.setenv("WGSASSIGN_Z_WINDOW_SITES", "20000")
    for name in ("WGSASSIGN_WINDOW_SITES", "WGSASSIGN_LOO_WINDOW_SITES", "WGSASSIGN_NE_WINDOW_SITES"):
        monkeypatch.delenv(name)
    score = _args("--beagle", "x.gz", "--pop_af_file", str(af), "--get_pop_like")
    assert WGSassign._window_sites(score, OneRank(), Ctx()) is None


def test_the_hint_names_the_variable_of_the_option():
    from wgsassign_amd import WGSassign
    e = RuntimeError("wgsassign_amd HIP call failed: hipMalloc of 123 bytes for population slab 0 failed")
    z = WGSassign.with_windows_hint(e, WGSassign.windowed_candidate(_args(*BASE), 1), WGSassign.windowed_z_candidate(_args(*BASE), 1))
    assert str(z) == str(e) + ": " + WGSassign.SET_WINDOW_SITES_Z and "WGSASSIGN_Z_WINDOW_SITES" in str(z)
    # --get_reference_z_score and several ranks keep today's message
    for args, world in ((_args(*BASE[:-1], "--get_reference_z_score"), 1), (_args(*BASE, "--get_reference_z_score"), 1), (_args(*BASE), 2)):
        h = WGSassign.with_windows_hint(e, WGSassign.windowed_candidate(args, world), WGSassign.windowed_z_candidate(args, world))
        assert str(h) == str(e) + ": " + WGSassign.WINDOWS_ONLY
    assert str(WGSassign.with_windows_hint(e)) == str(e) + ": " + WGSassign.WINDOWS_ONLY
    assert str(WGSassign.with_windows_hint(e, True)) == str(e) + ": " + WGSassign.SET_WINDOW_SITES
    other = RuntimeError("something else")
    assert WGSassign.with_windows_hint(other, False, True) is other


def test_individuals_of_the_plan():
    from wgsassign_amd.WGSassign import _z_individuals
    assert _z_individuals(_args(*BASE), 10) == 10
    assert _z_individuals(_args(*BASE, "--ind_start", "2", "--ind_end", "5"), 10) == 3
    assert _z_individuals(_args(*BASE, "--ind_end", "50"), 10) == 10


# ---------------------------------------------------------------- host functions alone
def test_merge_of_the_class_sweep_across_windows():
    """Counts and `over` add as int64; a first site is the smallest site0 + local among the windows that have the class."""
    from wgsassign_amd import zscore
    C = zscore.N_CLASSES
    cnt_tot = np.zeros((2, C), dtype=np.int64)
    first = np.full((2, C), -1, dtype=np.int64)
    over = np.zeros(2, dtype=np.int64)
    windows = []
    for w, site0 in enumerate((0, 8192, 16384)):
        cnt = np.zeros((2, C), dtype=np.int32)
        f = np.full((2, C), -1, dtype=np.int32)
        windows.append((site0, cnt, f, np.array([w, 2 * w], dtype=np.int32)))
    windows[0][1][0, 3], windows[0][2][0, 3] = 5, 17                 # class 3 of individual 0: windows 1 and 3
    windows[2][1][0, 3], windows[2][2][0, 3] = 2, 0
    windows[1][1][0, 7], windows[1][2][0, 7] = 1, 8191               # class 7: window 2 only, its last site
    windows[2][1][1, 9], windows[2][2][1, 9] = 4, 0                  # class 9 of individual 1: window 3 only, its first site
    windows[1][1][1, 0], windows[1][2][1, 0] = 2 ** 31 - 1, 5        # counts beyond int32 when added
    windows[2][1][1, 0], windows[2][2][1, 0] = 2 ** 31 - 1, 6
    for site0, cnt, f, o in windows:
        zscore.merge_windows(cnt_tot, first, over, site0, cnt, f, o)
    assert cnt_tot[0, 3] == 7 and first[0, 3] == 17
    assert cnt_tot[0, 7] == 1 and first[0, 7] == 8192 + 8191
    assert cnt_tot[1, 9] == 4 and first[1, 9] == 16384
    assert cnt_tot[1, 0] == 2 ** 32 - 2 and first[1, 0] == 8192 + 5
    assert list(over) == [3, 6] and first.dtype == np.int64 and cnt_tot.dtype == np.int64
    assert (first[cnt_tot == 0] == -1).all() and (first[cnt_tot > 0] >= 0).all()


def test_dictionary_from_merged_windows_equals_the_one_of_one_window():
    """zscore.dictionaries on merged per-window results: the order of first appearance is the global one."""
    from wgsassign_amd import zscore
    C = zscore.N_CLASSES
    rng = np.random.default_rng(5)
    m, W = 20000, 8192
    cls = rng.integers(0, 40, size=m)
    cls[:W][cls[:W] == 33] = 1                      # class 33 appears in window 2 first, class 35 in window 3
    cls[:2 * W][cls[:2 * W] == 35] = 2
    whole_cnt = np.bincount(cls, minlength=C)[None, :C].astype(np.int32)
    whole_first = np.array([[np.flatnonzero(cls == k)[0] if (cls == k).any() else -1 for k in range(C)]], dtype=np.int32)
    sums = rng.random((1, C, 3)).astype(np.float32)
    cnt_tot, first, over = np.zeros((1, C), dtype=np.int64), np.full((1, C), -1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    for lo in range(0, m, W):
        part = cls[lo:lo + W]
        cnt = np.bincount(part, minlength=C)[None, :C].astype(np.int32)
        f = np.array([[np.flatnonzero(part == k)[0] if (part == k).any() else -1 for k in range(C)]], dtype=np.int32)
        zscore.merge_windows(cnt_tot, first, over, lo, cnt, f, np.zeros(1, dtype=np.int32))
    assert np.array_equal(cnt_tot, whole_cnt) and np.array_equal(first, whole_first)
    assert first[0, 33] >= W and first[0, 35] >= 2 * W
    a = zscore.dictionaries(0, cnt_tot, first, sums, over, None, 0, False, True)[0]
    b = zscore.dictionaries(0, whole_cnt, whole_first, sums, np.zeros(1, dtype=np.int32), None, 0, False, True)[0]
    for k in ("keys", "counts", "means", "AD_array"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_deep_lists_concatenate_in_window_order():
    from wgsassign_amd import zscore
    parts = [(np.array([3, 8000], dtype=np.int64) + 0, np.array([[22, 0], [0, 23]], dtype=np.int32), np.array([[1, 0], [0, 0]], dtype=np.float32)),
             (np.array([0], dtype=np.int64) + 8192, np.array([[22, 0]], dtype=np.int32), np.array([[0.5, 0.25]], dtype=np.float32)),
             (np.array([1, 3626], dtype=np.int64) + 16384, np.array([[0, 23], [11, 11]], dtype=np.int32), np.array([[0, 1], [0, 1]], dtype=np.float32))]
    site, ad, g = zscore.concat_deep(parts)
    assert list(site) == [3, 8000, 8192, 16385, 20010] and site.dtype == np.int64
    assert ad.shape == (5, 2) and g.shape == (5, 2) and g.dtype == np.float32
    keys, counts, first, sums = zscore.deep_classes(site, ad, g)
    where = {tuple(k): i for i, k in enumerate(keys)}
    assert counts[where[(22, 0)]] == 2 and first[where[(22, 0)]] == 3
    assert counts[where[(0, 23)]] == 2 and first[where[(0, 23)]] == 8000
    assert counts[where[(11, 11)]] == 1 and first[where[(11, 11)]] == 20010
    assert sums[where[(22, 0)]].tobytes() == np.array([1.5, 0.25, 0.25], dtype=np.float32).tobytes()     # site order: 1 + 0.5, ...


def test_finish_of_the_sums_prints_what_the_resident_run_prints():
    from wgsassign_amd import zscore
    rng = np.random.default_rng(1)
    w, l, v = (rng.random(9000).astype(np.float32) for _ in range(3))
    a, b = [], []
    r1 = zscore._finish(4, 9000, w, l, v, a.append)
    r2 = zscore._finish_sums(4, 9000, np.sum(w, dtype=np.float32), np.sum(l), np.sum(v), b.append)
    assert a == b and len(a) == 6 and all(np.float32(r1[k]).tobytes() == np.float32(r2[k]).tobytes() for k in r1)
    zscore._finish_sums(0, 0, np.float32(0), np.float32(0), np.float32(0), b.append)          # N = 0: nan, no warning raised as an error
    assert b[-1] == "Z-score: nan" and b[-2] == "Loci used: 0"


# ---------------------------------------------------------------- the C ABI
def test_new_symbols_are_declared_and_the_version_stays():
    text = open(os.path.join(ROOT, "include", "wgsassign_hip.h")).read()
    assert re.search(r"#define WGS_ABI_VERSION 4\b", text)
    for name in ("wgs_zsum_create", "wgs_zsum_destroy", "wgs_zsum_push", "wgs_zsum_totals", "wgs_zsum_finish", "wgs_zscore_classes_carry",
                 "wgs_zscore_stats_dev", "wgs_depth_copy_rows", "wgs_depth_ingest_set_selectors"):
        assert re.search(r"\b%s\s*\(" % name, text), name
    debug = open(os.path.join(ROOT, "include", "wgsassign_hip_debug.h")).read()
    assert re.search(r"\bwgs_debug_zsum_push\s*\(", debug) and "wgs_debug_zsum" not in text
    from wgsassign_amd import _lib
    lib = _lib.load()
    assert lib.wgs_version() == 4 and all(hasattr(lib, n) for n in ("wgs_zsum_push", "wgs_debug_zsum_push", "wgs_zscore_classes_carry"))
