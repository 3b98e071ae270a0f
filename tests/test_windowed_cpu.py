"""Windowed scoring, the parts that need no GPU: the new C-ABI symbols are bound, WGSASSIGN_WINDOW_SITES is rounded and refused,
the window is derived from the free device memory as wgsassign_amd/windows.py writes it down, and the command line routes
--get_pop_like alone on one rank -- and nothing else -- to the windows."""
import os
import re

import pytest

from conftest import ROOT

NEW_SYMBOLS = ("wgs_score_stream_create", "wgs_score_stream_push", "wgs_score_stream_finish", "wgs_score_stream_destroy",
               "wgs_beagle_set_window")


def test_new_symbols_are_declared_bound_and_exported():
    from wgsassign_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "wgsassign_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(wgs_[a-z0-9_]+)\s*\(", text))
    build.build()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define WGS_WINDOW_ALIGN 8192" in open(os.path.join(ROOT, "include", "wgsassign_hip.h")).read()


def test_window_sites_variable_is_rounded_down_and_refused_below_one_window():
    from wgsassign_amd import windows
    from wgsassign_amd.comm import SHARD_ALIGN
    assert windows.ALIGN == SHARD_ALIGN == 8192
    assert windows.env_window_sites({}) is None
    assert windows.env_window_sites({windows.ENV: ""}) is None
    assert windows.env_window_sites({windows.ENV: "8192"}) == 8192
    assert windows.env_window_sites({windows.ENV: "8193"}) == 8192
    assert windows.env_window_sites({windows.ENV: "16383"}) == 8192
    assert windows.env_window_sites({windows.ENV: "16384"}) == 16384
    assert windows.env_window_sites({windows.ENV: " 1000000 "}) == 999424          # 122 x 8192
    for bad in ("100", "8191", "0", "-8192", "many"):
        with pytest.raises(ValueError, match="WGSASSIGN_WINDOW_SITES"):
            windows.env_window_sites({windows.ENV: bad})
    # the variable decides before the memory is looked at
    assert windows.plan(10, 6, 3, 1 << 40, {windows.ENV: "20000"}) == 16384


def test_window_from_free_memory_on_made_up_numbers():
    from wgsassign_amd import windows
    n, K = 200, 5
    per_site = 16 * 100 + 4 * 5 + 4 * 50 + 8 * 254 + 1 + 8          # matrix + frequencies + class codes, as the module's docstring lists them
    assert per_site == 3861 and windows.site_bytes(n, K) == per_site
    assert windows.site_bytes(7, 3) == 16 * 4 + 12 + 8 + 2032 + 9     # an odd n: whole pairs and whole quads
    GiB = 1 << 30
    # 100 GiB free: 0.8 x 100 - 4 = 76 GiB may be used
    assert windows.budget(100 * GiB) == 76 * GiB
    fits = 76 * GiB // per_site
    assert windows.plan(fits, n, K, 100 * GiB, {}) is None              # a matrix that fits: no windows
    assert windows.plan(1_000_000, n, K, 100 * GiB, {}) is None
    W = windows.plan(fits + 1, n, K, 100 * GiB, {})                     # one site more: two windows must fit
    assert W == 76 * GiB // (2 * per_site) // 8192 * 8192 and W % 8192 == 0
    assert 2 * W * per_site <= 76 * GiB < 2 * (W + 8192) * per_site
    # 10 GiB free: the reserve is a quarter of it, 8 - 2.5 = 5.5 GiB may be used; two windows of 761856 sites (93 x 8192)
    assert windows.budget(10 * GiB) == 8 * GiB - 5 * GiB // 2
    m = int(3.2 * 761856)
    assert windows.plan(m, n, K, 10 * GiB, {}) == 761856
    assert m / 761856 > 3.19 and windows.window_count(m, 761856) == 4    # a file that needs 3.2 windows is scored in 4
    assert windows.window_count(3 * 761856, 761856) == 3 and windows.window_count(3 * 761856 + 1, 761856) == 4
    # 64 MiB free: two windows of 8192 sites need 63 MB, 35 MB may be used
    with pytest.raises(MemoryError, match="two windows of 8192 sites"):
        windows.plan(10_000_000, n, K, 64 << 20, {})


def _args(*argv):
    from wgsassign_amd import WGSassign
    return WGSassign.parser.parse_args(list(argv))


def test_command_line_routing_is_a_function_of_the_options():
    from wgsassign_amd.WGSassign import windowed_candidate
    base = ("--beagle", "x.beagle.gz", "--pop_af_file", "x.npy", "--get_pop_like")
    assert windowed_candidate(_args(*base), 1)
    assert windowed_candidate(_args(*base, "--threads", "8", "--out", "y", "--partition_sites", "3"), 1)
    assert not windowed_candidate(_args(*base), 2)                      # a rank of several holds a shard
    assert not windowed_candidate(_args("--beagle", "x.beagle.gz"), 1)   # nothing to score
    for other in (("--get_reference_af",), ("--get_reference_af", "--loo"), ("--loo",), ("--ne_obs",), ("--get_assignment_z_score",),
                  ("--get_reference_z_score",), ("--get_reference_af", "--loo", "--loo_downsampled_beagle", "d.beagle.gz")):
        assert not windowed_candidate(_args(*base, *other), 1), other
        assert not windowed_candidate(_args(*base[:2], *other), 1), other


def test_a_frequency_file_that_is_missing_is_left_to_the_resident_path(monkeypatch, tmp_path):
    """... which reports it where it always did; and other options never look at the variable at all."""
    from wgsassign_amd import WGSassign

    class OneRank:
        world = 1
    monkeypatch.setenv("WGSASSIGN_WINDOW_SITES", "100")
    args = _args("--beagle", "x.beagle.gz", "--pop_af_file", str(tmp_path / "missing.npy"), "--get_pop_like")
    assert WGSassign._window_sites(args, OneRank(), None) is None
    args = _args("--beagle", "x.beagle.gz", "--pop_af_file", str(tmp_path / "missing.npy"), "--get_pop_like", "--get_reference_af")
    assert WGSassign._window_sites(args, OneRank(), None) is None
    (tmp_path / "af.npy").write_bytes(b"")
    args = _args("--beagle", "x.beagle.gz", "--pop_af_file", str(tmp_path / "af.npy"), "--get_pop_like")
    with pytest.raises(SystemExit, match="WGSASSIGN_WINDOW_SITES"):
        WGSassign._window_sites(args, OneRank(), None)


def test_a_matrix_that_does_not_fit_says_what_windows_cover():
    """The hint hangs on the library's own message for a population slab that could not be allocated: the words it is recognised by
    are those csrc/api.hip prints, and no other error is touched."""
    from wgsassign_amd import WGSassign
    src = open(os.path.join(ROOT, "wgsassign_amd", "csrc", "api.hip")).read()
    formats = re.findall(r'wgs_set_error\("([^"]*)"', src)
    assert [f for f in formats if all(part in f for part in WGSassign.SLAB_ALLOC_FAILED)] == ["hipMalloc of %zu bytes for population slab %d failed"]
    e = RuntimeError("wgsassign_amd: hipMalloc of 800000000000 bytes for population slab 0 failed")
    hinted = WGSassign.with_windows_hint(e)
    assert isinstance(hinted, RuntimeError) and str(hinted) == str(e) + ": " + WGSassign.WINDOWS_ONLY
    assert "--get_pop_like on one rank only" in str(hinted)
    # the options windows do cover, on a file that was only judged to fit: how to ask for them
    asked = WGSassign.with_windows_hint(e, candidate=True)
    assert str(asked) == str(e) + ": " + WGSassign.SET_WINDOW_SITES and "set WGSASSIGN_WINDOW_SITES" in str(asked)
    assert "one rank only" not in str(asked)
    for other in (RuntimeError("wgsassign_amd: hipMalloc of 64 bytes for the block sums failed"), RuntimeError("Beagle file shorter than counted"),
                  ValueError("hipMalloc of 1 bytes for population slab 0 failed")):
        assert WGSassign.with_windows_hint(other) is other and WGSassign.with_windows_hint(other, True) is other


def test_a_small_file_is_sent_to_the_resident_path_by_its_size_alone(monkeypatch, tmp_path):
    from wgsassign_amd import WGSassign, windows
    GiB = 1 << 30
    assert windows.surely_fits(GiB, 100 * GiB)                       # 64 GiB against the 76 that may be used
    assert windows.surely_fits(76 * GiB // 64, 100 * GiB) and not windows.surely_fits(76 * GiB // 64 + 1, 100 * GiB)
    assert not windows.surely_fits(1, 0)

    class OneRank:
        world = 1

    class Ctx:
        def mem_info(self):
            return 100 * GiB, 288 * GiB
    monkeypatch.delenv("WGSASSIGN_WINDOW_SITES", raising=False)
    (tmp_path / "af.npy").write_bytes(b"not an array")
    (tmp_path / "x.beagle.gz").write_bytes(b"not a Beagle file")        # never opened: 17 bytes fit
    args = _args("--beagle", str(tmp_path / "x.beagle.gz"), "--pop_af_file", str(tmp_path / "af.npy"), "--get_pop_like")
    assert WGSassign._window_sites(args, OneRank(), Ctx()) is None
