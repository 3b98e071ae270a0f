"""--ne_obs in site windows, the parts that need no GPU: the command line's routing (a candidate and a variable of its own, the three
older routes answering as before), the byte count per site and the window it gives, the population means continued window by window
against np.mean, the new C-ABI symbols and the host-only push checks."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _args(*argv):
    from wgsassign_amd import WGSassign
    return WGSassign.parser.parse_args(list(argv))


BASE = ("--beagle", "x.beagle.gz", "--pop_af_IDs", "ids.txt", "--get_reference_af", "--ne_obs")
OTHERS = (("--get_pop_like", "--pop_af_file", "a.npy"), ("--get_assignment_z_score",), ("--get_reference_z_score",),
          ("--loo", "--loo_downsampled_beagle", "d.beagle.gz"))


def test_command_line_routing():
    from wgsassign_amd.WGSassign import windowed_ne_candidate
    assert windowed_ne_candidate(_args(*BASE), 1)
    assert windowed_ne_candidate(_args(*BASE, "--loo"), 1)
    assert windowed_ne_candidate(_args(*BASE, "--loo", "--partition_sites", "7", "--threads", "8", "--maf_iter", "50"), 1)
    assert windowed_ne_candidate(_args(*BASE, "--partition_sites", "3"), 1)
    assert not windowed_ne_candidate(_args(*BASE), 2) and not windowed_ne_candidate(_args(*BASE, "--loo"), 8)
    assert not windowed_ne_candidate(_args(*BASE[:-1]), 1)                                         # no --ne_obs: the fit's own route
    assert not windowed_ne_candidate(_args(*BASE[:-1], "--loo"), 1)                                # ... and the leave-one-out run's
    assert not windowed_ne_candidate(_args("--beagle", "x.beagle.gz", "--ne_obs"), 1)              # no --get_reference_af
    for other in OTHERS:
        assert not windowed_ne_candidate(_args(*BASE, *other), 1), other


def test_the_older_routes_answer_as_before():
    from wgsassign_amd.WGSassign import windowed_candidate, windowed_fit_candidate, windowed_loo_candidate
    for argv in (BASE, BASE + ("--loo",), BASE + ("--loo", "--partition_sites", "3")):
        args = _args(*argv)
        assert not windowed_candidate(args, 1) and not windowed_fit_candidate(args, 1) and not windowed_loo_candidate(args, 1), argv
    assert windowed_fit_candidate(_args(*BASE[:-1]), 1) and windowed_loo_candidate(_args(*BASE[:-1], "--loo"), 1)
    assert windowed_candidate(_args("--beagle", "x.beagle.gz", "--get_pop_like", "--pop_af_file", "a.npy"), 1)


class OneRank:
    world = 1


class Ctx:
    def mem_info(self):
        return 100 << 30, 100 << 30


def test_only_its_own_variable_routes_the_run(monkeypatch, tmp_path):
    from wgsassign_amd import WGSassign
    ids = tmp_path / "ids.txt"
    ids.write_text("a\tp\nb\tq\n")
    argv = ("--beagle", "x.gz", "--pop_af_IDs", str(ids), "--get_reference_af", "--ne_obs")
    monkeypatch.delenv("WGSASSIGN_NE_WINDOW_SITES", raising=False)
    monkeypatch.setenv("WGSASSIGN_WINDOW_SITES", "20000")
    monkeypatch.setenv("WGSASSIGN_LOO_WINDOW_SITES", "20000")
    monkeypatch.setattr(WGSassign.os.path, "getsize", lambda p: 1)                  # (the first look: a file that surely fits)
    for more in ((), ("--loo",), ("--loo", "--partition_sites", "3")):
        args = _args(*argv, *more)
        assert WGSassign._fit_window_sites(args, OneRank(), None) is None           # the two older variables route no --ne_obs run
        assert WGSassign._loo_window_sites(args, OneRank(), None) is None
        assert WGSassign._ne_window_sites(args, OneRank(), Ctx()) is None
    monkeypatch.setenv("WGSASSIGN_NE_WINDOW_SITES", "20000")
    for more in ((), ("--loo",), ("--loo", "--partition_sites", "3")):
        args = _args(*argv, *more)
        assert WGSassign._ne_window_sites(args, OneRank(), None) == 16384
        assert WGSassign._fit_window_sites(args, OneRank(), None) is None and WGSassign._loo_window_sites(args, OneRank(), None) is None
    # its variable routes nothing else
    monkeypatch.delenv("WGSASSIGN_WINDOW_SITES")
    monkeypatch.delenv("WGSASSIGN_LOO_WINDOW_SITES")
    assert WGSassign._ne_window_sites(_args(*argv[:-1]), OneRank(), None) is None
    assert WGSassign._ne_window_sites(_args(*argv[:-1], "--loo"), OneRank(), None) is None
    assert WGSassign._fit_window_sites(_args(*argv[:-1]), OneRank(), Ctx()) is None
    assert WGSassign._loo_window_sites(_args(*argv[:-1], "--loo"), OneRank(), Ctx()) is None
    assert WGSassign._ne_window_sites(_args(*argv, "--get_reference_z_score"), OneRank(), None) is None
    assert WGSassign._ne_window_sites(_args(*argv), type("TwoRanks", (), {"world": 2})(), None) is None
    assert WGSassign._ne_window_sites(_args("--beagle", "x.gz", "--pop_af_IDs", str(tmp_path / "no.txt"), "--get_reference_af", "--ne_obs"),
                                      OneRank(), None) is None
    for bad in ("100", "many"):
        monkeypatch.setenv("WGSASSIGN_NE_WINDOW_SITES", bad)
        with pytest.raises(SystemExit, match="WGSASSIGN_NE_WINDOW_SITES"):
            WGSassign._ne_window_sites(_args(*argv), OneRank(), None)


def test_ne_bytes_per_site_on_made_up_numbers():
    from wgsassign_amd import windows
    n, K = 200, 5
    counts = [40] * 5
    # matrix 16 * 100 pairs, frequencies 4 K, results 12 K, leaf sums ceil(4 * 200 / 128) = 7
    assert windows.ne_site_bytes(n, K, counts) == 1600 + 20 + 60 + 7 == 1687
    assert windows.ne_site_bytes(n, K) == 16 * ((n + K) // 2) + 80 + 7                       # the worst split when the counts are not known
    assert windows.ne_site_bytes(13, 3, [1, 4, 7]) == 16 * (1 + 2 + 4) + 12 + 36 + 1
    fit, loo = windows.fit_site_bytes(n, K, counts), windows.loo_site_bytes(n, K, counts, 3)
    assert windows.ne_site_bytes(n, K, counts) < fit < loo          # the fit before the pass needs more per site than the pass
    GiB = 1 << 30
    fits = 76 * GiB // fit
    assert windows.plan_ne(fits, n, K, 100 * GiB, {}, counts) is None
    W = windows.plan_ne(fits + 1, n, K, 100 * GiB, {}, counts)
    assert W == 76 * GiB // (2 * fit) // 8192 * 8192 and W % 8192 == 0 and W == windows.plan_fit(fits + 1, n, K, 100 * GiB, {}, counts)
    Wl = windows.plan_ne(fits + 1, n, K, 100 * GiB, {}, counts, loo=True, P=3)
    assert Wl == 76 * GiB // (2 * loo) // 8192 * 8192 and Wl % 8192 == 0 and 0 < Wl < W      # with --loo: the smaller window
    assert Wl == windows.plan_loo(fits + 1, n, K, 100 * GiB, {}, counts, 3)
    assert windows.plan_ne(10, n, K, 1 << 40, {windows.ENV_NE: "20000"}) == 16384
    assert windows.plan_ne(10, n, K, 1 << 40, {windows.ENV_NE: "20000"}, loo=True) == 16384
    assert windows.plan_ne(10, n, K, 1 << 40, {windows.ENV: "20000", windows.ENV_LOO: "20000"}) is None     # the older variables route nothing
    assert windows.plan_fit(10, n, K, 1 << 40, {windows.ENV_NE: "20000"}) is None
    assert windows.plan_loo(10, n, K, 1 << 40, {windows.ENV_NE: "20000"}) is None
    with pytest.raises(MemoryError, match="two windows of 8192 sites"):
        windows.plan_ne(10_000_000, n, K, 64 << 20, {})
    for free in (8 * GiB, 33 * GiB, 250 * GiB):
        for many in (10 ** 8, 10 ** 9):
            w = windows.plan_ne(many, 1000, 7, free, {})
            assert w is None or (w >= 8192 and w % 8192 == 0)


@pytest.mark.parametrize("m", [1, 8191, 8192, 8193, 20000, 100003])
def test_continued_column_mean_is_numpy_mean(m):
    """np.mean(a, axis=0) of a C-contiguous (m, K) float32 array is a serial float32 chain down every column and one true_divide:
    continued over windows of 8192 (and 16384) rows it keeps its bytes.  One column (K = 1) is a contiguous vector, which NumPy sums
    pairwise within every 8192 elements: the continuation follows that, too."""
    from wgsassign_amd import fisher
    for K, seed in ((3, 1), (5, 2), (1, 3), (2, 4), (1, 5), (1, 6)):
        rng = np.random.default_rng(seed * 1000 + m % 997)
        a = (rng.random((m, K)) * rng.choice([1e-3, 1.0, 50.0], size=K)).astype(np.float32)
        want = np.mean(a, axis=0)
        for W in (8192, 16384):
            running = None
            for lo in range(0, m, W):
                running = fisher.continue_column_sum(running, a[lo:lo + W])
            before = running.copy()
            got = fisher.column_mean(running, m)
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (m, K, W)
            assert running.tobytes() == before.tobytes()            # the totals are left as they were


def test_new_symbols_are_declared_bound_and_exported():
    from wgsassign_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "wgsassign_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(wgs_[a-z0-9_]+)\s*\(", text))
    debug = open(os.path.join(ROOT, "include", "wgsassign_hip_debug.h")).read()
    build.build()
    lib = _lib.load()
    for name in ("wgs_fisher_stream_create", "wgs_fisher_stream_push", "wgs_fisher_stream_sweep_ms", "wgs_fisher_stream_finish",
                 "wgs_fisher_stream_destroy"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name not in debug
    version = int(re.search(r"#define WGS_ABI_VERSION (\d+)", header).group(1))
    assert version == 4 == _lib.ABI_VERSION == lib.wgs_version()
    assert "`WGS_ABI_VERSION` (4)" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert '"stream_checks.h"' in open(os.path.join(ROOT, "wgsassign_amd", "build.py")).read()


def test_push_checks_under_the_sanitizers(tmp_path):
    """csrc/stream_checks.h is host-only: the `fisher` part of tests/c_abi/stream_checks_check.cpp drives what wgs_fisher_stream_push
    and wgs_fisher_stream_finish refuse, and the accepted sequences, under AddressSanitizer + UBSan, as a program of its own."""
    import sanitized
    r = sanitized.run(tmp_path, "stream_checks_check.cpp", "fisher")
    assert r.returncode == 0 and r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 100, (r.stdout[-2000:], r.stderr[-3000:])
