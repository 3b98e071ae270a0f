"""--get_reference_af --loo --loo_downsampled_beagle in site windows, the parts that need no GPU: the byte count per kept site and
the plan, the mapping from windows of kept sites to file rows (a pure function of the mask and W), the command line's routing and
its hint, the new C-ABI symbol and the host-only checks of the scored window."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

GiB = 1 << 30


def test_bytes_per_kept_site_on_made_up_numbers():
    from wgsassign_amd import windows
    n, K = 200, 5
    counts = [40] * 5
    loo = windows.loo_site_bytes(n, K, counts)
    assert loo == 15855
    # one more set of population slabs (5 x 20 float4 per site) and the codes of a scoring sweep on them: the class counts, the
    # dictionary, the encoder's records, and per slab 10 quads of code bytes and the row counts
    extra = 16 * 100 + (1 + 8 * 254 + 8) + 4 * 50 + 5
    assert windows.loo_ds_site_bytes(n, K, counts) == loo + extra == 19701
    assert windows.loo_ds_site_bytes(n, K, counts, P=5) == windows.loo_site_bytes(n, K, counts, P=5) + extra
    # the worst split when the counts are not known: never less
    assert windows.loo_ds_site_bytes(n, K) - windows.loo_site_bytes(n, K) == 16 * ((n + K) // 2) + 2041 + 4 * ((n + 3 * K) // 4) + K
    assert windows.loo_ds_site_bytes(n, K) >= windows.loo_ds_site_bytes(n, K, counts)
    # uneven populations: pairs and quads are rounded up per slab
    assert windows.loo_ds_site_bytes(12, 3, [2, 4, 6]) - windows.loo_site_bytes(12, 3, [2, 4, 6]) == 16 * 6 + 2041 + 4 * 4 + 3


def test_plan_on_made_up_numbers():
    from wgsassign_amd import windows
    n, K = 200, 5
    counts = [40] * 5
    fit, per_site = windows.fit_site_bytes(n, K, counts), windows.loo_ds_site_bytes(n, K, counts)
    resident = fit + per_site - windows.loo_site_bytes(n, K, counts)          # two matrices: the fitted one, and the scored one with its codes
    assert resident == 14247 + 3846
    fits = 76 * GiB // resident                 # budget(100 GiB) = 80 - 4
    assert windows.budget(100 * GiB) == 76 * GiB
    assert windows.fits_resident_loo_ds(fits, n, K, 100 * GiB, counts) and not windows.fits_resident_loo_ds(fits + 1, n, K, 100 * GiB, counts)
    assert windows.plan_loo_ds(fits, n, K, 100 * GiB, {}, counts) is None
    W = windows.plan_loo_ds(fits + 1, n, K, 100 * GiB, {}, counts)
    assert W == 76 * GiB // (2 * per_site) // 8192 * 8192 and W % 8192 == 0 and W >= 8192
    assert 2 * W * per_site <= 76 * GiB < 2 * (W + 8192) * per_site
    # what one resident matrix would take is not the question: a file pair that fits once and not twice goes to windows
    assert windows.plan_loo(fits + 1, n, K, 100 * GiB, {}, counts) is None
    # more partitions, smaller windows -- never larger
    assert windows.plan_loo_ds(fits + 1, n, K, 100 * GiB, {}, counts, P=4096) <= W
    with pytest.raises(MemoryError, match="two windows of 8192 sites x 200 individuals of both files"):
        windows.plan_loo_ds(10_000_000, n, K, 64 << 20, {})
    # exactly two windows of 8192 sites: the smallest memory that is enough, and one byte of budget less
    need = 2 * 8192 * per_site
    free = next(f for f in range(need * 5 // 4, need * 2) if windows.budget(f) >= need)
    assert windows.plan_loo_ds(10_000_000, n, K, free, {}, counts) == 8192
    with pytest.raises(MemoryError, match="can be used"):
        windows.plan_loo_ds(10_000_000, n, K, free - 2, {}, counts)


def test_only_its_own_variable_routes_the_plan():
    from wgsassign_amd import windows
    assert windows.ENV_LOO_DS == "WGSASSIGN_LOO_DS_WINDOW_SITES"
    assert windows.plan_loo_ds(10, 12, 3, 1 << 40, {windows.ENV_LOO_DS: "20000"}) == 16384
    assert windows.plan_loo_ds(10, 12, 3, 1 << 40, {windows.ENV_LOO_DS: "8192"}) == 8192
    for other in (windows.ENV, windows.ENV_LOO, windows.ENV_NE, windows.ENV_Z, windows.ENV_ZREF):
        assert windows.plan_loo_ds(10, 12, 3, 1 << 40, {other: "20000"}) is None, other
    assert windows.plan_loo(10, 12, 3, 1 << 40, {windows.ENV_LOO_DS: "20000"}) is None
    assert windows.plan_fit(10, 12, 3, 1 << 40, {windows.ENV_LOO_DS: "20000"}) is None
    with pytest.raises(ValueError, match="WGSASSIGN_LOO_DS_WINDOW_SITES=100 is below 8192"):
        windows.plan_loo_ds(10, 12, 3, 1 << 40, {windows.ENV_LOO_DS: "100"})


def by_hand(keep, W):
    """kept_windows the slow way: walk the rows, count the kept ones."""
    out, rows = [], []
    for r, k in enumerate(keep):
        if k:
            rows.append(r)
    for lo in range(0, len(rows), W):
        part = rows[lo:lo + W]
        out.append((lo, len(part), part[0], part[-1] + 1))
    return out


def check_windows(keep, W):
    from wgsassign_amd import windows
    keep = np.asarray(keep, dtype=bool)
    got = windows.kept_windows(keep, W)
    assert got == by_hand(keep, W)
    kept = int(keep.sum())
    assert len(got) == windows.window_count(kept, W) and sum(c for _, c, _, _ in got) == kept
    end = 0
    for w, (lo, count, r0, r1) in enumerate(got):
        assert lo == w * W and count == min(W, kept - lo)
        assert keep[r0] and keep[r1 - 1] and r0 >= end          # a window begins and ends with a kept row; windows do not overlap
        assert int(keep[r0:r1].sum()) == count                  # ... and holds exactly its kept sites
        assert not keep[end:r0].any()                           # the rows between two windows are dropped rows
        end = r1
    assert not keep[end:].any()
    return got


def test_kept_windows_to_file_rows():
    W = 8
    assert check_windows(np.ones(20, dtype=bool), W) == [(0, 8, 0, 8), (8, 8, 8, 16), (16, 4, 16, 20)]
    assert check_windows(np.ones(16, dtype=bool), W) == [(0, 8, 0, 8), (8, 8, 8, 16)]
    keep = np.ones(20, dtype=bool)
    keep[0] = False                                             # a dropped first row
    assert check_windows(keep, W) == [(0, 8, 1, 9), (8, 8, 9, 17), (16, 3, 17, 20)]
    keep = np.ones(20, dtype=bool)
    keep[-1] = False                                            # a dropped last row: the last window ends before it
    assert check_windows(keep, W) == [(0, 8, 0, 8), (8, 8, 8, 16), (16, 3, 16, 19)]
    keep = np.ones(21, dtype=bool)
    keep[[7, 8, 10]] = False                                    # dropped rows on both sides of a window edge
    assert check_windows(keep, W) == [(0, 8, 0, 10), (8, 8, 11, 19), (16, 2, 19, 21)]       # row 10 belongs to neither window
    keep = np.ones(40, dtype=bool)
    keep[8:30] = False                                          # an all-dropped stretch longer than W, right at a window edge
    assert check_windows(keep, W) == [(0, 8, 0, 8), (8, 8, 30, 38), (16, 2, 38, 40)]
    keep = np.ones(40, dtype=bool)
    keep[3:25] = False                                          # ... and inside a window
    assert check_windows(keep, W) == [(0, 8, 0, 30), (8, 8, 30, 38), (16, 2, 38, 40)]
    keep = np.zeros(40, dtype=bool)
    keep[[5, 39]] = True
    assert check_windows(keep, W) == [(0, 2, 5, 40)]
    assert check_windows(np.zeros(40, dtype=bool), W) == []    # a mask with no kept site: no windows
    assert check_windows(np.zeros(0, dtype=bool), W) == []
    assert check_windows([0, 1, 0], 8192) == [(0, 1, 1, 2)]
    rng = np.random.default_rng(17)
    for _ in range(50):
        m = int(rng.integers(1, 300))
        check_windows(rng.random(m) < rng.random(), int(rng.integers(1, 40)))
    with pytest.raises(ValueError):
        check_windows(np.ones(4, dtype=bool), 0)
    # at the sizes of the GPU tests: window edges of 8192 kept sites
    keep = np.ones(21000, dtype=bool)
    keep[0] = keep[-1] = False
    keep[3000:3400] = False
    got = check_windows(keep, 8192)
    assert got[0] == (0, 8192, 1, 8593) and got[1][2] == 8593 and got[-1][3] == 20999


def _args(*argv):
    from wgsassign_amd import WGSassign
    return WGSassign.parser.parse_args(list(argv))


BASE = ("--beagle", "x.beagle.gz", "--pop_af_IDs", "ids.txt", "--get_reference_af", "--loo", "--loo_downsampled_beagle", "d.beagle.gz")


def test_command_line_routing():
    from wgsassign_amd.WGSassign import (windowed_candidate, windowed_fit_candidate, windowed_loo_candidate, windowed_loo_ds_candidate,
                                         windowed_ne_candidate, windowed_z_candidate, windowed_zref_candidate)
    assert windowed_loo_ds_candidate(_args(*BASE), 1)
    assert windowed_loo_ds_candidate(_args(*BASE, "--partition_sites", "7", "--threads", "8", "--maf_iter", "50"), 1)
    assert not windowed_loo_ds_candidate(_args(*BASE), 2)
    assert not windowed_loo_ds_candidate(_args(*BASE[:-2]), 1)                                  # no downsampled file: the route of --loo
    assert not windowed_loo_ds_candidate(_args(*BASE[:4], *BASE[5:]), 1)                        # no --get_reference_af
    assert not windowed_loo_ds_candidate(_args(*BASE[:5], *BASE[6:]), 1)                        # no --loo (refused by main() anyway)
    for other in (("--ne_obs",), ("--get_pop_like", "--pop_af_file", "a.npy"), ("--get_assignment_z_score",), ("--get_reference_z_score",)):
        assert not windowed_loo_ds_candidate(_args(*BASE, *other), 1), other
    # the older candidates answer as before: False as soon as the flag is given
    for older in (windowed_candidate, windowed_fit_candidate, windowed_loo_candidate, windowed_ne_candidate, windowed_z_candidate,
                  windowed_zref_candidate):
        assert not older(_args(*BASE), 1), older.__name__
        assert not older(_args(*BASE, "--ne_obs"), 1), older.__name__
    assert windowed_loo_candidate(_args(*BASE[:-2]), 1) and windowed_fit_candidate(_args(*BASE[:5]), 1)
    assert windowed_ne_candidate(_args(*BASE[:-2], "--ne_obs"), 1)


class OneRank:
    world = 1


class TwoRanks:
    world = 2


class Ctx:
    def __init__(self, free=100 * GiB):
        self.free = free

    def mem_info(self):
        return self.free, self.free


def test_window_sites_of_the_command_line(monkeypatch, tmp_path):
    from wgsassign_amd import WGSassign, reader_cy, windows
    ids = tmp_path / "ids.txt"
    ids.write_text("".join("i%d\tp%d\n" % (i, i % 3) for i in range(12)))
    argv = ("--beagle", "x.gz", "--pop_af_IDs", str(ids), "--get_reference_af", "--loo", "--loo_downsampled_beagle", "d.gz")
    for name in (windows.ENV, windows.ENV_LOO, windows.ENV_NE, windows.ENV_LOO_DS):
        monkeypatch.delenv(name, raising=False)
    sizes = {"x.gz": 1, "d.gz": 1}
    monkeypatch.setattr(WGSassign.os.path, "getsize", lambda p: sizes[p])
    # unset: a pair that surely fits is looked at no further (no index, no ID file read)
    monkeypatch.setattr(reader_cy, "ensure_index", lambda *a, **kw: pytest.fail("the index was asked for"))
    assert WGSassign._loo_ds_window_sites(_args(*argv), OneRank(), Ctx()) is None
    # the other variables route nothing
    monkeypatch.setenv(windows.ENV, "20000")
    monkeypatch.setenv(windows.ENV_LOO, "20000")
    assert WGSassign._loo_ds_window_sites(_args(*argv), OneRank(), Ctx()) is None
    assert WGSassign._loo_window_sites(_args(*argv), OneRank(), Ctx()) is None
    assert WGSassign._fit_window_sites(_args(*argv), OneRank(), Ctx()) is None
    # set: checked first, before the device is asked anything
    monkeypatch.setenv(windows.ENV_LOO_DS, "20000")
    assert WGSassign._loo_ds_window_sites(_args(*argv), OneRank(), None) == 16384
    assert WGSassign._loo_ds_window_sites(_args(*argv, "--partition_sites", "3"), OneRank(), None, m_kept=5) == 16384
    assert WGSassign._loo_ds_window_sites(_args(*argv), TwoRanks(), None) is None
    assert WGSassign._loo_ds_window_sites(_args(*argv, "--ne_obs"), OneRank(), None) is None
    assert WGSassign._loo_ds_window_sites(_args(*argv[:-2]), OneRank(), None) is None
    monkeypatch.delenv(windows.ENV_LOO)
    assert WGSassign._loo_window_sites(_args(*argv[:-2]), OneRank(), Ctx()) is None          # ... and it routes no plain --loo
    missing = ("--beagle", "x.gz", "--pop_af_IDs", str(tmp_path / "no.txt")) + argv[4:]
    assert WGSassign._loo_ds_window_sites(_args(*missing), OneRank(), None) is None           # reported where it always was
    monkeypatch.setenv(windows.ENV_LOO_DS, "100")
    with pytest.raises(SystemExit, match="WGSASSIGN_LOO_DS_WINDOW_SITES"):
        WGSassign._loo_ds_window_sites(_args(*argv), OneRank(), None)
    monkeypatch.setenv(windows.ENV_LOO_DS, "many")
    with pytest.raises(SystemExit, match="WGSASSIGN_LOO_DS_WINDOW_SITES"):
        WGSassign._loo_ds_window_sites(_args(*argv), OneRank(), None)
    # unset, and the SUM of the two sizes does not surely fit (either alone would): the plan on the kept count decides
    monkeypatch.delenv(windows.ENV_LOO_DS)
    half = windows.budget(100 * GiB) // windows.SURELY_FITS // 2
    sizes.update({"x.gz": half + 1, "d.gz": half + 1})
    assert windows.surely_fits(half + 1, 100 * GiB) and not windows.surely_fits(2 * half + 2, 100 * GiB)
    counts = [4, 4, 4]
    resident = windows.fit_site_bytes(12, 3, counts) + windows.loo_ds_site_bytes(12, 3, counts) - windows.loo_site_bytes(12, 3, counts)
    fits = windows.budget(100 * GiB) // resident
    assert WGSassign._loo_ds_window_sites(_args(*argv), OneRank(), Ctx(), m_kept=fits) is None
    W = WGSassign._loo_ds_window_sites(_args(*argv, "--partition_sites", "3"), OneRank(), Ctx(), m_kept=fits + 1)
    assert W == windows.plan_loo_ds(fits + 1, 12, 3, 100 * GiB, {}, counts, 3) and W % 8192 == 0
    # no kept count given: the reference file's sites bound it
    monkeypatch.setattr(reader_cy, "ensure_index", lambda path, *a, **kw: ("idx", None, fits + 1 if path == "x.gz" else 10 ** 12))
    assert WGSassign._loo_ds_window_sites(_args(*argv, "--partition_sites", "3"), OneRank(), Ctx()) == W
    with pytest.raises(SystemExit, match="two windows of 8192 sites"):
        WGSassign._loo_ds_window_sites(_args(*argv), OneRank(), Ctx(64 << 20), m_kept=10_000_000)
    ids.write_text("not a table")
    assert WGSassign._loo_ds_window_sites(_args(*argv), OneRank(), Ctx(), m_kept=fits + 1) is None    # reported where it always was


def test_hint_texts():
    from wgsassign_amd import WGSassign
    from wgsassign_amd.WGSassign import with_windows_hint
    assert WGSassign.WINDOWS_ONLY == "windowed scoring (WGSASSIGN_WINDOW_SITES) covers --get_pop_like on one rank only"
    assert "WGSASSIGN_LOO_DS_WINDOW_SITES" in WGSassign.SET_WINDOW_SITES_LOO_DS and "8192" in WGSassign.SET_WINDOW_SITES_LOO_DS
    e = RuntimeError("wgsassign_amd HIP call failed: api.hip:1: hipMalloc of 123 bytes for population slab 0 failed: out of memory")
    assert str(with_windows_hint(e, loo_ds_candidate=True)) == str(e) + ": " + WGSassign.SET_WINDOW_SITES_LOO_DS
    assert str(with_windows_hint(e)) == str(e) + ": " + WGSassign.WINDOWS_ONLY == str(with_windows_hint(e, loo_ds_candidate=False))
    assert str(with_windows_hint(e, candidate=True)) == str(e) + ": " + WGSassign.SET_WINDOW_SITES
    assert str(with_windows_hint(e, z_candidate=True)) == str(e) + ": " + WGSassign.SET_WINDOW_SITES_Z
    assert str(with_windows_hint(e, zref_candidate=True)) == str(e) + ": " + WGSassign.SET_WINDOW_SITES_ZREF
    assert str(with_windows_hint(e, True, False, False)) == str(e) + ": " + WGSassign.SET_WINDOW_SITES        # positional, as before
    other = RuntimeError("something else")
    assert with_windows_hint(other, loo_ds_candidate=True) is other
    assert with_windows_hint(ValueError(str(e)), loo_ds_candidate=True).args == (str(e),)


def test_keywords_exist():
    import inspect

    from wgsassign_amd import device, emMAF, glassy, reader_cy
    assert inspect.signature(reader_cy.stream_windows).parameters["keep"].default is None
    assert inspect.signature(emMAF.emMAF_windowed).parameters["keep"].default is None
    sig = inspect.signature(glassy.loo_windowed).parameters
    assert all(sig[k].default is None for k in ("keep", "scored_path", "scored_keep"))
    assert list(inspect.signature(device.LooStream.push).parameters) == ["self", "em", "afset", "mode", "scored"]


def test_new_symbol_is_declared_bound_and_exported():
    from wgsassign_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "wgsassign_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int wgs_loo_stream_push_scored\(wgs_loo_stream \*stream, wgs_em \*window_em, wgs_beagle \*scored_window, "
                     r"wgs_afset \*window_af, int mode\);", text)
    assert "int wgs_loo_stream_push(wgs_loo_stream *stream, wgs_em *window_em, wgs_afset *window_af, int mode);" in text
    assert re.search(r"#define WGS_ABI_VERSION 4\b", text) and "wgs_loo_stream_push_scored" in header.split("#define WGS_ABI_VERSION")[0]
    build.build()
    lib = _lib.load()
    assert "wgs_loo_stream_push_scored" in _lib.SIGNATURES and hasattr(lib, "wgs_loo_stream_push_scored")
    assert len(_lib.SIGNATURES["wgs_loo_stream_push_scored"][1]) == 5


def test_one_body_behind_both_entry_points():
    """wgs_loo_stream_push is the scored_window == window_em->b case: one wgs_score_create and one parts_exact_literal call in the
    stream's push, both on the scored matrix."""
    src = open(os.path.join(ROOT, "wgsassign_amd", "csrc", "score_api.hip")).read()
    plain = src[src.index("int wgs_loo_stream_push(wgs_loo_stream *st"):src.index("int wgs_loo_stream_push_scored(wgs_loo_stream *st")]
    assert "return wgs_loo_stream_push_scored(st, window_em, window_em->b, window_af, mode);" in plain
    assert "wgs_score_create" not in plain and "parts_exact_literal" not in plain
    body = src[src.index("int wgs_loo_stream_push_scored(wgs_loo_stream *st"):src.index("int wgs_loo_stream_finish(")]
    assert body.count("wgs_score_create(") == 1 and "wgs_score_create(scored_window, window_af" in body
    assert body.count("parts_exact_literal(") == 1 and "parts_exact_literal(scored_window, window_af" in body
    assert "loo_stream_scored_refusal(" in body


def test_scored_window_checks_under_the_sanitizers(tmp_path):
    """csrc/stream_checks.h is host-only: the `scored` part of tests/c_abi/stream_checks_check.cpp drives what
    wgs_loo_stream_push_scored refuses of the scored window under AddressSanitizer + UBSan, as a program of its own."""
    import sanitized
    r = sanitized.run(tmp_path, "stream_checks_check.cpp", "scored")
    assert r.returncode == 0 and r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 100, (r.stdout[-2000:], r.stderr[-3000:])
