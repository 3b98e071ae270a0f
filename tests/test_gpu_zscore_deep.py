"""GPU: z-scores of individuals with sites deeper than 21 reads -- the sparse second tier of wgsassign_amd/zscore.py (deep-site list,
merged dictionary, deep tables read by the mask and statistic sweeps) held to the CPU restatement (tests/zscore_cpu.py, which
tests/test_zscore_deep_cpu.py pins to the real reference on such data) with no tolerance: every `details` array, the sums, z and
the iteration counts of the subset fits; the CLI byte for byte against the files recorded from the reference's CLI.

Main case: 20011 sites (not a multiple of 64, 313 tiles, across the 4096-site block boundary), 6 individuals in populations of
3 / 2 / 1, batches of 4 (the boundary falls inside the population of two).  Individual 0 has no deep site and shares its batch
with deep ones; 1 and 4 have 40 sites of depths 22-60 that are never complete (dropped); 2 has every class of the depths 22 and
23, four sites each (kept); 3 has single sites at (255, 255), (200, 0), (0, 37).  Every deep individual has its first deep sites at
sites 0 and 63 (lanes 0 and 63, two in the first tile), 4095 and 4096, 19968 and 20010 (the last, partial tile)."""
import contextlib
import io
import os

import numpy as np
import pytest

import synth_deep
import synth_depth
import zscore_cpu
from conftest import GOLDEN
from test_zscore_cpu import same
from test_zscore_deep_cpu import deep_inputs

pytestmark = pytest.mark.gpu

M, ROLES, SIZES = 20011, ("none", "dropped", "kept", "single", "dropped", "none"), (3, 2, 1)
_main, _want = [], {}


def main_case():
    if not _main:
        _main.append(synth_deep.make_deep(M, 6, 3, 11, ROLES, sizes=SIZES))
    return _main[0]


def restatement(oracle, flavour, thr=0, srt=False):
    """Computed once per (flavour, options) and shared."""
    key = (flavour, thr, srt)
    if key not in _want:
        L, AD, IDs, A, _ = main_case()
        if flavour == "assignment":
            _want[key] = zscore_cpu.assignment(L, AD, IDs, np.unique(IDs[:, 1]), A, thr, srt)
        else:               # the population of one has nobody left for a leave-one-out fit: individuals 0 .. 4
            _want[key] = zscore_cpu.reference(L, AD, IDs, lambda Lp, it, tol: oracle.emMAF(Lp, it, tol, 8), 200, 1e-4, thr, srt, None, 5)
    return _want[key]


def device_run(L, AD, IDs, A, flavour, thr=0, srt=False, batch=4, table=None, **kw):
    from wgsassign_amd import zscore
    from wgsassign_amd.device import AFSet, DeviceBeagle
    pops = np.unique(IDs[:, 1])
    group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
    b = DeviceBeagle.from_host(L, group_of, len(pops)) if flavour == "reference" else DeviceBeagle.from_host(L)
    depth = table(b) if table else zscore.DepthTable(b, AD, chunk_rows=3000)
    details = []
    try:
        if flavour == "reference":
            z = zscore.reference_z_scores(b, depth, IDs, group_of, 200, 1e-4, thr, srt, 0, 5, batch=batch, say=lambda *_: None,
                                          details=details, **kw)
        else:
            afs = AFSet.from_host(A)
            z = zscore.assignment_z_scores(b, depth, IDs, pops, afs, thr, srt, 0, None, batch=batch, say=lambda *_: None, details=details, **kw)
            for i, d in enumerate(details):
                d["A"] = np.ascontiguousarray(A[d["keep"], int(np.argwhere(pops == IDs[i, 1])[0][0])])
            afs.close()
    finally:
        depth.close()
        b.close()
    return z, details


def compare(details, want, flavour):
    assert len(details) == len(want) > 0
    for i, (d, w) in enumerate(zip(details, want)):
        tag = "individual %d " % i
        for k in ("keys", "counts", "means", "AD_array", "keep", "fac", "like", "index", "A", "wobs", "wl", "var"):
            same(d[k], w[k], tag + k)
        for k in ("W_l_obs", "z_mu", "z_var", "z"):
            same(np.float32(d[k]), np.float32(w[k]), tag + k)
        if flavour == "reference":
            assert d["it"] == w["extra"], tag + "iteration of the subset fit"


def kept_depths(r):
    return sorted(set(int(d) for d in r["AD_array"][:, 2] if d > 21))


def test_main_case_is_what_it_claims(oracle):
    """Conditions on the inputs, checked on the restatement: where the deep sites sit, which depths are kept, and that at least half of
    the kept individual's deep sites are in L_keep (otherwise a passing comparison could hide an untested deep path)."""
    L, AD, IDs, A, deep = main_case()
    assert [len(x) for x in deep] == [0, 40, 186, 3, 40, 0] and M % 64 and (M + 63) // 64 > 256
    for i in (1, 2, 4):
        assert set(deep[i][:2]) == {0, 63} and {4095, 4096, M // 64 * 64, M - 1} <= set(deep[i])
    assert set(deep[3]) == {0, 63, 4095}
    assert {tuple(AD[s, 6:8]) for s in deep[3]} == {(255, 255), (200, 0), (0, 37)}
    dl = AD[:, 0::2] + AD[:, 1::2]
    assert [int((dl[:, i] > 21).sum()) for i in range(6)] == [len(x) for x in deep]
    assert 22 <= dl[deep[1], 1].min() and dl[deep[1], 1].max() <= 60
    want = restatement(oracle, "assignment")
    assert [kept_depths(r) for r in want] == [[], [], [22, 23], [], [], []]
    assert want[2]["index"].shape == (24, 24)
    in_keep = np.isin(deep[2], want[2]["keep"]).sum()
    assert len(deep[2]) // 2 <= in_keep < len(deep[2])               # ... and the 0.01 filter drops some of them
    for i in (1, 3, 4):
        assert not np.isin(deep[i], want[i]["keep"]).any()


def test_assignment_flavour(oracle):
    """(On a build whose classes end at depth 21 this raises ValueError.)"""
    L, AD, IDs, A, _ = main_case()
    z, details = device_run(L, AD, IDs, A, "assignment")
    compare(details, restatement(oracle, "assignment"), "assignment")
    assert zscore_cpu.file_text(z[:, 0]) == zscore_cpu.file_text([w["z"] for w in restatement(oracle, "assignment")])


def test_reference_flavour(oracle):
    L, AD, IDs, A, deep = main_case()
    z, details = device_run(L, AD, IDs, A, "reference")
    want = restatement(oracle, "reference")
    compare(details, want, "reference")
    assert kept_depths(want[2]) == [22, 23] and np.isin(deep[2], want[2]["keep"]).sum() >= len(deep[2]) // 2
    assert all(w["extra"] > 0 for w in want)


def test_threshold_removes_one_class_of_depth_22(oracle):
    """--allele_count_threshold 3: class (10, 12) has two sites, every other class of the depths 22 and 23 four -- 22 is dropped, 23 kept."""
    L, AD, IDs, A, deep = main_case()
    want = restatement(oracle, "assignment", thr=3)
    assert kept_depths(want[2]) == [23]
    in_keep = np.isin(deep[2], want[2]["keep"]).sum()
    assert 48 <= in_keep <= 96
    z, details = device_run(L, AD, IDs, A, "assignment", thr=3)
    compare(details, want, "assignment")


def test_single_read_threshold(oracle):
    """Depth 1 only: the deep classes are in the dictionary and nowhere else."""
    L, AD, IDs, A, _ = main_case()
    want = restatement(oracle, "assignment", srt=True)
    assert (want[2]["keys"].sum(axis=1) > 21).sum() == 47 and list(want[2]["AD_array"][:, 2]) == [1, 1]
    z, details = device_run(L, AD, IDs, A, "assignment", srt=True)
    compare(details, want, "assignment")


def test_deep_site_list():
    """wgs_zscore_deep_sites: per individual the deep sites in site order with their depths and likelihoods, exact-sized from the
    counts of the class sweep; a batch that starts inside the deep individuals; sizes that are not the table's are refused."""
    from wgsassign_amd import _lib, zscore
    from wgsassign_amd._lib import check, f32p, i32p
    from wgsassign_amd.device import DeviceBeagle
    L, AD, IDs, A, deep = main_case()
    b = DeviceBeagle.from_host(L)
    depth = zscore.DepthTable(b, AD)
    lib = _lib.load()
    for i0, count in ((0, 6), (2, 3), (5, 1)):
        over = np.array([len(deep[i]) for i in range(i0, i0 + count)], dtype=np.int32)
        total = int(over.sum())
        site, ad, g = np.full(total + 1, -7, dtype=np.int32), np.full((total + 1, 2), -7, dtype=np.int32), np.full((total + 1, 2), -7, dtype=np.float32)
        check(lib.wgs_zscore_deep_sites(depth.handle, i0, count, i32p(over), i32p(site), i32p(ad), f32p(g)))
        assert site[-1] == -7 and ad[-1, 0] == -7 and g[-1, 0] == -7                  # nothing behind the exact size
        at = 0
        for i in range(i0, i0 + count):
            n = len(deep[i])
            assert np.array_equal(site[at:at + n], deep[i])
            assert np.array_equal(ad[at:at + n], AD[deep[i]][:, 2 * i:2 * i + 2])
            same(g[at:at + n], np.ascontiguousarray(L[deep[i]][:, 2 * i:2 * i + 2]), "likelihoods of the deep sites")
            at += n
    over = np.array([0, 41, 186], dtype=np.int32)
    site, ad, g = np.empty(227, dtype=np.int32), np.empty((227, 2), dtype=np.int32), np.empty((227, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="deeper than 21"):             # individual 1 has 40
        check(lib.wgs_zscore_deep_sites(depth.handle, 0, 3, i32p(over), i32p(site), i32p(ad), f32p(g)))
    depth.close()
    b.close()


def test_without_the_keyword_such_data_is_still_refused():
    from wgsassign_amd import zscore
    from wgsassign_amd.device import DeviceBeagle
    L, AD, IDs, A, _ = main_case()
    b = DeviceBeagle.from_host(L)
    depth = zscore.DepthTable(b, AD)
    with pytest.raises(ValueError, match="deeper than 21"):
        zscore.AD_summary(depth, 0, 4, 0, False)
    assert len(zscore.AD_summary(depth, 0, 1, 0, False)) == 1                       # individual 0 alone has no deep site
    with pytest.raises(ValueError, match="deeper than 21"):
        device_run(L, AD, IDs, A, "assignment", deep=False)
    got = zscore.AD_summary(depth, 0, 4, 0, False, deep=True)
    assert (got[3]["keys"].sum(axis=1) > 21).sum() == 3
    bad = np.full((4, 511), -1, dtype=np.int32)
    bad[1, 30] = 5                                                                  # rows 5 .. 35 of 8: outside
    with pytest.raises(ValueError, match="outside the rows"):
        zscore.KeepSet(depth, 0, np.zeros((4, 253), dtype=np.float32), np.full((4, 253), -1, dtype=np.int32), bad, np.zeros((8, 8), dtype=np.float32))
    depth.close()
    b.close()


def test_table_read_from_a_text_file(tmp_path, oracle):
    """The depth table of the main case through DepthTable.from_file (text): three-digit counts included."""
    from wgsassign_amd import zscore
    L, AD, IDs, A, _ = main_case()
    path = str(tmp_path / "ad.txt")
    np.savetxt(path, AD, fmt="%d")
    seen = []

    def table(b):
        t = zscore.DepthTable.from_file(b, path)
        seen.append(t.download_rows())
        return t
    z, details = device_run(L, AD, IDs, A, "assignment", table=table)
    assert np.array_equal(seen[0], AD)
    compare(details, restatement(oracle, "assignment"), "assignment")


@pytest.mark.parametrize("r, flavour", [(0, "assignment"), (1, "reference")])
def test_cli_matches_the_recorded_reference_cli(tmp_path, r, flavour):
    """Nothing new to type: both options on the recorded deep case, stdout lines and output file byte for byte."""
    from wgsassign_amd import WGSassign
    gold = np.load(os.path.join(GOLDEN, "zscore_deep.npz"), allow_pickle=False)
    L, AD, IDs, A, _ = deep_inputs(gold)
    paths = synth_depth.write_inputs(str(tmp_path / "in"), L, AD, IDs, A)
    out = str(tmp_path / ("run%d" % r))
    argv = ["--beagle", paths["beagle"], "--pop_af_IDs", paths["ids"], "--pop_names", paths["names"], "--ind_ad_file", paths["ad"],
            "--out", out, "--get_%s_z_score" % flavour]
    argv += ["--pop_af_file", paths["af"]] if flavour == "assignment" else ["--ind_end", "5"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        WGSassign.main(argv)
    keep = ("Finished individual", "z_mu", "z_var", "z_obs", "Loci used", "Z-score")
    lines = [ln.replace(str(tmp_path) + os.sep, "") for ln in buf.getvalue().splitlines()
             if ln.startswith(keep) or (ln.startswith("Saved ") and "z-scores" in ln)]
    assert lines == str(gold["run%d_stdout" % r]).splitlines()
    name = out + (".z_ind.txt" if flavour == "assignment" else ".reference_z_ind.txt")
    assert open(name).read() == str(gold["run%d_file" % r])
