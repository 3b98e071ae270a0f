"""CPU-only: the enumerated z-score inputs of tests/zscore_cases.py are what they claim to be, checked on the restatement
(tests/zscore_cpu.py) -- so that a passing comparison in tests/test_gpu_zscore_classes.py cannot hide a path that the inputs never
reach -- and the restatement itself reproduces, bit for bit, what the real reference returned on such inputs
(tests/golden/zscore_classes.npz, made by tests/golden/make_golden_zscore_classes.py): every depth 1 .. 21 kept, AD_index (22, 22)."""
import ast
import os

import numpy as np
import pytest

import synth_depth
import zscore_cases as zc
import zscore_cpu
from conftest import GOLDEN
from test_zscore_cpu import compare_individual, runs

F32 = np.float32
_cache = {}


def classes_case(name="every_class", **kw):
    """(inputs, restatement of the assignment flavour), computed once and shared."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        inputs = getattr(zc, name)(**kw)
        L, AD, IDs, A = inputs[:4]
        _cache[key] = (inputs, zscore_cpu.assignment(L, AD, IDs, np.unique(IDs[:, 1]), A))
    return _cache[key]


def kept_depths(r):
    return sorted(set(int(d) for d in r["AD_array"][:, 2]))


def classes_of(AD, i):
    return zc.class_index(AD[:, 2 * i].astype(np.int64), AD[:, 2 * i + 1].astype(np.int64))


def every_class_claims(L, AD, IDs, A, placed, want, thr=0):
    """The conditions of every_class; AssertionError where one does not hold."""
    assert L.shape[0] % 64 and (L.shape[0] + 63) // 64 == 66 and L.shape[0] > 4097
    for i in zc.FULL:
        r = want[i]
        assert len(r["keys"]) == 253 and r["counts"].min() >= 6
        assert kept_depths(r) == list(range(1, 22)), "kept depths of individual %d" % i
        assert r["index"].shape == (22, 22)
        k = classes_of(AD, i)
        for lo, hi in ((0, 64), (64, 128), (128, 192), (192, 253)):
            sites = np.flatnonzero((k >= lo) & (k < hi) & (k > 0))
            kept = int(np.isin(sites, r["keep"]).sum())
            assert len(sites) // 2 <= kept < len(sites), (i, lo, hi, kept, len(sites))
        _, _, _, fwd = zscore_cpu.depth_classes(L, AD, i)
        keys_rev, _, _, rev = zscore_cpu.depth_classes(L[::-1], AD[::-1], i)
        rev_of = {tuple(a): b.tobytes() for a, b in zip(keys_rev, rev)}
        assert sum(rev_of[tuple(a)] != b.tobytes() for a, b in zip(r["keys"], fwd)) >= 100, "float32 sums that depend on the site order"
        for name in ("wobs", "wl", "var"):
            assert np.isfinite(r[name]).all(), name
        assert np.isfinite(r["z"])
    for i in (0, 3):
        assert max(kept_depths(want[i])) <= 10 and classes_of(AD, i).max() < 128


def test_every_class_is_what_it_claims():
    (L, AD, IDs, A, placed), want = classes_case()
    every_class_claims(L, AD, IDs, A, placed, want)
    assert IDs[1, 1] != IDs[2, 1] and 1 // 2 != 2 // 2            # one in each population; batches of 2 part them, batches of 3 do not


def test_every_class_placements():
    """What fixed_places says: a class of each wavefront at lanes 0 and 63 of one of the first four tiles (the first site of the first
    tile holds wavefront 0's class in one individual and wavefront 2's in the other), classes >= 64 at the sites 4095 and 4096,
    classes of depth 21 at the first and the last site of the last, partial tile."""
    (L, AD, IDs, A, placed), _ = classes_case()
    m = L.shape[0]
    assert sorted(placed) == list(zc.FULL)
    assert [k >> 6 for k in zc.WAVE_CLASSES] == [0, 1, 2, 3]
    for q, i in enumerate(zc.FULL):
        k = classes_of(AD, i)
        for site, cls in placed[i].items():
            assert k[site] == cls
        for w, cls in enumerate(zc.WAVE_CLASSES):
            t = (w + 2 * q) % 4
            assert k[64 * t] == cls and k[64 * t + 63] == cls
        assert k[0] == zc.WAVE_CLASSES[(4 - 2 * q) % 4] and np.flatnonzero(k == k[0])[0] == 0
        assert k[4095] >= 64 and k[4096] >= 64
        last = (m - 1) // 64 * 64
        assert last > 4096 and m - last < 64 and zc.D_OF[k[last]] == 21 and zc.D_OF[k[m - 1]] == 21


def test_a_claim_can_fail():
    """The conditions are not vacuous: four sites per class with a threshold of 5 miss them (depths go), and so does the incomplete
    variant."""
    (inputs, want) = classes_case(per_class=4)
    with pytest.raises(AssertionError):
        every_class_claims(*inputs, want)
    L, AD, IDs, A, placed = inputs
    thin = zscore_cpu.assignment(L, AD, IDs, np.unique(IDs[:, 1]), A, 5)
    assert max(kept_depths(thin[1])) < 21
    (inputs, want) = classes_case("incomplete_21")
    with pytest.raises(AssertionError):
        every_class_claims(*inputs, want)


def test_incomplete_21():
    (L, AD, IDs, A, _), want = classes_case("incomplete_21")
    assert kept_depths(want[1]) == list(range(1, 21)) and kept_depths(want[2]) == list(range(1, 22))
    assert len(want[1]["keys"]) == 252 and want[1]["index"].shape[0] <= 21
    at21 = np.flatnonzero(AD[:, 2] + AD[:, 3] == 21)
    assert len(at21) == 22 * 6 and not np.isin(at21, want[1]["keep"]).any()


def test_edge_of_dense():
    L, AD, IDs, A, claims = zc.edge_of_dense()
    dl = AD[:, 0::2] + AD[:, 1::2]
    assert [int((dl[:, i] > 21).sum()) for i in range(4)] == [0, 0, claims["over"], 0] and claims["over"] == 42
    k = np.where(dl[:, zc.EDGE_IND] <= 21, classes_of(AD, zc.EDGE_IND), -1)
    assert sorted(claims["counts"]) == [231, 242, 252]
    for cls, n in claims["counts"].items():
        assert (k == cls).sum() == n > 0
    pairs = {tuple(p) for p in AD[dl[:, zc.EDGE_IND] > 21][:, 2 * zc.EDGE_IND:2 * zc.EDGE_IND + 2]}
    assert pairs == set(zc.EDGE_OVER) and {(22, 0), (0, 22), (11, 11), (255, 255)} <= pairs
    over = np.flatnonzero(dl[:, zc.EDGE_IND] > 21)
    assert (dl[over - 1, zc.EDGE_IND] == 21).all()                  # every deep site follows a site of the last dense depth
    assert {63, 64} <= set(over) | set(over - 1) and over.max() >= 128


def test_threshold_sites():
    t = zc.threshold_sites()
    L, expect = t["L"], t["expect"]
    assert L.shape[0] == 182 and len(t["groups"]) == 24
    ties = 0
    for cls, mean, c, sites in t["groups"]:
        g0, g1 = L[sites, 0], L[sites, 1]
        v = (g0, g1, (F32(1) - g0) - g1)[c]
        assert len(set(v.tolist())) == 7 and np.all(np.diff(v.view(np.int32)) == 1)          # seven neighbouring float32
        want = ~(np.abs(mean - v) > F32(0.01))
        assert np.array_equal(expect[sites, 0], want) and np.array_equal(expect[sites, 1], want)
        assert want.sum() == 4 and (~want).sum() == 3
        assert want[3] and (not want[0] or not want[6])                                       # the edge lies inside the group
        if mean == F32(0.02):
            ties += int((np.abs(mean - v) == F32(0.01)).sum())
    assert ties >= 1, "no site exactly on the threshold"
    assert np.isnan(t["key_mean"]).sum() == 2 and expect[t["nan_sites"]].all() and not expect[t["dropped_sites"]].any()
    for i in range(2):
        used = np.unique(classes_of(t["AD"], i))
        assert sorted(used) == sorted(zc.THRESHOLD_CLASSES) and (used >= 64).sum() >= 7 and {0, 1, 2, 3} == {int(k) >> 6 for k in used}
        assert (t["key_comp"][i, used] >= 0).sum() == 13
    assert not np.array_equal(t["AD"][:, 0:2], t["AD"][:, 2:4])


def test_scan_shapes():
    shapes = zc.scan_shapes()
    assert sorted((m + 63) // 64 for m, _, _ in shapes) == [1, 2, 255, 256, 257, 257, 511, 512, 513]
    assert max(m for m, _, _ in shapes) == 32832 and 256 * 64 + 1 in [m for m, _, _ in shapes]
    seen = set()
    for m, names, keep in shapes:
        assert keep.shape == (m, 3) and len(set(names)) == 3
        seen |= set(names)
        for nm, col in zip(names, keep.T):
            want = dict(all=m, none=0, last=1, lane0=(m + 63) // 64, half=m // 2)[nm]
            assert col.sum() == want
        L, AD, key_mean, key_comp = zc.scan_inputs(m, keep)
        near = ~(np.abs(F32(0.5) - L[:, 0::2]) > F32(0.01))
        assert np.array_equal(near, keep) and not AD.any()
        assert len(np.unique(L[:, 0::2])) == 3 * m
        with np.errstate(divide="ignore"):
            assert len(np.unique(zscore_cpu._logf(L[:, 0::2][keep]))) == keep.sum()
    assert seen == set(zc.SCAN_PATTERNS)


def test_log_arguments():
    parts = zc.log_arguments()
    assert {k: len(v) for k, v in parts.items()} == dict(quarter=1 << 23, half=1 << 23, one=1 << 23, stride=261089, edges=384, specials=5)
    for name, bits in parts.items():
        assert bits.dtype == np.uint32 and len(np.unique(bits)) == len(bits), name
        assert bits.max() < 0x7F800000, name                      # sign bit clear, finite
    for name, lo in (("quarter", 0.25), ("half", 0.5), ("one", 1.0)):
        x = parts[name].view(F32)
        assert x[0] == F32(lo) and x[-1] < F32(2 * lo) and parts[name][-1] + 1 == F32(2 * lo).view(np.uint32)
    edges = parts["edges"].reshape(128, 3)
    iv = zc.log_interval(edges)
    assert np.all(iv[:, 1] == iv[:, 2]) and np.all(iv[:, 0] != iv[:, 1])
    assert edges[0, 1] == F32(0.6875).view(np.uint32) and edges.view(F32).max() < F32(1.375)
    assert sorted(set(iv[:, 1] & 127)) == list(range(128))
    x = parts["specials"].view(F32)
    assert list(parts["specials"]) == [0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF]
    assert x[0] == 0 and x[1] == np.finfo(F32).smallest_subnormal and x[3] == np.finfo(F32).tiny and x[4] == np.finfo(F32).max


def test_the_cut_of_the_sharded_case():
    """tests/zscore_shard_worker.py, case `classes`: among the classes >= 64 of individual 1 some have all their sites before the cut,
    some all behind it and some on both sides, and the cut lies inside a tile."""
    import zscore_shard_worker as worker
    (L, AD, IDs, A), cuts, _ = worker.jobs("classes", 2, 64)[0]
    assert cuts == [zc.CLASSES_CUT] and cuts[0] % 64
    before, after, both = zc.sides_of_cut(AD, 1, cuts[0])
    assert len(before) >= 1 and len(after) >= 1 and len(both) >= 100
    assert len(before) + len(after) + len(both) == 253 - 64


# ---------------------------------------------------------------- the record from the real reference
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "zscore_classes.npz"), allow_pickle=False)


_inputs = []


def recorded_inputs(gold):
    if not _inputs:
        L, AD, IDs, A, placed = zc.every_class(**ast.literal_eval(str(gold["case_classes_gen"])))
        assert synth_depth.digest(L, AD, A) == str(gold["case_classes_digest"]), "the generator no longer reproduces the recorded inputs"
        _inputs.append((L, AD, IDs, A))
    return _inputs[0]


def test_restatement_reproduces_every_recorded_array(gold, oracle):
    L, AD, IDs, A = recorded_inputs(gold)
    pops = np.unique(IDs[:, 1])
    seen = 0
    for r, spec in runs(gold):
        if spec["flavour"] == "assignment":
            res = zscore_cpu.assignment(L, AD, IDs, pops, A, spec["thr"], spec["srt"], spec["ind_start"], spec["ind_end"])
        else:
            res = zscore_cpu.reference(L, AD, IDs, lambda Lp, it, tol: oracle.emMAF(Lp, it, tol, 2), 200, 1e-4, spec["thr"], spec["srt"],
                                       spec["ind_start"], spec["ind_end"])
        lines = []
        for j, one in enumerate(res):
            compare_individual(gold, r, j, one, one["extra"] if spec["flavour"] == "reference" else None)
            lines += zscore_cpu.stdout_lines(j, one)
            seen += 1
        assert lines == str(gold["run%d_stdout" % r]).splitlines()[:-1], "stdout lines of run %d" % r
        assert zscore_cpu.file_text([one["z"] for one in res]) == str(gold["run%d_file" % r])
    assert seen == 8


def test_recorded_case_keeps_every_depth(gold):
    L, AD, IDs, A = recorded_inputs(gold)
    for r in (0, 1):
        for i in zc.FULL:
            arr = gold["run%d_i%d_AD_array" % (r, i)]
            assert sorted(set(arr[:, 2])) == list(range(1, 22)) and arr.shape[0] == 252
            assert gold["run%d_i%d_index" % (r, i)].shape == (22, 22) and len(gold["run%d_i%d_keys" % (r, i)]) == 253
            at = np.flatnonzero(AD[:, 2 * i] + AD[:, 2 * i + 1] >= 11)
            kept = np.isin(at, gold["run%d_i%d_keep" % (r, i)]).sum()
            assert len(at) // 2 <= kept < len(at)
        assert gold["run%d_i0_index" % r].shape[0] < 12
