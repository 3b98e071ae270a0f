"""CPU-only: the host side of the z-scores over SNP shards.  The product merges the dense tier of the shards in C
(wgs_zscore_classes_sharded: counts added, the smallest global first site, sums handed from shard to shard), which needs a GPU and
is covered by tests/test_gpu_zscore_sharded.py.  Here that merge is restated by NumPy from the inputs of
tests/golden/zscore_deep.npz, cut at three places, only to FEED the product's Python side: concat_deep (the shards' deep-site
lists, as they travel between the ranks) and dictionaries (deep_classes / merge_tiers / key_filter on global first sites).  Their
result must be the dictionary tests/zscore_cpu.py gives for the whole table, which the records from the real reference pin.  And the
command line no longer refuses the two options with several ranks, but does refuse a communicator the library cannot use."""
import os

import numpy as np
import pytest

import zscore_cpu
from conftest import GOLDEN
from test_zscore_cpu import same
from test_zscore_deep_cpu import deep_inputs

N_CLASSES, MAX_DENSE = 253, 21


@pytest.fixture(scope="module")
def inputs():
    return deep_inputs(np.load(os.path.join(GOLDEN, "zscore_deep.npz"), allow_pickle=False))


def shard_tables(L, AD, i, lo, hi, carry):
    """What one rank's class sweep and deep-site list give for individual i over sites [lo, hi): counts, first sites (global, -1: none),
    the sums continued from `carry`, and (sites, ad, g) of the sites deeper than 21 reads."""
    Ar, Aa = AD[lo:hi, 2 * i].astype(np.int64), AD[lo:hi, 2 * i + 1].astype(np.int64)
    d = Ar + Aa
    T = np.stack(zscore_cpu.triple(L[lo:hi], i), axis=1)
    cnt = np.zeros(N_CLASSES, dtype=np.int32)
    first = np.full(N_CLASSES, -1, dtype=np.int64)
    sums = carry.copy()
    cls = np.where(d <= MAX_DENSE, d * (d + 1) // 2 + Aa, -1)
    for k in np.unique(cls[cls >= 0]):
        at = np.flatnonzero(cls == k)
        cnt[k] = len(at)
        first[k] = lo + at[0]
        sums[k] = np.cumsum(np.concatenate((sums[k][None], T[at])), axis=0, dtype=np.float32)[-1]       # the chain goes on
    over = np.flatnonzero(cls < 0)
    return cnt, first, sums, (over + lo, np.stack((Ar[over], Aa[over]), axis=1).astype(np.int32),
                              np.ascontiguousarray(L[lo:hi][over][:, 2 * i:2 * i + 2]))


@pytest.mark.parametrize("cuts", [(750,), (63, 64), (1, 700, 1499)])
def test_merged_dictionary_of_the_shards_is_the_whole_table_s(inputs, cuts):
    from wgsassign_amd import zscore
    L, AD, IDs, A, deep = inputs
    m, n = L.shape[0], L.shape[1] // 2
    bounds = (0,) + cuts + (m,)
    cnt = np.zeros((n, N_CLASSES), dtype=np.int32)
    first = np.full((n, N_CLASSES), -1, dtype=np.int64)
    sums = np.zeros((n, N_CLASSES, 3), dtype=np.float32)
    over = np.zeros(n, dtype=np.int64)
    listed = []
    for i in range(n):
        parts = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            c, f, sums[i], lst = shard_tables(L, AD, i, lo, hi, sums[i])
            cnt[i] += c                                                        # counts add
            first[i] = np.where(first[i] < 0, f, np.where(f < 0, first[i], np.minimum(first[i], f)))      # the smallest, -1: none
            parts.append([x.tolist() for x in lst])                            # (as the lists travel between the ranks)
            over[i] += len(lst[0])
        listed.append(zscore.concat_deep(parts))
        assert np.array_equal(listed[i][0], deep[i])
    assert over.max() > 0 and (first[cnt > 0] >= 0).all() and (first[cnt == 0] == -1).all()
    assert any((first[i][cnt[i] > 0] >= cuts[0]).any() for i in range(n)), "no class is first seen behind the first cut"
    for thr, srt in ((0, False), (3, False), (0, True)):
        got = zscore.dictionaries(0, cnt, first, sums, over, listed, thr, srt, True)
        for i in range(n):
            keys, counts, means, _ = zscore_cpu.depth_classes(L, AD, i)
            same(got[i]["keys"], keys, "keys of individual %d" % i)
            same(got[i]["counts"], counts, "counts")
            same(got[i]["means"], means, "means")
            same(got[i]["AD_array"], zscore_cpu.key_filter(keys, counts, thr, srt), "AD_array")
    with pytest.raises(ValueError, match="deeper than 21"):
        zscore.dictionaries(0, cnt, first, sums, over, listed, 0, False, False)


def test_z_score_options_are_not_refused_with_several_ranks(tmp_path, monkeypatch):
    """Before anything touches a device: `--gpus 2` starts the ranks (the launcher is replaced), and a rank of two gets past the
    place where the options used to be refused."""
    from wgsassign_amd import WGSassign, comm
    started = []
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(comm, "launch_local_ranks", lambda n, argv, **kw: started.append((n, argv)) or 0)
    ad = tmp_path / "ad.txt"
    ad.write_text("1 0\n")
    for flag in ("--get_assignment_z_score", "--get_reference_z_score"):
        argv = [flag, "--gpus", "2", "--ind_ad_file", str(ad), "--out", str(tmp_path / "x")]
        with pytest.raises(SystemExit) as e:
            WGSassign.main(argv)
        assert e.value.code == 0 and "shard" not in str(e.value)
        assert started[-1][0] == 2 and flag in started[-1][1]

        class TwoRanks:
            rank, world, handle = 1, 2, 1
        monkeypatch.setattr(comm, "init_from_env", lambda: TwoRanks())
        monkeypatch.setenv("WORLD_SIZE", "2")
        assert WGSassign.main(argv) is None                  # (no --beagle: the options were checked and nothing else was asked for)
        monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("WORLD_SIZE", "2")

    class NoHandle:
        rank, world = 1, 2
    monkeypatch.setattr(comm, "init_from_env", lambda: NoHandle())
    with pytest.raises(SystemExit, match="need the library's own communicator"):    # e.g. torch.distributed over gloo
        WGSassign.main(["--get_assignment_z_score", "--ind_ad_file", str(ad), "--out", str(tmp_path / "x")])
    with pytest.raises(SystemExit, match="outside the scope"):                      # mixture proportions stay refused
        WGSassign.main(["--get_em_mix", "--out", str(tmp_path / "y")])
