"""GPU: the window-to-window float32 sums (csrc/zscore_kernels.hip: zsum_chunk_kernel, zsum_close_kernel, through the test hook
wgs_debug_zsum_push) held to np.sum of the installed NumPy, bit for bit and NaN for NaN, on the enumerated lengths and cuts of
tests/zsum_cases.py: five individuals of DIFFERENT lengths in one state, three arrays each, every cut into pushes.  The references are
np.sum itself, computed once per group and shared."""
import numpy as np
import pytest

import zsum_cases as zc

pytestmark = pytest.mark.gpu

_groups = {}


def group(g):
    """(lengths, arrays, want (5, 3) float32) of a group: made once, shared, read-only."""
    if g not in _groups:
        lengths = zc.groups()[g]
        arrays = zc.group_arrays(lengths)
        want = np.array([[np.sum(a) for a in arr] for arr in arrays], dtype=np.float32)
        for arr in arrays:
            for a in arr:
                a.setflags(write=False)
        want.setflags(write=False)
        _groups[g] = (lengths, arrays, want)
    return _groups[g]


def run(arrays, how):
    from wgsassign_amd import zscore
    zs = zscore.ZSum(len(arrays))
    try:
        for kept, host in zc.pushes_of(arrays, how):
            zs.push_host(host, kept)
        totals, run_, tails = zs.state()
        _, sums = zs.finish()
    finally:
        zs.close()
    return totals, run_, tails, sums


@pytest.mark.parametrize("how", zc.CUTS)
@pytest.mark.parametrize("g", range(len(zc.groups())))
def test_sums_are_np_sum(g, how):
    lengths, arrays, want = group(g)
    totals, run_, tails, sums = run(arrays, how)
    assert list(totals) == list(lengths)
    for j, n in enumerate(lengths):
        for a in range(3):
            assert zc.same(sums[j, a], want[j, a]), (n, a, how, sums[j, a], want[j, a])
            # the state itself: the open chunk holds the last n % 8192 elements, the running value the chunks before them
            assert tails[j][a].tobytes() == arrays[j][a][n - n % zc.CHUNK:].tobytes(), (n, a, how)
            assert zc.same(run_[j, a], zc.numpy_order(arrays[j][a][:n - n % zc.CHUNK])), (n, a, how)


def test_the_long_arrays_tell_the_orders_apart():
    """The arrays the device was just held to are those on which np.sum differs from every wrong order (tests/zsum_cases.py)."""
    told = {name: 0 for name in zc.WRONG_ORDERS}
    for g in range(len(zc.groups())):
        lengths, arrays, want = group(g)
        for j, n in enumerate(lengths):
            if n > zc.CHUNK and n != 2 * zc.CHUNK:
                for name, wrong in zc.WRONG_ORDERS.items():
                    told[name] += sum(not zc.same(wrong(arrays[j][a]), want[j, a]) for a in range(2))
    assert all(v >= 8 for v in told.values()), told


@pytest.mark.parametrize("how", zc.CUTS)
def test_specials(how):
    s = zc.specials()
    names = sorted(s)
    for lo in range(0, len(names), zc.GROUP):
        part = names[lo:lo + zc.GROUP]
        arrays = [[s[name]] * 3 for name in part]
        _, _, _, sums = run(arrays, how)
        for j, name in enumerate(part):
            with np.errstate(invalid="ignore", over="ignore"):
                want = np.sum(s[name])
            for a in range(3):
                assert zc.same(sums[j, a], want), (name, how, sums[j, a], want)


def test_refusals():
    from wgsassign_amd import zscore
    zs = zscore.ZSum(2)
    try:
        with pytest.raises(ValueError, match="add up"):
            zs.push_host(np.zeros((3, 5), dtype=np.float32), np.array([2, 2]))
        assert list(zs.totals()) == [0, 0]
        totals, sums = zs.finish()                              # N = 0: +0.0
        assert sums.tobytes() == np.zeros((2, 3), dtype=np.float32).tobytes()
    finally:
        zs.close()
    with pytest.raises(ValueError, match="between 1 and"):
        zscore.ZSum(0)
