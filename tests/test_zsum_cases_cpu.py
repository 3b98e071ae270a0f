"""CPU-only: the Python twin of np.sum's float32 order (tests/zsum_cases.py) is the INSTALLED NumPy's order bit for bit, the
state machine the device runs (full chunks as they come, the ragged chunk at the end) is that order under every cut into pushes the
GPU test uses, and the inputs tell the order from the plausible wrong ones."""
import numpy as np
import pytest

import zsum_cases as zc


def test_the_twin_is_np_sum_on_every_length():
    for n in zc.CPU_LENGTHS:
        a = zc.values(n, 1)
        want = np.sum(a)
        assert want.dtype == np.float32
        assert zc.same(zc.numpy_order(a), want), n
        assert zc.same(np.sum(a, dtype=np.float32), want), n
        if n:                                              # a view offset by one element: another alignment, the same order
            b = zc.values(n + 1, 2)[1:]
            assert zc.same(zc.numpy_order(b), np.sum(b)), n


def test_a_full_chunk_is_the_tree_over_64_leaves():
    for seed in range(4):
        a = zc.values(zc.CHUNK, seed)
        assert zc.same(zc.full_chunk(a), zc.pairwise(a))
        assert zc.same(np.float32(0.0) + zc.full_chunk(a), np.sum(a))


@pytest.mark.parametrize("how", zc.CUTS)
def test_the_continued_sum_is_np_sum_under_every_cut(how):
    lengths = sorted(set(zc.GPU_LENGTHS) | {1000, 4097, 100003})
    for n in lengths:
        a = zc.values(n, 3)
        st = zc.Continued()
        for p in zc.pieces(a, how):
            st.push(p)
        assert st.tail.size == n % zc.CHUNK
        assert zc.same(st.finish(), np.sum(a)), (how, n)
        assert zc.same(zc.close(st.run, st.tail), np.sum(a)), (how, n)      # the host's route: run + np.sum(tail)


@pytest.mark.parametrize("how", zc.CUTS)
def test_the_specials(how):
    for name, a in zc.specials().items():
        st = zc.Continued()
        for p in zc.pieces(a, how):
            st.push(p)
        with np.errstate(invalid="ignore", over="ignore"):
            want = np.sum(a)
        assert zc.same(zc.close(st.run, st.tail), want), (name, how)
    with np.errstate(invalid="ignore"):
        s = zc.specials()
        assert np.isnan(np.sum(s["nan"])) and np.isnan(np.sum(s["inf-inf"]))
        assert np.sum(s["+inf"]) == np.inf and np.sum(s["-inf"]) == -np.inf
        for name in ("-0.0", "-0.0 short", "cancel"):
            assert np.sum(s[name]).tobytes() == np.float32(0.0).tobytes(), name     # +0.0, not -0.0


def test_the_running_value_is_never_minus_zero():
    """Why run + np.sum(tail) is exact: a float32 that started at +0.0 and only took additions is -0.0 never."""
    st = zc.Continued()
    st.push(np.full(2 * zc.CHUNK, -0.0, dtype=np.float32))
    assert st.run.tobytes() == np.float32(0.0).tobytes()


def test_the_inputs_tell_the_orders_apart():
    """At least half of the finite cases longer than 8192 differ from each wrong order -- and np.sum itself says so."""
    assert sorted(zc.ORDER_SEEDS) == sorted(set(n for n in zc.CPU_LENGTHS + zc.GPU_LENGTHS if n > zc.CHUNK))
    cases = [zc.values(n, seed) for n, seeds in zc.ORDER_SEEDS.items() for seed in seeds]
    assert len(cases) >= 14 and all(np.isfinite(a).all() for a in cases)
    for name, wrong in zc.WRONG_ORDERS.items():
        differ = sum(not zc.same(wrong(a), np.sum(a)) for a in cases)
        assert 2 * differ >= len(cases), (name, differ, len(cases))


def test_groups_and_pushes():
    groups = zc.groups()
    assert sorted(n for g in groups for n in g) == sorted(zc.GPU_LENGTHS)
    for lengths in groups:
        assert len(set(lengths)) == zc.GROUP
        arrays = zc.group_arrays(lengths)
        for how in zc.CUTS:
            ps = zc.pushes_of(arrays, how)
            for j, n in enumerate(lengths):
                assert sum(int(k[j]) for k, _ in ps) == n
            back = np.concatenate([h[1, int(k[:4].sum()):int(k[:5].sum())] for k, h in ps])     # array 1 of the last individual
            assert back.tobytes() == arrays[4][1].tobytes()
    assert zc.cut(zc.CHUNK + 5, "8191+1") == [8191, 1, 5] and zc.cut(0, "1000") == [0] and zc.cut(3, "empty") == [1, 0, 2]
