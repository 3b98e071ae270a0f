"""tests/order_cases.py held to its own claims, without a GPU: every block's float64 sum is exact in any order (in integers), every
(individual, population, block) is of the magnitude class claimed, numpy_order of the exact block sums IS np.sum(vec, dtype=float) of
the oracle's vector in every cell of every shape, and every wrong order a plausible bug would produce differs from np.sum in at least
MIN_DIFFERENT cells wherever it can differ at all -- so tests/test_gpu_order_cases.py, which holds the device to np.sum on these
inputs, would notice each of them.  These are conditions on the inputs, computed here from the twins alone; nothing is taken from the
device.  (That NumPy adds in chunks of 8192 sites is pinned by test_installed_numpy_sums_float32_in_8192_element_chunks.)"""
import numpy as np
import pytest

import order_cases as oc


@pytest.fixture(scope="module")
def shapes(oracle):
    """shape -> (Values, exact block sums (blocks, n, K_ALL), np.sum of every cell (n, K_ALL)); once, shared, read-only."""
    out = {}
    for shape in oc.SHAPES:
        vals = oc.reference(oracle, shape)
        S = oc.block_sums(vals)
        S.setflags(write=False)
        out[shape] = (vals, S, oc.expected(vals))
    return out


def test_the_shapes_take_every_exit_of_the_prefix_loops():
    """block_prefix_kernel: 8 blocks at a time, then pairs, then a single block -- no, one and two rounds of the unrolled loop, each
    with no tail, a single block, a pair, and pairs and a single block behind it."""
    exits = {(b // 8, (b % 8) // 2 > 0, b % 2) for b in oc.NBLOCKS}
    assert exits >= {(0, False, 1), (0, True, 0), (0, True, 1), (1, False, 0), (1, False, 1), (1, True, 0), (1, True, 1), (2, False, 0), (2, False, 1)}
    assert max(oc.sites_of(s) for s in oc.SHAPES) == 17 * 4096 == 69632
    for b in oc.NBLOCKS:
        full, ragged, single = (oc.sites_of((b, t)) for t in oc.TAILS)
        assert full == b * 4096 and single == (b - 1) * 4096 + 1 and (b - 1) * 4096 < ragged < full
        assert ragged % 64 not in (0, 1) and (ragged - (b - 1) * 4096) // 64 >= 1          # a full tile and a ragged one in the last block
    c = oc.case()
    n = len(c["labels"])
    assert 20 <= n <= 30 and c["sizes"] == (1, 2, 5, 8, 9) and sorted(np.bincount(c["labels"])) == [1, 2, 5, 8, 9]
    assert set(np.unique(c["L"])) == {0.0, 1.0}
    assert len(set(oc.PATTERNS)) == n
    for bits in range(1, 15):                                # every mixed big/small pattern of two chunks; its shifts are patterns too
        p = "".join("B" if bits >> j & 1 else "S" for j in range(4))
        assert p in oc.PATTERNS and p[1:] + p[:1] in oc.PATTERNS and p[2:] + p[:2] in oc.PATTERNS
    assert {"".join(c["letters"][i]).find("B") for i in range(n) if "".join(c["letters"][i]).count("B") == 1} == {0, 6, 8, 9, 16}
    # low bits that differ from site to site: thousands of frequencies per block at a population next to 0, all there are next to 1
    A = c["A"]
    for k, (kind, e) in enumerate(oc.FAMILIES):
        distinct = len(np.unique(A[:4096, k]))
        assert distinct > 3000 if kind == "low" else distinct == 2 ** (24 - e) + 1, (k, distinct)


def test_every_block_sum_is_exact_in_any_order(shapes):
    """In integers: the terms of a block are multiples of 2^g and their magnitudes sum to less than 2^(g + 53).  The same for the last
    chunk as a whole where a partial block closes it (order_cases: THE LAST CHUNK)."""
    worst = 0
    for shape, (vals, _, _) in shapes.items():
        for b in range(shape[0]):
            worst = max(worst, int(oc.exact_margin(vals.block(b)).max()))
        if oc.closes_a_chunk(shape):
            chunk = np.concatenate((vals.block(shape[0] - 2), vals.block(shape[0] - 1)), axis=-1)
            worst = max(worst, int(oc.exact_margin(chunk).max()))
    print("largest sum of |v| / 2^g over the blocks: 2^%.1f" % np.log2(worst))
    assert worst < 2 ** 53


def test_every_block_is_of_the_class_claimed(shapes):
    counts = dict.fromkeys(oc.CLASSES, 0)
    for shape, (vals, _, _) in shapes.items():
        if shape != (oc.MAX_BLOCKS, "full") and not oc.closes_a_chunk(shape):
            continue                                         # (a prefix of the largest shape)
        for b in range(shape[0]) if shape[1] == "full" else (shape[0] - 1,):
            mag = np.abs(vals.block(b))
            lo_, hi_ = mag.min(axis=-1), mag.max(axis=-1)
            for i in range(vals.n):
                for k in range(vals.K):
                    cls = oc.claimed_class(i, k, b, shape)
                    lo, hi = oc.CLASS_RANGE[cls]
                    assert lo <= lo_[i, k] and hi_[i, k] < hi, (shape, i, k, b, cls, lo_[i, k], hi_[i, k])
                    counts[cls] += 1
    print("(cell, block)s per class: %r" % counts)
    assert all(c > 500 for c in counts.values())


def test_numpy_order_of_the_block_sums_is_np_sum_in_every_cell(shapes):
    cells = 0
    for shape, (vals, S, want) in shapes.items():
        assert want.shape == (vals.n, oc.K_ALL) and np.isfinite(want).all()
        assert oc.different_cells(oc.numpy_order(S), want) == 0, shape
        C = oc.chunk_sums(S)
        assert len(C) == (shape[0] + 1) // 2
        run = np.zeros_like(want)
        for c in C:
            run = run + c
        assert oc.different_cells(run, want) == 0, shape
        # ... and cut at any chunk edges and continued, as the shards and the windows do
        for cuts in [(c,) for c in range(2, shape[0], 2)] + [oc.SHARD_CUTS, (2, 12)]:
            assert oc.different_cells(oc.continued_order(S, cuts), want) == 0, (shape, cuts)
        cells += want.size
    print("%d cells over %d shapes" % (cells, len(shapes)))


@pytest.mark.parametrize("order", list(oc.WRONG_ORDERS))
def test_a_wrong_order_shows_wherever_it_can(shapes, order):
    """... in at least MIN_DIFFERENT cells of the first 6 populations and of all 13, at every shape but those where it is NumPy's order
    whatever the data (order_cases.cannot_differ) -- and there in none."""
    f, least = oc.WRONG_ORDERS[order], {}
    applies = 0
    for shape, (vals, S, want) in shapes.items():
        diff = np.ascontiguousarray(f(S)).view(np.uint64) != want.view(np.uint64)
        if oc.cannot_differ(order, shape[0]):
            assert not diff.any(), (order, shape)
            continue
        applies += 1
        for K in oc.K_TESTED:
            d = int(diff[:, :K].sum())
            least[K] = min(least.get(K, (d, shape)), (d, shape))
            assert d >= oc.MIN_DIFFERENT, (order, shape, K, d)
    print("%s: applies to %d of %d shapes; fewest differing cells %r" % (order, applies, len(shapes), least))
    assert applies >= 5


def test_shard_totals_added_show_at_every_cut_of_the_shard_test(shapes):
    """The cuts tests/test_gpu_order_cases.py makes on one device: the shards' own sums added differ from np.sum in at least
    MIN_DIFFERENT cells wherever a later shard holds a block beyond its first chunk, and in none elsewhere."""
    for shape in oc.SHARD_SHAPES:
        _, S, want = shapes[shape]
        cuts_of = oc.shard_cuts(shape)
        assert len(cuts_of) >= (shape[0] + 1) // 2
        for cuts in cuts_of:
            d = oc.different_cells(oc.shard_totals_added(S, cuts), want)
            print(shape, cuts, d)
            assert d >= oc.MIN_DIFFERENT if oc.shards_can_differ(shape, cuts) else d == 0, (shape, cuts, d)


def test_orders_that_can_never_show(shapes):
    """A restart at every 8192 sites is total + chunk either way; a carry added last is the shard totals added (a + b = b + a)."""
    assert len(oc.NEVER_DIFFERENT) == 2
    for shape, (_, S, want) in shapes.items():
        assert oc.different_cells(oc.restart_order(S, 8192), want) == 0
        assert oc.different_cells(oc.carry_last_order(S, oc.SHARD_CUTS), oc.shard_totals_added(S, oc.SHARD_CUTS)) == 0
        assert oc.different_cells(oc.pair_split_order(S, "all"), oc.plain_order(S)) == 0


def test_a_mixed_last_chunk_is_not_its_block_sums(oracle):
    """Why a partial block that closes a chunk holds its neighbour's pairs (order_cases: THE LAST CHUNK): left as the prefix of the
    largest case, a full block and a ragged one of another class, np.sum itself -- which splits the short chunk inside its first
    block -- is not S[0] + S[1] in a dozen cells, although both block sums are exact."""
    shape = (2, "ragged")
    V = oc.reference(oracle, shape).V
    m = oc.sites_of(shape)
    n, K = V.shape[:2]
    mixed = same = 0
    for i in range(n):
        for k in range(K):
            vec = np.array(V[i, k, :m], dtype=np.float32)
            blocks = vec[:4096].astype(np.float64).sum() + vec[4096:].astype(np.float64).sum()
            if oc.pattern_class(i, 0) == oc.pattern_class(i, 1):
                assert np.sum(vec, dtype=float) == blocks
                same += 1
            else:
                mixed += np.sum(vec, dtype=float) != blocks
    print("cells of one class %d; cells of two classes where np.sum is not S[0] + S[1]: %d" % (same, mixed))
    assert same >= 50 and mixed >= oc.MIN_DIFFERENT


def test_the_text_form_parses_back():
    shape = (3, "ragged")
    L, _ = oc.matrix_of(shape)
    text = oc.beagle_text(L)
    lines = text.split(b"\n")
    assert len(lines) == L.shape[0] + 2 and lines[-1] == b"" and lines[1].startswith(b"chr1_1\tA\tC\t")
    fields = lines[-2].split(b"\t")
    assert len(fields) == 3 + 3 * (L.shape[1] // 2) and set(fields[3:]) == {b"0.000000", b"1.000000"}
    back = oc.parse_text(text)
    assert back.dtype == L.dtype and back.shape == L.shape and back.tobytes() == L.tobytes()
    third = np.array([float(t) for t in fields[3:]]).reshape(-1, 3)
    assert (third.sum(axis=1) == 1).all()
