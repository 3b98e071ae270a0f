"""The additions that turn the scoring sweeps' 4096-site block sums into the n x K float64 totals -- block_prefix_kernel,
chunk_total_kernel and combine_parts_kernel of csrc/assign_kernels.hip and their callers in csrc/score_api.hip -- held to the ORDER of
np.sum(vec, dtype=float) (glassy.py:38) where the order shows.  Every comparison is of bits, NaN equal to NaN; there is no tolerance.

The three kernels alone (wgs_debug_block_prefix, wgs_debug_chunk_total, wgs_debug_combine_parts: one launch of the product path's
launcher on host arrays) run on made-up float64 sums of which every addition rounds, with +-inf, NaN, -0.0 and sums that cancel among
them, against the Python loops of their own comments: 0 to 33 blocks, 1 to 513 cells, with and without kept prefixes, chunk sums
and a carry, 1 to 16 parts.

The sweeps, the shards and the windows run on the inputs of tests/order_cases.py, whose blocks are exact in any order and whose cells
are not: tests/test_order_cases_cpu.py shows, without a GPU, that NumPy's order of the exact block sums is np.sum in every cell and
that every wrong order a plausible bug would produce -- plain block order, a split pair, a window or a shard that restarts the
running total, a carry added last -- differs from it in at least eight cells of every shape at which it can differ at all.  The
yardstick is np.sum itself on the oracle's per-site vector, computed once per shape, shared and read-only."""
import ctypes
import gzip

import numpy as np
import pytest

import order_cases as oc

pytestmark = pytest.mark.gpu
F32 = np.float32
INF, NAN = float("inf"), float("nan")
compared = {}                     # what -> float64 results compared (printed by the last test)


@pytest.fixture(scope="module")
def dev():
    from wgsassign_amd import device
    device.get_context()
    return device


@pytest.fixture(autouse=True)
def _exact_mode(monkeypatch):
    for var in ("WGSASSIGN_MODE", "WGSASSIGN_PARTS", "WGS_SCORE_CODED_PARTS", "WGS_SCORE_CODED_TABLE", "WGSASSIGN_CODES_TABLE", "WGSASSIGN_WINDOW_SITES"):
        monkeypatch.delenv(var, raising=False)


def lib():
    return __import__("wgsassign_amd._lib", fromlist=["x"])


def equal_bits(got, want, what, kind):
    """Float64 arrays: the same bits, NaN for NaN; names the first element that differs and counts the others."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    compared[kind] = compared.get(kind, 0) + want.size
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        first = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d values differ, first at %r: device %r (%s), expected %r (%s)" % (
            what, int(bad.sum()), want.size, first, float(got[first]), float(got[first]).hex(), float(want[first]), float(want[first]).hex()))


# ---- the three kernels alone ------------------------------------------------------------------------------------------------------------
CELLS = (1, 255, 256, 257, 513)
SPECIALS = (INF, -INF, NAN, -0.0, 0.0)


def made_up(rows, cells, seed):
    """(rows, cells) float64 of which every addition rounds: full 53-bit mantissas, both signs, magnitudes 2^-30 .. 2^30 -- and, at a
    cell in eight, one of +inf, -inf, NaN, -0.0, 0.0 in one row, or a value and its negative in two rows (next to each other: one chunk;
    or three rows apart: the total cancels), so that an infinity meets its opposite and a NaN every position of the loops."""
    rng = np.random.default_rng(seed)
    S = np.ldexp(rng.uniform(1.0, 2.0, (rows, cells)) * rng.choice((-1.0, 1.0), (rows, cells)), rng.integers(-30, 31, (rows, cells)))
    for cell in range(seed % 8, cells, 8):
        if rows == 0:
            break
        kind, r = (cell // 8) % (len(SPECIALS) + 2), (cell // 8 * 5 + seed) % rows
        if kind < len(SPECIALS):
            S[r, cell] = SPECIALS[kind]
            if kind < 2 and cell % 16 < 8 and rows > 1:
                S[(r + 1 + cell % 3) % rows, cell] = -SPECIALS[kind]                  # inf - inf somewhere behind it
        else:
            other = (r + (1 if kind == len(SPECIALS) else 3)) % rows
            if other != r:
                S[other, cell] = -S[r, cell]
    return S


def prefix_loop(S, keep_prefix):
    """block_prefix_kernel's comment as a loop: (out, S afterwards, chunk sums)."""
    nblocks, cells = S.shape
    after, chunks = S.copy(), np.zeros(((nblocks + 1) // 2, cells))
    run = np.zeros(cells)
    with np.errstate(all="ignore"):
        for b in range(0, nblocks, 2):
            pair = b + 1 < nblocks
            if keep_prefix:
                after[b] = run
                if pair:
                    after[b + 1] = run + S[b]
            chunks[b // 2] = S[b] + S[b + 1] if pair else S[b]
            run = run + chunks[b // 2]
    return run, after, chunks


def run_block_prefix(ctx, S, keep_prefix, with_chunks):
    L = lib()
    nblocks, cells = S.shape
    S = np.ascontiguousarray(S.copy())
    out = np.full(cells, 12345.0)
    chunks = np.full(((nblocks + 1) // 2, cells), 12345.0) if with_chunks else None
    L.check(L.load().wgs_debug_block_prefix(ctx.handle, L.f64p(S) if nblocks else None, nblocks, cells, int(keep_prefix), L.f64p(out),
                                            L.f64p(chunks) if with_chunks else None))
    return out, S, chunks


@pytest.mark.parametrize("with_chunks", [False, True], ids=["chunks null", "chunks given"])
@pytest.mark.parametrize("keep_prefix", [0, 1])
@pytest.mark.parametrize("cells", CELLS)
def test_block_prefix_kernel_alone(dev, cells, keep_prefix, with_chunks):
    """0 to 33 blocks: no, one, two, three and four rounds of the unrolled loop, every tail behind each of them."""
    ctx = dev.get_context()
    for nblocks in range(34):
        S = made_up(nblocks, cells, 1000 * cells + nblocks)
        want_out, want_S, want_chunks = prefix_loop(S, keep_prefix)
        out, after, chunks = run_block_prefix(ctx, S, keep_prefix, with_chunks)
        what = "block_prefix_kernel, %d blocks x %d cells, keep_prefix %d" % (nblocks, cells, keep_prefix)
        equal_bits(out, want_out, what + ": out", "block_prefix_kernel")
        equal_bits(after, want_S, what + ": S afterwards", "block_prefix_kernel")
        if with_chunks:
            equal_bits(chunks, want_chunks, what + ": chunk sums", "block_prefix_kernel")


def test_the_made_up_sums_round_and_hold_every_special_value():
    """(Of the inputs above: what they are claimed to be.)"""
    S = made_up(33, 513, 7)
    out, _, chunks = prefix_loop(S, 0)
    finite = np.isfinite(S).all(axis=0)
    plain = np.zeros(513)
    with np.errstate(all="ignore"):
        for row in S:
            plain = plain + row
    assert (plain[finite] != out[finite]).sum() > 300                                    # the order shows in most finite cells
    assert np.isnan(out).sum() >= 10 and np.isposinf(out).any() and np.isneginf(out).any()
    assert ((S == 0) & np.signbit(S)).any() and (np.isposinf(S).any(axis=0) & np.isneginf(S).any(axis=0)).any()
    one = made_up(1, 513, 3)
    assert ((one == 0) & np.signbit(one)).any()                                          # -0.0 as the only block: out is 0.0 + -0.0
    cancel = [(S[r] == -S[r + 1]) & finite for r in range(32)]
    assert np.any(cancel)


@pytest.mark.parametrize("carried", [False, True], ids=["carry null", "carry given"])
@pytest.mark.parametrize("cells", CELLS)
def test_chunk_total_kernel_alone(dev, cells, carried):
    ctx, L = dev.get_context(), lib()
    for nchunks in range(18):
        C = made_up(nchunks, cells, 77 * cells + nchunks)
        carry = made_up(1, cells, 5 * cells + nchunks + 3)[0] * 2.0 ** 10 if carried else None
        want = np.zeros(cells) if carry is None else carry.copy()
        with np.errstate(all="ignore"):
            for c in C:
                want = want + c
        out = np.full(cells, 12345.0)
        L.check(L.load().wgs_debug_chunk_total(ctx.handle, L.f64p(C) if nchunks else None, nchunks, cells, L.f64p(carry) if carried else None, L.f64p(out)))
        equal_bits(out, want, "chunk_total_kernel, %d chunks x %d cells, %s" % (nchunks, cells, "carry" if carried else "from zero"), "chunk_total_kernel")
        if carried and nchunks >= 2 and cells >= 255:
            with np.errstate(all="ignore"):
                last = np.zeros(cells)
                for c in C:
                    last = last + c
                last = last + carry
            assert (last != want)[np.isfinite(want)].sum() >= 8                           # a carry added last would show


@pytest.mark.parametrize("parts", [1, 2, 5, 16])
def test_combine_parts_kernel_alone(dev, parts):
    """S = ((Sp[0] + Sp[1]) + Sp[2]) + ... -- on sums that round, so that a part left out, added twice or added in another order
    shows (on the product path the parts of a block are exact in any order)."""
    ctx, L = dev.get_context(), lib()
    for total in CELLS + (3 * 513,):
        Sp = made_up(parts, total, 31 * total + parts)
        want = Sp[0].copy()
        with np.errstate(all="ignore"):
            for p in range(1, parts):
                want = want + Sp[p]
        out = np.full(total, 12345.0)
        L.check(L.load().wgs_debug_combine_parts(ctx.handle, L.f64p(Sp), total, parts, L.f64p(out)))
        equal_bits(out, want, "combine_parts_kernel, %d parts x %d sums" % (parts, total), "combine_parts_kernel")


# ---- the sweeps on the order cases ------------------------------------------------------------------------------------------------------
_values = {}


def values(oracle, shape):
    """(Values, exact block sums (blocks, n, K_ALL), np.sum of every cell (n, K_ALL)) of a shape: once, shared, read-only."""
    if shape not in _values:
        vals = oc.reference(oracle, shape)
        S = oc.block_sums(vals)
        S.setflags(write=False)
        _values[shape] = (vals, S, oc.expected(vals))
    return _values[shape]


def on_device(dev, shape, site_lo=0, site_hi=None):
    """(DeviceBeagle of the shape's sites [site_lo, site_hi) in its slabs, A (sites, K_ALL))."""
    L, A = oc.matrix_of(shape)
    c = oc.case()
    hi = L.shape[0] if site_hi is None else site_hi
    b = dev.DeviceBeagle.from_host(np.ascontiguousarray(L[site_lo:hi]), c["labels"].astype(np.int32), len(c["sizes"]), site0=site_lo)
    return b, A[site_lo:hi]


def sweep(dev, b, afs, colptr=None, rows=None, chunks=False):
    from wgsassign_amd._lib import MODE_EXACT
    s = dev.Score(b, afs, colptr, rows)
    out = s.sums(MODE_EXACT)
    plan = s.plan()
    ch = s.chunk_sums() if chunks else None
    s.close()
    return out, plan, ch


ROWS = (3, 18)                    # cuts a pair of the wave in the slabs of 5, 8 and 9 columns and leaves the slab of 1 out


@pytest.mark.parametrize("shape", oc.SHAPES, ids=["%d blocks, last %s" % s for s in oc.SHAPES])
def test_sweeps_add_their_blocks_in_numpys_order(dev, oracle, monkeypatch, shape):
    """score_coded_kernel in 1, 5 and 16 parts (combine_parts_kernel behind 5 and 16), score_sweep_kernel with shared columns at one
    register batch and two, with a row range that cuts a pair, and with per-individual columns; block_prefix_kernel behind each.
    Every cell of the float64 output is np.sum(vec, dtype=float) of the oracle's vector, every chunk sum the exact one."""
    vals, S, want = values(oracle, shape)
    what = "%d blocks, last %s (%d sites)" % (shape + (vals.m,))
    b, A = on_device(dev, shape)
    n = vals.n
    sets = {K: dev.AFSet.from_host(np.ascontiguousarray(A[:, :K])) for K in oc.K_TESTED}
    want_chunks = oc.chunk_sums(S)
    # through the class codes
    monkeypatch.setenv("WGSASSIGN_CODES", "1")
    monkeypatch.setenv("WGSASSIGN_CODES_TABLE", "64")
    for parts, K in ((1, 6), (5, 13), (16, 6)):
        monkeypatch.setenv("WGS_SCORE_CODED_PARTS", str(parts))
        out, plan, ch = sweep(dev, b, sets[K], chunks=True)
        info = b.codes_info()
        assert info["available"] and plan["path"] == 1 and plan["parts"] == parts and plan["kb"] == {6: 6, 13: 7}[K], (what, plan, info)
        equal_bits(out, want[:, :K], "%s, score_coded_kernel in %d parts, K = %d" % (what, parts, K), "score_coded_kernel")
        equal_bits(ch, want_chunks[:, :, :K], "%s, score_coded_kernel in %d parts, K = %d: chunk sums" % (what, parts, K), "chunk sums")
    # over the float32 slabs
    monkeypatch.setenv("WGSASSIGN_CODES", "0")
    for K in oc.K_TESTED:
        out, plan, ch = sweep(dev, b, sets[K], chunks=True)
        assert plan["path"] == 0 and (plan["kb"], plan["pairs"]) == {6: (6, 2), 13: (7, 1)}[K], (what, plan)
        equal_bits(out, want[:, :K], "%s, score_sweep_kernel, K = %d" % (what, K), "score_sweep_kernel")
        equal_bits(ch, want_chunks[:, :, :K], "%s, score_sweep_kernel, K = %d: chunk sums" % (what, K), "chunk sums")
    lo, hi = ROWS
    out, plan, ch = sweep(dev, b, sets[13], rows=ROWS, chunks=True)
    only, only_chunks = np.zeros_like(want), np.zeros_like(want_chunks)
    only[lo:hi], only_chunks[:, lo:hi] = want[lo:hi], want_chunks[:, lo:hi]
    assert plan["path"] == 0, plan
    equal_bits(out, only, "%s, score_sweep_kernel, rows [%d, %d)" % (what, lo, hi), "score_sweep_kernel rows")
    equal_bits(ch, only_chunks, "%s, score_sweep_kernel, rows [%d, %d): chunk sums" % (what, lo, hi), "chunk sums")
    # per-individual columns: every individual points at 6 columns of its own of the 13; the set handed to the score holds NaN only
    K = 6
    dummy = dev.AFSet.from_host(np.full((vals.m, K), np.nan, dtype=F32))
    pops = np.stack([oc.permutation(i, K) for i in range(n)])
    colptr = np.array([[sets[13].col_dev(int(c)) for c in row] for row in pops], dtype=np.uint64)
    out, plan, _ = sweep(dev, b, dummy, colptr)
    assert plan["path"] == 0 and (plan["kb"], plan["pairs"]) == (6, 1), plan
    equal_bits(out, np.take_along_axis(want, pops, axis=1), "%s, score_sweep_kernel, per-individual columns" % what, "score_sweep_kernel PER_IND")
    for x in (dummy, sets[6], sets[13], b):
        x.close()


# ---- shards in one process --------------------------------------------------------------------------------------------------------------
def sharded_total(dev, shape, cuts, K):
    """The matrix cut at `cuts` (sites), every shard a DeviceBeagle with its site0: wgs_score_sums on each, wgs_score_total_from
    chained.  (the last total, every shard's own sums)"""
    L = lib()
    m = oc.sites_of(shape)
    edges = [0] + list(cuts) + [m]
    run, own = None, []
    for lo, hi in zip(edges[:-1], edges[1:]):
        b, A = on_device(dev, shape, lo, hi)
        afs = dev.AFSet.from_host(np.ascontiguousarray(A[:, :K]))
        s = dev.Score(b, afs)
        own.append(s.sums(L.MODE_EXACT))
        out = np.zeros_like(own[-1])
        L.check(L.load().wgs_score_total_from(s._h, L.f64p(run) if run is not None else None, L.f64p(out)))
        run = out
        for x in (s, afs, b):
            x.close()
    return run, own


@pytest.mark.parametrize("shape", oc.SHARD_SHAPES, ids=["%d blocks, last %s" % s for s in oc.SHARD_SHAPES])
def test_shards_continue_numpys_running_total(dev, oracle, shape):
    """Cut at every multiple of 8192 sites, and at two cuts at once: the total handed from shard to shard is np.sum of the whole
    vector in every cell -- and is not the shards' own sums added, which differ from it in at least eight cells wherever a later
    shard holds a block beyond its first chunk (tests/test_order_cases_cpu.py shows that on the twins)."""
    vals, S, want = values(oracle, shape)
    K = oc.K_ALL
    for cuts in oc.shard_cuts(shape):
        sites = [c * oc.BLOCK for c in cuts]
        run, own = sharded_total(dev, shape, sites, K)
        equal_bits(run, want, "%d blocks, last %s, cut at %r" % (shape + (sites,)), "shards")
        added = own[0]
        for o in own[1:]:
            added = added + o
        equal_bits(added, oc.shard_totals_added(S, cuts), "%d blocks, last %s, cut at %r: the shards' own sums" % (shape + (sites,)), "shards")
        assert oc.different_cells(added, want) >= oc.MIN_DIFFERENT or not oc.shards_can_differ(shape, cuts), cuts


# ---- windows ----------------------------------------------------------------------------------------------------------------------------
WINDOW_SHAPE = (9, "ragged")      # 32933 sites: five windows of 8192, three of 16384, two of 24576 -- the last one short each time


@pytest.fixture(scope="module")
def window_file(tmp_path_factory):
    root = tmp_path_factory.mktemp("order_windows")
    L, A = oc.matrix_of(WINDOW_SHAPE)
    path = str(root / "order.beagle.gz")
    with gzip.open(path, "wb", compresslevel=1) as fh:
        fh.write(oc.beagle_text(L))
    return root, path, np.ascontiguousarray(A)


@pytest.mark.parametrize("forced", [True, False], ids=["coded", "direct"])
@pytest.mark.parametrize("W, windows", [(8192, 5), (16384, 3), (24576, 2)])
def test_windows_continue_numpys_running_total(dev, oracle, window_file, monkeypatch, W, windows, forced):
    """The case as a gzipped Beagle file through glassy.assignLL_windowed, swept through the class codes and over the float32 slabs
    (as test_gpu_windowed.py::test_both_modes forces them): np.sum in every cell.  A window that restarted the running total would
    differ in at least eight cells at 16384 and 24576 sites (at 8192 it cannot: total + chunk either way)."""
    from wgsassign_amd import device, glassy
    root, path, A = window_file
    monkeypatch.setenv("WGSASSIGN_INDEX_DIR", str(root))
    if forced:
        monkeypatch.setenv("WGSASSIGN_CODES_TABLE", "64")
    else:
        monkeypatch.delenv("WGSASSIGN_SCORE_CODES_ALWAYS")
    states = []
    push = device.ScoreStream.push

    def recording(self, beagle, afset, mode=None):
        push(self, beagle, afset, mode)
        states.append(beagle.codes_state())
    monkeypatch.setattr(device.ScoreStream, "push", recording)
    vals, S, want = values(oracle, WINDOW_SHAPE)
    restarted = oc.different_cells(oc.restart_order(S, W), want)
    assert restarted == 0 if W == 8192 else restarted >= oc.MIN_DIFFERENT
    out = glassy.assignLL_windowed(path, A, W)
    st = glassy.assignLL_windowed.stats
    assert st["windows"] == windows and st["window_sites"] == W and vals.m % W != 0          # a short last window
    assert len(states) == windows and all((s == 1) == forced for s in states), states
    equal_bits(out, want, "windows of %d sites, %s" % (W, "coded" if forced else "direct"), "windows")


def test_everything_was_compared():
    """(Last in the file: how many float64 results each part was held to.)"""
    print("compared float64 results: %r" % compared)
    if len(compared) > 3:                                  # (fewer when tests are selected alone)
        for kind in ("block_prefix_kernel", "chunk_total_kernel", "combine_parts_kernel", "score_coded_kernel", "score_sweep_kernel", "score_sweep_kernel rows",
                     "score_sweep_kernel PER_IND", "chunk sums", "shards", "windows"):
            assert compared.get(kind, 0) >= 1000, (kind, compared)
