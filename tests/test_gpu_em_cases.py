"""The four EM sweep kernels on the enumerated terms of tests/em_cases.py: sums that are subnormal, a signed zero, negative, infinite
or NaN, negative and cancelling numerators, frequencies outside (0, 1), each at a chosen column of its slab -- the first and the last
of the first plain buffer, a later plain buffer (the restore of the running sum before the fixup-free loop redoes a buffer), the
checked buffer with the odd tail or a left-out individual.  Every comparison is of bits: NaN exactly where the oracle has NaN, the
same bits elsewhere, the sign of a zero and of an infinity included; there is no tolerance and no exclusion.  The yardstick is the
oracle (oracle/wgs_oracle.c), which tests/test_em_cases_cpu.py ties to the real reference on these inputs
(tests/golden/em_cases.npz) and which holds the builders to what they claim; its results are computed once, shared and read-only.

Each test forces one kernel and asserts through EMBatch.sweep_paths() that exactly that kernel swept:
    em_sweep_kernel            WGSASSIGN_CODES=0, one fit per slab (all twenty populations; a lone leave-one-out re-fit)
    em_sweep_group_kernel      WGSASSIGN_CODES=0 or WGSASSIGN_LOO_CODES=0, 3, 4 and 5 re-fits per slab
    em_coded_kernel            the codes forced; one iteration per sweep through step(), two through fit() at limits 1, 2 and 3
    em_coded_group_kernel      the codes forced, 3, 4 and 5 re-fits per slab
the coded ones with the smallest and the largest quotient table that codes the case (8 and 64 rows).  em_cases.negative_zero_sums
adds the one place where the SIGN of a zero quotient reaches the result: a running sum that a term has underflowed to -0.0.  The float32 EM mode
(WGSASSIGN_EM_MODE=fast) of the two float32-slab kernels is held on the same inputs by tests/test_gpu_fast_cases.py (tests/fast_cases.py)."""
import math

import numpy as np
import pytest

import em_cases as ec

pytestmark = pytest.mark.gpu
F32 = np.float32
KERNELS = ("em_sweep_kernel", "em_sweep_group_kernel", "em_coded_kernel", "em_coded_group_kernel")
compared = {}                     # kernel -> (fit, site) results compared (printed by the last test)


def force(monkeypatch, kernel, rows=None, fuse=None, how="codes off"):
    """The environment that sends the sweeps of the next EMBatch calls to `kernel`."""
    if kernel.startswith("em_sweep"):
        if how == "codes off":
            monkeypatch.setenv("WGSASSIGN_CODES", "0")
        else:                                              # the codes exist and serve single fits; leave-one-out batches keep the float32 kernel
            monkeypatch.setenv("WGSASSIGN_CODES", "1")
            monkeypatch.setenv("WGSASSIGN_LOO_CODES", "0")
            monkeypatch.setenv("WGSASSIGN_EM_CODES_MIN", "1")
    else:
        monkeypatch.setenv("WGSASSIGN_CODES", "1")
        monkeypatch.setenv("WGSASSIGN_EM_CODES_SWEEPS", "0")
        monkeypatch.setenv("WGSASSIGN_EM_CODES_MIN", "1")
        if rows is not None:
            monkeypatch.setenv("WGSASSIGN_EM_TABLE_ROWS", str(rows))
    if fuse is not None:
        monkeypatch.setenv("WGSASSIGN_EM_FUSE", str(fuse))
    monkeypatch.delenv("WGSASSIGN_EM_MODE", raising=False)
    monkeypatch.delenv("WGSASSIGN_MODE", raising=False)


def on_device(grid):
    from wgsassign_amd import device
    return device.DeviceBeagle.from_host(grid["L"], grid["labels"].astype(np.int32), len(grid["sizes"]))


def swept(em, before, kernel, sweeps=None):
    """Exactly `kernel` swept since `before` (sweeps: how often; None: at least once)."""
    after = em.sweep_paths()
    delta = [a - b for a, b in zip(after, before)]
    i = KERNELS.index(kernel)
    assert delta[i] >= 1 and (sweeps is None or delta[i] == sweeps) and all(d == 0 for j, d in enumerate(delta) if j != i), \
        "%s expected%s, the sweeps went %r" % (kernel, "" if sweeps is None else " %d times" % sweeps, dict(zip(KERNELS, delta)))
    return after


def coded_all(b, rows):
    """The codes serve every tile of the case with a table of `rows` rows: no tile goes direct inside a coded kernel."""
    info = b.codes_info()
    assert info["available"] and info["em_table_rows"] == rows and info["em_direct_tile_share"] == 0.0 and info["rich_snp_share"] == 0.0, \
        "the case is not coded throughout: %r" % {k: info[k] for k in ("available", "em_table_rows", "em_direct_tile_share", "rich_snp_share")}


def equal(got, want, grid, fits, what, kernel):
    """got, want (fits, m) float32; fits: [(population, left-out slab column or None)].  AssertionError naming the first (fit, site)
    that is not the reference's, with its cell and place."""
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    compared[kernel] = compared.get(kernel, 0) + want.size
    bad = ec.first_difference(got, want)
    if bad is not None:
        j, site = (int(x) for x in np.unravel_index(bad, want.shape))
        n_bad = int(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).sum())
        raise AssertionError("%s, %s: %d of %d results differ, first at fit %d, site %d: device %r (0x%08x), reference %r (0x%08x)\n    %s" % (
            what, kernel, n_bad, want.size, j, site, got[j, site], got.view(np.uint32)[j, site], want[j, site], want.view(np.uint32)[j, site],
            ec.describe(grid, fits[j][0], site, fits[j][1])))
    assert ec.same_nan(want, got), what


def sums_agree(ssq, f_new, f_old, what):
    """step()'s float64 sums: non-finite exactly when a per-site float32 square (f_new - f_old)^2 is, else within m * 2^-53 relative of
    math.fsum of those squares -- the rounding bound of a float64 sum of m non-negative terms in any order."""
    for j in range(len(ssq)):
        sq = ec.squares(f_new[j], f_old[j])
        if not np.isfinite(sq).all():
            assert not math.isfinite(ssq[j]), (what, j, ssq[j])
        else:
            exact = math.fsum(sq.astype(np.float64))
            assert math.isfinite(ssq[j]) and abs(ssq[j] - exact) <= len(sq) * 2.0 ** -53 * exact, (what, j, ssq[j], exact)


def get_all(em):
    return np.stack([em.get_f(j) for j in range(em.n_fits)])


def one_fit_per_population(oracle, monkeypatch, variant, kernel, rows=None):
    """Two step()s of all twenty populations from the enumerated frequencies, the sums of squares of both."""
    from wgsassign_amd import device
    grid, want = ec.reference(oracle, variant)
    K = len(grid["sizes"])
    force(monkeypatch, kernel, rows, fuse=1)
    b = on_device(grid)
    em = device.EMBatch(b, np.arange(K, dtype=np.int32))
    for k in range(K):
        em.set_f(k, grid["f_old"][k])
    fits = [(k, None) for k in range(K)]
    paths, old = em.sweep_paths(), grid["f_old"]
    assert paths == [0, 0, 0, 0]
    for u in range(2):
        with np.errstate(all="ignore"):
            ssq = em.step()
        paths = swept(em, paths, kernel, 1)
        got = get_all(em)
        equal(got, want[u], grid, fits, "%s, update %d" % (variant, u + 1), kernel)
        sums_agree(ssq, want[u], old, "%s, update %d" % (variant, u + 1))
        old = want[u]
    if rows is not None:
        coded_all(b, rows)
    em.close()
    b.close()


def leave_one_out(oracle, monkeypatch, variant, kernel, single, rows=None, how="codes off"):
    """1, 3, 4 and 5 re-fits of each of the populations of 9, 17, 33 and 49 in one batch: a lone fit per slab goes to the single-fit
    kernel `single` (its checked buffer holds the left-out individual), 3 and 4 share a tile, 5 make two groups."""
    from wgsassign_amd import device
    grid = ec.grid_of(variant)
    force(monkeypatch, kernel, rows, fuse=1, how=how)
    b = on_device(grid)
    pops = [ec.SIZES.index(size) for size in ec.LOO_SIZES]
    refs = {k: ec.reference_loo(oracle, variant, k) for k in pops}
    for count in ec.LOO_BATCHES:
        if count == 1 and single is None:
            continue
        groups, skips, fits, want, old = [], [], [], [], []
        for k in pops:
            g, s, cols = ec.loo_fits(grid, k, count)
            groups += list(g)
            skips += list(s)
            fits += [(k, c) for c in cols]
            want.append(refs[k][2][:2, :count])
            old += [grid["f_old"][k]] * count
        want = np.concatenate(want, axis=1)
        em = device.EMBatch(b, np.array(groups, dtype=np.int32), np.array(skips, dtype=np.int32))
        for j in range(em.n_fits):
            em.set_f(j, old[j])
        paths, prev = em.sweep_paths(), np.stack(old)
        for u in range(2):
            with np.errstate(all="ignore"):
                ssq = em.step()
            paths = swept(em, paths, single if count == 1 else kernel, 1)
            what = "%s, %d re-fits per slab, update %d" % (variant, count, u + 1)
            equal(get_all(em), want[u], grid, fits, what, single if count == 1 else kernel)
            sums_agree(ssq, want[u], prev, what)
            prev = want[u]
        em.close()
    if rows is not None:
        coded_all(b, rows)
    b.close()


@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_em_sweep_kernel(oracle, monkeypatch, variant):
    one_fit_per_population(oracle, monkeypatch, variant, "em_sweep_kernel")


@pytest.mark.parametrize("how", ["codes off", "leave-one-out codes off"])
@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_em_sweep_group_kernel(oracle, monkeypatch, variant, how):
    leave_one_out(oracle, monkeypatch, variant, "em_sweep_group_kernel", "em_sweep_kernel" if how == "codes off" else None, how=how)


@pytest.mark.parametrize("rows", [8, 64])
@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_em_coded_kernel_one_iteration_per_sweep(oracle, monkeypatch, variant, rows):
    one_fit_per_population(oracle, monkeypatch, variant, "em_coded_kernel", rows)


@pytest.mark.parametrize("max_iter", [1, 2, 3])
@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_em_coded_kernel_fused(oracle, monkeypatch, variant, max_iter):
    """fit() with a tolerance nothing meets: `max_iter` updates of the oracle, two per sweep -- limit 1: one single sweep; 2: one fused
    sweep; 3: a fused sweep and a single one."""
    from wgsassign_amd import device
    grid, want = ec.reference(oracle, variant)
    K = len(grid["sizes"])
    force(monkeypatch, "em_coded_kernel", 8)
    monkeypatch.delenv("WGSASSIGN_EM_FUSE", raising=False)
    b = on_device(grid)
    em = device.EMBatch(b, np.arange(K, dtype=np.int32))
    for k in range(K):
        em.set_f(k, grid["f_old"][k])
    paths = em.sweep_paths()
    iters = em.fit(max_iter, 1e-30)
    print("max_iter %d: sweeps %r, iterations enqueued %d" % (max_iter, em.sweep_paths(), em.fit_stats()[0]))
    swept(em, paths, "em_coded_kernel", (max_iter + 1) // 2)
    assert (iters == 0).all(), iters
    equal(get_all(em), want[max_iter - 1], grid, [(k, None) for k in range(K)], "%s, fit(%d)" % (variant, max_iter), "em_coded_kernel")
    coded_all(b, 8)
    em.close()
    b.close()


@pytest.mark.parametrize("rows", [8, 64])
@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_em_coded_group_kernel(oracle, monkeypatch, variant, rows):
    leave_one_out(oracle, monkeypatch, variant, "em_coded_group_kernel", "em_coded_kernel", rows)


@pytest.mark.parametrize("kernel", ["em_sweep_kernel", "em_coded_kernel"])
def test_a_running_sum_of_negative_zero(oracle, monkeypatch, kernel):
    """em_cases.negative_zero_sums: once a term has underflowed the float32 sum to -0.0, a numerator of -0.0 over a positive sum has to
    give a quotient of -0.0 -- in the fixup-free loop too -- or the sum turns to +0.0 and the frequency with it.  The reference returns
    -0.0 at every site."""
    from wgsassign_amd import device
    case, want = ec.reference_zeros(oracle)
    K = len(case["sizes"])
    force(monkeypatch, kernel, 8, fuse=1)
    b = on_device(case)
    em = device.EMBatch(b, np.arange(K, dtype=np.int32))
    for k in range(K):
        em.set_f(k, case["f_old"][k])
    paths = em.sweep_paths()
    ssq = em.step()
    swept(em, paths, kernel, 1)
    got = get_all(em)
    compared[kernel] = compared.get(kernel, 0) + got.size
    bad = ec.first_difference(got, want[0])
    if bad is not None:
        k, site = (int(x) for x in np.unravel_index(bad, got.shape))
        raise AssertionError("%s: %d of %d results are not the reference's -0.0, first at population %d of %d, site %d (the pair (1, 0.5) at column %d): %r (0x%08x)" % (
            kernel, int((got.view(np.uint32) != want[0].view(np.uint32)).sum()), got.size, k, case["sizes"][k], site, case["lead_col"][site, k],
            got[k, site], got.view(np.uint32)[k, site]))
    sums_agree(ssq, want[0], case["f_old"], "negative zero sums")
    em.close()
    b.close()


@pytest.mark.parametrize("variant", ec.VARIANTS)
def test_the_thin_mirror(oracle, variant):
    """emMAF_cy.emMAF_update, the upload path: one population's gathered columns and its frequencies in, the update in place."""
    from wgsassign_amd import emMAF_cy
    grid, want = ec.reference(oracle, variant)
    for size in (1, 9, 16, 33):
        k = ec.SIZES.index(size)
        f = grid["f_old"][k].copy()
        with np.errstate(all="ignore"):
            emMAF_cy.emMAF_update(ec.columns(grid["L"], grid["members"][k]), f, 1)
        equal(f[None, :], want[0, k][None, :], grid, [(k, None)], "%s, emMAF_update" % variant, "the thin mirror")


@pytest.mark.parametrize("fuse", [1, 2])
@pytest.mark.parametrize("kernel", ["em_sweep_kernel", "em_coded_kernel"])
def test_whole_fits_of_the_finite_variant(oracle, golden, monkeypatch, kernel, fuse):
    """emMAF.py:15-27 from 0.25, 200 iterations, 1e-4: the iteration at which every population's fit stops and its frequencies, against
    the oracle on all twenty populations and against the real reference's record on the six it holds."""
    from wgsassign_amd import device
    g = golden("em_cases.npz")
    for sizes in (ec.SIZES, ec.GOLDEN_SIZES):
        grid = ec.grid_of("finite", sizes)
        K = len(sizes)
        force(monkeypatch, kernel, 8, fuse=fuse)
        b = on_device(grid)
        em = device.EMBatch(b, np.arange(K, dtype=np.int32))
        paths = em.sweep_paths()
        iters = em.fit(200, 1e-4)
        swept(em, paths, kernel)
        got = get_all(em)
        em.close()
        b.close()
        ref = [oracle.emMAF(ec.columns(grid["L"], grid["members"][k]), 200, 1e-4, 1) for k in range(K)]
        assert list(iters) == [it for _, it in ref] and min(iters) > 0, (list(iters), [it for _, it in ref])
        equal(got, np.stack([f for f, _ in ref]), grid, [(k, None) for k in range(K)], "finite, whole fits", kernel)
        if sizes == ec.GOLDEN_SIZES:
            assert ec.digest(grid) == str(g["finite_digest"]) and list(iters) == list(g["finite_fit_iters"])
            equal(got, g["finite_fit"], grid, [(k, None) for k in range(K)], "finite, whole fits against the golden", kernel)


def test_every_kernel_was_compared():
    """(Last in the file: how many (fit, site) results each kernel was held to.)"""
    print("compared (fit, site) results per kernel: %r" % compared)
    if compared:                                           # (empty when this test is selected alone)
        assert set(KERNELS) <= set(compared) and all(compared[k] >= 10000 for k in KERNELS), compared
