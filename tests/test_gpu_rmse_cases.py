"""The block-parallel emulation of the reference's serial float32 convergence sum (csrc/em_kernels.hip: rmse_block_sum_kernel,
rmse_predict_kernel, rmse_candidates_kernel / chain_step, rmse_walk_kernel, chain_set_carry_kernel) on the enumerated chains of
tests/rmse_cases.py, through wgs_debug_rmse_chain_batch.  Every comparison is of bits or of integers; there is no tolerance:
    carry_out       the bits of the strict serial float32 accumulation (NaN where it is NaN)
    serial_blocks   exactly the number of NECESSARY serial blocks, derived from the reference chain alone: one more and the fast path
                    lost a block, one fewer and a block was applied that the definition does not allow
    expo            the exponent predicted from the exact prefix sum, per block
    cand            for every block with expo > 0 all six increments by definition, whether the walk uses them or not (an increment
                    of 2^39 or more is compared as "at least 2^24": it does not fit, which is all the walk can learn from it)
tests/test_rmse_cases_cpu.py holds the builders to what they claim and ties the accumulation to the oracle and the real reference."""
import ctypes

import numpy as np
import pytest

import rmse_cases as rc

pytestmark = pytest.mark.gpu
F32 = np.float32
compared = {"rmse_walk_kernel: chains": 0, "rmse_walk_kernel: blocks": 0, "rmse_predict_kernel: blocks": 0, "rmse_candidates_kernel: increments": 0,
            "rmse_candidates_kernel: non-zero terms": 0, "rmse_chain_kernel (literal): chains": 0, "chain_set_carry_kernel: carries": 0}


@pytest.fixture(scope="module")
def dev():
    from wgsassign_amd import _lib, device
    return _lib.load(), device.get_context(), _lib


def run(dev, cases):
    """[(carry_out, serial_blocks, expo, cand)] of the cases (all of one length) as one batch of len(cases) jobs."""
    lib, ctx, _lib = dev
    n, m = len(cases), cases[0].m
    assert all(c.m == m for c in cases)
    nb = rc.nblocks(m)
    a, b = np.ascontiguousarray(np.stack([c.a for c in cases])), np.ascontiguousarray(np.stack([c.b for c in cases]))
    carry = np.array([c.carry for c in cases], dtype=F32)
    out, ser = np.full(n, -1.0, dtype=F32), np.full(n, -7, dtype=np.int32)
    expo, cand = np.full((n, nb), -7, dtype=np.int32), np.full((n, nb, 6), -7, dtype=np.int64)
    _lib.check(lib.wgs_debug_rmse_chain_batch(ctx.handle, _lib.f32p(a), _lib.f32p(b), n, m, _lib.f32p(carry), _lib.f32p(out), _lib.i32p(ser),
                                              _lib.i32p(expo), cand.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    compared["chain_set_carry_kernel: carries"] += n
    return [(out[j], int(ser[j]), expo[j], cand[j]) for j in range(n)]


def same_bits(got, want):
    return rc.bits(got) == rc.bits(want) or (np.isnan(got) and np.isnan(want))


def hold(case, got, what=""):
    """The four outputs of one job against the truth of its case."""
    out, ser, expo, cand = got
    t = case.truth
    bad = np.flatnonzero(expo != t["expo"])
    assert bad.size == 0, "%s%s\n    predicted exponent: device %d, exact prefix sum %d" % (what, rc.describe(case, int(bad[0])), expo[bad[0]], t["expo"][bad[0]])
    for k in np.flatnonzero(t["expo"] > 0):
        for j in range(6):
            want, have = int(t["cand"][k, j]), int(cand[k, j])
            assert (have == want) if want < 1 << 39 else (have >= 1 << 24), "%s%s\n    candidate %d (exponent %d), %s entry mantissa: device %d, by definition %d" % (
                what, rc.describe(case, int(k)), j // 2, t["expo"][k] - 1 + j // 2, ("even", "odd")[j & 1], have, want)
    assert same_bits(out, t["final"]), "%s%s\n    carry_out: device %r (0x%08x), serial float32 sum %r (0x%08x)" % (
        what, rc.describe(case), out, rc.bits(out), t["final"], rc.bits(t["final"]))
    assert ser == len(t["serial"]), "%s%s\n    serial blocks: device %d, necessary %d %r" % (what, rc.describe(case), ser, len(t["serial"]), t["serial"])
    compared["rmse_walk_kernel: chains"] += 1
    compared["rmse_walk_kernel: blocks"] += len(t["expo"])
    compared["rmse_predict_kernel: blocks"] += len(t["expo"])
    compared["rmse_candidates_kernel: increments"] += 6 * int((t["expo"] > 0).sum())
    compared["rmse_candidates_kernel: non-zero terms"] += int((t["sq"] != 0).sum())


def literal(dev, case):
    """wgs_debug_rmse1d(serial = 1), the one-lane kernel, on the case's vectors from a zero carry."""
    lib, ctx, _lib = dev
    out, nser = ctypes.c_double(), ctypes.c_int()
    a, b = np.array(case.a), np.array(case.b)
    _lib.check(lib.wgs_debug_rmse1d(ctx.handle, _lib.f32p(a), _lib.f32p(b), case.m, ctypes.byref(out), 1, ctypes.byref(nser)))
    want = rc.chain_diff(rc.reference_chain(case.truth["sq"], F32(0))[1], case.m)
    assert out.value == want or (np.isnan(out.value) and np.isnan(want)), "%s\n    literal kernel from zero: %r, serial float32 sum %r" % (rc.describe(case), out.value, want)
    compared["rmse_chain_kernel (literal): chains"] += 1


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("be", rc.GRID_BE)
def test_term_grid(dev, be, parity):
    """Every shift and remainder class at entry exponent be, every rotation: the rotations as one batch, rotation 0 also on its own."""
    cases = rc.term_grid(be, parity)
    for case, got in zip(cases, run(dev, list(cases))):
        hold(case, got, "in the batch of rotations: ")
    hold(cases[0], run(dev, [cases[0]])[0])
    for case in cases:
        literal(dev, case)


@pytest.mark.parametrize("family", ["ahead", "behind", "edges", "hostile", "carries"])
def test_family(dev, family):
    for case in rc.cases(family):
        hold(case, run(dev, [case])[0])
        if rc.nblocks(case.m) <= 130:
            literal(dev, case)


def test_long(dev):
    """1025 and 2049 blocks: two and three blocks per thread of rmse_predict_kernel, 17 and 33 rounds of 64 blocks of the walk."""
    for case in rc.cases("long"):
        hold(case, run(dev, [case])[0])


@pytest.mark.parametrize("n", rc.JOB_COUNTS)
def test_jobs(dev, n):
    """Batches of different cases with different carries: every job's outputs are those of the same case run alone, and the truth's."""
    cases = rc.jobs(n)
    batch = run(dev, cases)
    for j, (case, got) in enumerate(zip(cases, batch)):
        alone = run(dev, [case])[0]
        what = "job %d of %d: " % (j, n)
        assert same_bits(got[0], alone[0]) and got[1] == alone[1] and (got[2] == alone[2]).all() and (got[3] == alone[3]).all(), what + rc.describe(case)
        hold(case, got, what)
        if n == max(rc.JOB_COUNTS):
            literal(dev, case)


def em_batch(device, cur, prev):
    """An EM batch of one fit whose current and previous frequencies are cur and prev (tests/test_gpu_rmse.py: test_carry_across_shards)."""
    b = device.DeviceBeagle.from_host(np.zeros((len(cur), 2), dtype=F32))
    em = device.EMBatch(b, [0])
    em.set_f(0, np.ascontiguousarray(prev))
    em.step()                                        # flips the buffers: previous := what was set
    em.set_f(0, np.ascontiguousarray(cur))
    return b, em


def test_carried_chains(dev):
    """wgs_em_rmse_chain, the entry a later SNP shard continues the chain through: the `carries` family, and an `ahead` case cut in two
    at a block edge, one element before and one behind it."""
    from wgsassign_amd import device
    for case in rc.cases("carries"):
        b, em = em_batch(device, case.a, case.b)
        got = em.rmse_chain(0, case.carry)
        em.close(), b.close()
        assert same_bits(got, case.truth["final"]), "%s\n    wgs_em_rmse_chain: %r, serial float32 sum %r" % (rc.describe(case), got, case.truth["final"])
    case = rc.cases("ahead")[1]
    for cut in (2 * rc.RB, 2 * rc.RB - 1, 2 * rc.RB + 1):
        b1, e1 = em_batch(device, case.a[:cut], case.b[:cut])
        b2, e2 = em_batch(device, case.a[cut:], case.b[cut:])
        mid = e1.rmse_chain(0, case.carry)
        got = e2.rmse_chain(0, mid)
        for x in (e1, e2, b1, b2):
            x.close()
        assert same_bits(mid, rc.reference_chain(case.truth["sq"][:cut], case.carry)[1]), (case, cut)
        assert same_bits(got, case.truth["final"]), "%s cut at %d\n    two shards: %r, the whole chain %r" % (rc.describe(case), cut, got, case.truth["final"])


def test_product_entry(dev, golden):
    """emMAF_cy.rmse1d, the drop-in entry, against what the real reference returned (tests/golden/rmse_cases.npz)."""
    from WGSassign import emMAF_cy
    g = golden("rmse_cases.npz")
    cases = rc.golden_cases()
    assert [repr(c) for c in cases] == list(g["names"])
    for case, want in zip(cases, g["rmse1d"]):
        got = emMAF_cy.rmse1d(np.array(case.a), np.array(case.b))
        assert got == want or (np.isnan(got) and np.isnan(want)), "%s\n    emMAF_cy.rmse1d: %r, the reference %r" % (rc.describe(case), got, want)


def test_zz_counts():
    """What the tests above compared (of those that ran)."""
    for name, n in compared.items():
        print("%-45s %9d" % (name, n))
