"""The assignment kernel's double-precision log of float32 arguments (csrc/assign_kernels.hip:
log_f32arg) against libm.  The reference stores (float)log((double)s) per site
(glassy_cy.pyx:21); the device function must give the same float32 for every float32 s, up to
the handful of arguments whose true log lies within a double ulp of a float32 rounding boundary."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from wgsassign_amd import _lib, device
    ctx = device.get_context()
    return _lib.load(), ctx, _lib


def values(dev, x, use_libm=0):
    lib, ctx, _lib = dev
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    _lib.check(lib.wgs_debug_log_values(ctx.handle, _lib.f32p(x), _lib.f32p(out), x.shape[0], use_libm))
    return out


def test_exhaustive_vs_device_libm(dev):
    """Every positive finite float32 (2^31 - 2^23 bit patterns): custom vs the device math library."""
    lib, ctx, _lib = dev
    count, first = ctypes.c_uint64(), ctypes.c_uint32()
    _lib.check(lib.wgs_debug_log_mismatch(ctx.handle, 1, 0x7F800000, ctypes.byref(count), ctypes.byref(first)))
    print("float32-rounded log mismatches vs ocml over all positive float32:", count.value, "first bits", hex(first.value))
    assert count.value <= 64, (count.value, hex(first.value))


def test_dense_sample_vs_glibc(dev, oracle):
    """Against the reference's own libm: every 61st bit pattern of the whole positive range, every
    pattern of [0.999, 1.001] (where log passes through zero) and the likelihood-sum range (0, 1]
    at stride 7."""
    total = mism = 0
    worst = []
    for bits in (np.arange(1, 0x7F800000, 61, dtype=np.uint32),
                 np.arange(np.float32(0.999).view(np.uint32), np.float32(1.001).view(np.uint32) + 1, dtype=np.uint32),
                 np.arange(0x2F000000, 0x3F800001, 7, dtype=np.uint32)):
        x = bits.view(np.float32)
        mine = values(dev, x)
        ref = oracle.log_f32(np.ascontiguousarray(x), 8)
        bad = mine.view(np.uint32) != ref.view(np.uint32)
        total += len(x)
        mism += int(bad.sum())
        if bad.any():
            worst.append(int(np.max(np.abs(mine[bad].view(np.int32).astype(np.int64) - ref[bad].view(np.int32)))))
    print("vs glibc: %d of %d float32-rounded values differ" % (mism, total))
    assert mism <= max(8, total // 20_000_000) and all(w <= 1 for w in worst)     # at most 1 float32 ulp, a handful of cases


def test_exhaustive_vs_glibc(dev, oracle):
    """EVERY positive finite float32 (2,139,095,039 arguments): the device function against
    (float)log((double)x) of the host's glibc -- the exact expression the reference evaluates
    (glassy_cy.pyx:21 with a zero-initialised vector)."""
    threads = min(len(__import__("os").sched_getaffinity(0)), 16)
    total = mism = 0
    first = []
    step = 1 << 26
    for b0 in range(0, 0x7F800000, step):
        bits = np.arange(max(b0, 1), min(b0 + step, 0x7F800000), dtype=np.uint32)
        x = bits.view(np.float32)
        mine = values(dev, x)
        ref = oracle.log_f32(x, threads)
        bad = np.flatnonzero(mine.view(np.uint32) != ref.view(np.uint32))
        total += len(x)
        mism += len(bad)
        first += [hex(int(bits[i])) for i in bad[:4]]
    print("exhaustive vs glibc: %d of %d float32-rounded logs differ %s" % (mism, total, first[:8]))
    assert total == 0x7F800000 - 1 and mism <= 16


def test_special_values(dev):
    x = np.array([0.0, -0.0, -1.0, np.inf, np.nan, 1.0, 1e-45, 1.1754944e-38, 3.4028235e38, -np.inf], dtype=np.float32)
    with np.errstate(all="ignore"):
        want = np.log(x.astype(np.float64)).astype(np.float32)
    got = values(dev, x)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok])
    assert got[5] == 0.0 and got[0] == -np.inf and got[1] == -np.inf and got[3] == np.inf


def test_special_values_of_negative_and_subnormal_arguments(dev):
    """The hardware log that supplies libm's special values flushes a subnormal argument to a zero of its sign: a NEGATIVE subnormal
    must still give NaN (log of a negative number), not -inf, and a positive one its finite log (tests/score_cases.py reaches both
    through subnormal likelihoods)."""
    x = np.array([-1e-45, -1e-40, -1.1754942e-38, -1.1754944e-38, -1e-30, -3.4028235e38, -np.inf, 1e-40, 1.1754942e-38, 2e-45], dtype=np.float32)
    with np.errstate(all="ignore"):
        want = np.log(x.astype(np.float64)).astype(np.float32)
    got = values(dev, x)
    assert np.isnan(want[:7]).all() and np.isfinite(want[7:]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want)), got
    assert got[7:].tobytes() == want[7:].tobytes()


# ---- the two hardware steps of the float32 modes (csrc/fast_math.h) ------------------------------------------------------------------
# Their error constants are measurements of the chip, recorded in tests/fast_cases.py and DESIGN section 4; the passes are exhaustive,
# so the recorded constants carry no margin beyond rounding up to the next half ulp, and the measured maxima may not exceed them.
def fast_values(dev, which, x):
    lib, ctx, _lib = dev
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    _lib.check(lib.wgs_debug_fast_values(ctx.handle, which, _lib.f32p(x), _lib.f32p(out), x.shape[0]))
    return out


def fast_scan(dev, which, b0, b1):
    """dict(ulps, ulps_arg, abs, abs_arg, differ, first) over the bit patterns [b0, b1) (wgs_debug_fast_scan)."""
    lib, ctx, _lib = dev
    st = (ctypes.c_double * 6)()
    _lib.check(lib.wgs_debug_fast_scan(ctx.handle, which, b0, b1, st))
    return dict(ulps=st[0], ulps_arg=int(st[1]), abs=st[2], abs_arg=int(st[3]), differ=int(st[4]), first=None if st[5] < 0 else int(st[5]))


def test_fast_log_exhaustive(dev):
    """fast_log over EVERY positive finite float32, subnormals included, against log_f32arg (which the tests above tie to glibc): the
    error in float32 ulps of the true log, and no argument whose result is of another class.  The relative form holds around x = 1
    too, so there is no absolute part."""
    import fast_cases as fc
    whole = fast_scan(dev, 0, 1, 0x7F800000)
    near_one = fast_scan(dev, 0, 126 << 23, 128 << 23)
    subnormal = fast_scan(dev, 0, 1, 0x00800000)
    print("fast_log: %.6f ulps at 0x%08x over every positive float32; %.6f at 0x%08x over [0.5, 2); %.6f at 0x%08x over the subnormals; %d class differences" % (
        whole["ulps"], whole["ulps_arg"], near_one["ulps"], near_one["ulps_arg"], subnormal["ulps"], subnormal["ulps_arg"], whole["differ"]))
    assert whole["differ"] == 0 and whole["first"] is None
    assert 0 < whole["ulps"] <= fc.FAST_LOG_REL_ULPS
    assert max(near_one["ulps"], subnormal["ulps"]) <= whole["ulps"]
    assert fc.FAST_LOG_REL_ULPS - 0.5 < fc.FAST_LOG_MEASURED[0] <= fc.FAST_LOG_REL_ULPS          # the record is the measurement rounded up, no more


def test_fast_log_special_arguments(dev):
    """+-0 -> -inf; every negative argument, subnormal, normal or -inf -> NaN; NaN -> NaN; +inf -> +inf; 1 -> +0; positive subnormals and
    the largest finite value their finite logs within the recorded error."""
    import fast_cases as fc
    x = np.array([0.0, -0.0, -1e-45, -1e-40, -1.1754942e-38, -1.1754944e-38, -1.0, -3.4028235e38, -np.inf, np.nan, np.inf, 1.0,
                  1e-45, 1e-40, 2e-40, 1.1754942e-38, 1.1754944e-38, 3.4028235e38], dtype=np.float32)
    got = fast_values(dev, 0, x)
    print(got.tolist())
    assert np.isneginf(got[:2]).all() and np.isnan(got[2:10]).all() and got[10] == np.inf
    assert got[11] == 0.0 and not np.signbit(got[11])
    want = np.log(x[12:].astype(np.float64))
    assert np.isfinite(got[12:]).all() and (np.abs(got[12:] - want) <= fc.FAST_LOG_REL_ULPS * fc.ulp32(want)).all(), (got[12:], want)
    assert abs(got[14] + 91.4) < 0.05                      # a likelihood of 2e-40: -91.4, not -inf


def test_fast_rcp_exhaustive(dev):
    """fast_rcp = v_rcp_f32 over EVERY finite float32 of either sign against the IEEE double division: the error where both are finite
    and not zero, and the arguments whose result is of another class -- exactly the subnormals above 2^-128 (taken for zero: +-inf)
    and the arguments above 2^126 (a subnormal reciprocal: +-0)."""
    import fast_cases as fc
    for sign in (0, 0x80000000):
        whole = fast_scan(dev, 1, sign, sign + 0x7F800000)
        print("fast_rcp, sign bit %d: %.6f ulps at 0x%08x; %d class differences, first 0x%08x" % (sign >> 31, whole["ulps"], whole["ulps_arg"], whole["differ"], whole["first"]))
        assert 0 < whole["ulps"] <= fc.FAST_RCP_REL_ULPS
        assert (whole["differ"], whole["first"]) == (fc.FAST_RCP_CLASS_DIFFERENCES[0], sign + fc.FAST_RCP_CLASS_DIFFERENCES[1])
        assert fast_scan(dev, 1, sign, sign + 0x00200001)["differ"] == 0                         # +-0 and |x| <= 2^-128: +-inf either way
        assert fast_scan(dev, 1, sign + 0x00200001, sign + 0x00800000)["differ"] == 0x00800000 - 0x00200001
        assert fast_scan(dev, 1, sign + 0x00800000, sign + 0x7E800001)["differ"] == 0            # normal arguments up to 2^126
        assert fast_scan(dev, 1, sign + 0x7E800001, sign + 0x7F800000)["differ"] == 0x7F800000 - 0x7E800001
    assert fc.FAST_RCP_REL_ULPS - 0.5 < fc.FAST_RCP_MEASURED[0] <= fc.FAST_RCP_REL_ULPS


def test_fast_rcp_special_arguments(dev):
    x = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, np.inf, -np.inf, np.nan, 3.4028235e38, -3.4028235e38,
                  1.1754944e-38, -1.1754944e-38, 2.0 ** 126, 1.0, -1.0, 3.0], dtype=np.float32)
    got = fast_values(dev, 1, x)
    print(got.tolist())
    assert got[0] == np.inf and got[1] == -np.inf
    assert got[2] == np.inf and got[3] == -np.inf and got[4] == np.inf and got[5] == -np.inf       # subnormals of either sign: a zero of their sign
    assert got[6] == 0.0 and not np.signbit(got[6]) and got[7] == 0.0 and np.signbit(got[7]) and np.isnan(got[8])
    assert got[9] == 0.0 and not np.signbit(got[9]) and got[10] == 0.0 and np.signbit(got[10])     # a subnormal reciprocal: a zero of its sign
    assert got[11] == np.float32(2.0 ** 126) and got[12] == -np.float32(2.0 ** 126) and got[13] == np.float32(2.0 ** -126)
    assert got[14] == 1.0 and got[15] == -1.0 and abs(float(got[16]) - 1 / 3) <= 2.0 ** -25


def test_em_divide_is_ieee_exact(dev):
    """The EM kernel's Newton-core divide (no v_div_scale) against the compiler's IEEE double divide
    on 4.3e9 pseudo-random EM-shaped operand pairs (incl. 0/0 and 100 binades of magnitude)."""
    lib, ctx, _lib = dev
    bad = ctypes.c_uint64(123)
    _lib.check(lib.wgs_debug_div_mismatch(ctx.handle, 20260313, 4096, ctypes.byref(bad)))
    assert bad.value == 0, bad.value


def test_em_divide_is_ieee_exact_on_signed_and_cancelling_operands(dev):
    """The same divide over the operands the enumerated EM terms show to exist (tests/em_cases.py): p2 of either sign, sums that cancel
    to a few ulps under a negative numerator, denominators from the smallest float32 subnormal to 2^127 and quotients from 2^-277 to
    2^277 -- with the fixup against the IEEE divide on all 5.4e8 pairs, and the fixup-free form of em_sweep_kernel's hot loop wherever
    its precondition (a positive finite denominator) holds."""
    lib, ctx, _lib = dev
    bad = (ctypes.c_uint64 * 2)(123, 456)
    _lib.check(lib.wgs_debug_div_mismatch_signed(ctx.handle, 20260313, 512, bad))
    assert (bad[0], bad[1]) == (0, 0), (bad[0], bad[1])


def test_em_divide_reciprocal_bound_exhaustive(dev):
    """div_exact uses ONE Newton refinement of v_rcp_f64.  Its exactness argument (csrc/em_kernels.hip) needs the
    refined reciprocal within 2^-48 of 1/den: checked here for EVERY float32 mantissa of the denominator (2^23 values),
    at exponents from float32-denormal sums to the largest possible sum."""
    lib, ctx, _lib = dev
    for exponent in (-149, -126, -100, -30, -1, 0, 1, 2):
        worst = ctypes.c_double(-1.0)
        _lib.check(lib.wgs_debug_rcp_error(ctx.handle, exponent, ctypes.byref(worst)))
        assert 0 <= worst.value < 2.0 ** -48, (exponent, worst.value)
