"""The float32 modes on enumerated terms.  First the scoring kernels (csrc/assign_kernels.hip: site_ll_fast in assign_kernel,
loglike_site_kernel, score_sweep_kernel and score_coded_kernel; MODE_FAST, WGSASSIGN_MODE=fast) on the terms of tests/score_cases.py;
this file invents no input.  NumPy and the standard library only.  Four things:

THE RESTATEMENT.  fast_sum / fast_terms: site_ll_fast operation by operation in NumPy float32, written from its contract --
    g2   = (float)((1.0 - (double)g0) - (double)g1)                 formed as the reference forms it, rounded once
    oma  = 1 - a;  like0 = (g0 * oma) * oma;  like1 = ((g1 * 2) * oma) * a;  like2 = (g2 * a) * a;  s = (like0 + like1) + like2
    v    = fast_log(s)
every operation an IEEE float32 one (the build has -ffp-contract=off), fast_log (csrc/fast_math.h) handed in as a function.  Given the
device's own fast_log values (one call of wgs_debug_fast_values on the distinct sums) the restatement predicts a float32-mode kernel
BIT FOR BIT: tests/test_gpu_fast_cases.py.  A cell's float64 sum is exact in any order (score_cases.exact_sum_margin holds for the
restated values too), so the expected sum of a cell is math.fsum of its terms.

THE REFERENCE.  real_terms: the term in real arithmetic from the float32 inputs, S = g0 (1-a)^2 + 2 g1 (1-a) a + ((1-g0)-g1) a^2
with fractions.Fraction on the distinct (pair, frequency) products -- a few thousand -- and broadcast; log S = math.log of the
correctly rounded double.  Its own error: 2^-53 relative in S and an ulp of math.log, together below REF_ERR (1 + |log S|).

THE BOUND.  term_bound: what a float32 evaluation may deviate by from log S where S > 0, DERIVED (DESIGN section 4 has the same
derivation in prose).  With u = 2^-24 and L0, L1, L2 the three real likelihood terms:
  * the computed s = sum_j L_j (1 + theta_j) + underflow, |theta_j| <= gamma_6 = 6u / (1 - 6u): L0 passes the rounding of oma
    twice, two products and two additions (6 roundings), L1 that of oma, two products (g1 * 2 is exact) and two additions (5), L2 that
    of g2 -- whose double operations add 2^-52 -- two products and one addition (4);
  * so |s - S| / S <= gamma_6 kappa + E_under / S =: eps with the condition number kappa = sum_j |L_j| / S and E_under one half
    of the smallest subnormal, 2^-150, per product that can underflow (six, the first of each term carried through a factor |1-a|
    or |a|) and for the rounding of g2; the two additions are exact where they underflow;
  * through the log: |log s - log S| <= -log(1 - eps)                                                   (eps < 1, else no bound);
  * fast_log(s) is within fast_log_error of log s: the chip's measured error, FAST_LOG_REL_ULPS float32 ulps of the log
    (tests/test_gpu_log.py holds it over every positive float32), which includes the rounding of the multiplication by ln 2 and of the 32 taken off a scaled argument;
  * the reference's own error.
A term is compared by bound exactly when S > 0; every other term by class against the oracle, -inf or NaN as the oracle has it.

THE CLASS TABLE.  class_table: for every term the class of the reference's float32 sum (score_cases.like_sum, the oracle's rounding
sequence) against the class of the float32 mode's sum, the differences counted and named.  On `finite` there is none.

What the enumerated terms found in the parent of this file: g2 formed in float32 is exactly 0 for the pair (0.001,
0.999), whose double g2 is -1.29e-8 -- a sum of 0 (-inf) at a = 1 where the reference's is negative (NaN), 696 terms of the grid, and
12 % off at a = 1 - 2^-24, 1269 terms beyond 1e-6; v_log_f32 takes a positive subnormal sum for zero (813 terms of the grid, 5237 of
the block: -inf where the reference has -91.4), and a negative subnormal one for -0 (-inf where the reference has NaN).

The float32 EM sweeps (em_sweep_kernel<FAST>, em_sweep_group_kernel<FAST>: term_fast) on the cells of tests/em_cases.py have the same
four things in the second half of this file: fast_update, real_quotients, update_bound, and the count of compared (fit, site)."""
import math
from fractions import Fraction

import numpy as np

import score_cases as sc

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of float32
GAMMA6 = 6 * U / (1 - 6 * U) + 2.0 ** -50       # six float32 roundings, and the double operations that form g2 and widen nothing else
ETA = 2.0 ** -150                   # the largest error of one rounding into the subnormal range
REF_ERR = 2.0 ** -50                # the reference's own error, relative to 1 + |log S|
TINY = float(np.finfo(F32).tiny)

# ---- the chip's constants ------------------------------------------------------------------------------------------------------------
# Measured on the MI355X by tests/test_gpu_log.py (wgs_debug_fast_scan), rounded up to the next half ulp and nothing more; the test
# asserts that the measured maxima do not exceed them.
#   fast_log over EVERY positive finite float32, subnormals included, against log_f32arg: the error in float32 ulps of the true log.
#   The measurement supports the relative form everywhere: around x = 1, where the log passes through zero and an ulp of it vanishes,
#   the error is 1.842003 ulps at most (over [0.5, 2), at 0x3f1b90c2) -- no absolute part is needed.  The largest, 2.219845 ulps,
#   stands at 0x2864232e (1.2664e-14); over the subnormal arguments, which are scaled, 1.916582 at 0x001f8fb5.
FAST_LOG_REL_ULPS = 2.5
FAST_LOG_MEASURED = (2.219845, 0x2864232E)
#   fast_rcp = v_rcp_f32 over every finite float32 of either sign against the IEEE double division, where both are finite and not
#   zero: 0.881809 ulps at 0x00837bf0 (and at its negative).  The classes differ for 23 068 670 arguments of either sign: the
#   6 291 455 subnormals above 2^-128 are taken for zero (+-inf where the reciprocal is finite; at and below 2^-128 it overflows
#   anyway), and the 16 777 215 arguments above 2^126 give +-0 where the reciprocal is subnormal.
FAST_RCP_REL_ULPS = 1.0
FAST_RCP_MEASURED = (0.881809, 0x00837BF0)
FAST_RCP_CLASS_DIFFERENCES = (23068670, 0x00200001)     # per sign: how many, and the first among the positive arguments


def ulp32(t):
    """The float32 ulp of |t| (array or scalar): 2^(exponent - 23), no smaller than 2^-149."""
    t = np.abs(np.asarray(t, dtype=np.float64))
    e = np.frexp(np.where(t > 0, t, 1.0))[1] - 1
    return np.ldexp(1.0, np.maximum(np.where(t > 0, e, -126), -126) - 23)


def fast_log_error(x_lo, x_hi, rel_ulps=None):
    """The largest |fast_log(x) - log x| over the float32 x of [x_lo, x_hi] (arrays of positive float64) that the measurement allows."""
    x_lo, x_hi = np.asarray(x_lo, dtype=np.float64), np.asarray(x_hi, dtype=np.float64)
    with np.errstate(all="ignore"):
        far = np.maximum(np.abs(np.log(np.maximum(x_lo, 2.0 ** -150))), np.abs(np.log(x_hi)))
    return (FAST_LOG_REL_ULPS if rel_ulps is None else rel_ulps) * ulp32(far)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def g2_rounded(g0, g1):
    with np.errstate(all="ignore"):
        return ((1.0 - np.asarray(g0, dtype=F32).astype(np.float64)) - np.asarray(g1, dtype=F32).astype(np.float64)).astype(F32)


def fast_sum(g0, g1, a, g2=None):
    """s of site_ll_fast for float32 g0, g1, a (broadcast).  g2: another way to form it (what a mutation would do)."""
    g0, g1, a = (np.asarray(x, dtype=F32) for x in (g0, g1, a))
    g2 = g2_rounded(g0, g1) if g2 is None else np.asarray(g2, dtype=F32)
    one, two = F32(1.0), F32(2.0)
    with np.errstate(all="ignore"):
        oma = one - a
        like0 = (g0 * oma) * oma
        like1 = ((g1 * two) * oma) * a
        like2 = (g2 * a) * a
        s = (like0 + like1) + like2
    assert s.dtype == F32
    return s


def fast_sums_of(case, pops=None):
    """(m, n, K) float32: the float32 mode's s of every (site, individual, population)."""
    A = case["A"] if pops is None else case["A"][:, pops]
    return fast_sum(case["L"][:, 0::2, None], case["L"][:, 1::2, None], A[:, None, :])


def log_correct(s):
    """The correctly rounded natural log of float32 s as float32, with libm's special values."""
    with np.errstate(all="ignore"):
        return np.log(np.asarray(s, dtype=F32).astype(np.float64)).astype(F32)


def through(prim, s):
    """prim on the DISTINCT values of s (by bit pattern), broadcast back: prim may be a call to the device."""
    s = np.ascontiguousarray(s, dtype=F32)
    bits, inverse = np.unique(s.view(np.uint32).ravel(), return_inverse=True)
    values = np.asarray(prim(bits.view(F32)), dtype=F32)
    assert values.shape == bits.shape
    return values[inverse].reshape(s.shape), len(bits)


def fast_terms(case, prim, pops=None):
    """(n, K, m) float32: the restated float32-mode term of every (individual, population, site), and how many distinct sums there were."""
    v, distinct = through(prim, fast_sums_of(case, pops))
    return np.ascontiguousarray(v.transpose(1, 2, 0)), distinct


def perturbed_log(sign):
    """A primitive as wrong as the measurement allows: the float32 farthest from log s, towards `sign`, that is still within
    fast_log_error of it."""
    def prim(s):
        s64 = np.asarray(s, dtype=F32).astype(np.float64)
        ok = np.isfinite(s64) & (s64 > 0) & (s64 != 1)                   # (fast_log(1) is exactly 0: a matter of class, not of error)
        t = np.log(np.where(ok, s64, 1.0))
        err = fast_log_error(np.where(ok, s64, 1.0), np.where(ok, s64, 1.0))
        v = (t + sign * err).astype(F32)
        too_far = np.abs(v.astype(np.float64) - t) > err
        v = np.where(too_far, np.nextafter(v, t.astype(F32)), v)
        assert (np.abs(v.astype(np.float64) - t) <= err)[ok].all()
        return np.where(ok, v, log_correct(s))
    return prim


# ---- the reference in real arithmetic --------------------------------------------------------------------------------------------------
def real_terms(g0, g1, a):
    """For finite float32 g0, g1, a (broadcast): dict of float64 arrays of the broadcast shape --
    S (the real sum, correctly rounded), sign (of the real sum: exact), kappa (sum |L_j| / S where S > 0, else inf), log (math.log(S)
    where S > 0, else NaN), bound (term_bound), distinct (how many distinct products were evaluated)."""
    g0, g1, a = np.broadcast_arrays(*(np.asarray(x, dtype=F32) for x in (g0, g1, a)))
    shape = g0.shape
    pair = (np.ascontiguousarray(g0).view(np.uint32).astype(np.uint64).ravel() << np.uint64(32)) | np.ascontiguousarray(g1).view(np.uint32).astype(np.uint64).ravel()
    upair, pinv = np.unique(pair, return_inverse=True)
    ua, ainv = np.unique(np.ascontiguousarray(a).view(np.uint32).ravel(), return_inverse=True)
    ucombo, cinv = np.unique(pinv.astype(np.int64) * len(ua) + ainv, return_inverse=True)
    out = {k: np.empty(len(ucombo)) for k in ("S", "sign", "kappa", "log", "bound")}
    pair_f = [(Fraction(float(np.uint32(p >> np.uint64(32)).view(F32))), Fraction(float(np.uint32(p & np.uint64(0xFFFFFFFF)).view(F32)))) for p in upair]
    a_f = [Fraction(float(x)) for x in ua.view(F32)]
    for j, c in enumerate(ucombo.tolist()):
        (G0, G1), A = pair_f[c // len(ua)], a_f[c % len(ua)]
        L = (G0 * (1 - A) ** 2, 2 * G1 * (1 - A) * A, (1 - G0 - G1) * A ** 2)
        S = L[0] + L[1] + L[2]
        out["S"][j], out["sign"][j] = float(S), (S > 0) - (S < 0)
        if S > 0:
            kappa = float((abs(L[0]) + abs(L[1]) + abs(L[2])) / S)
            out["kappa"][j], out["log"][j] = kappa, math.log(float(S)) if float(S) > 0 else float(math.log(S.numerator) - math.log(S.denominator))
            out["bound"][j] = term_bound(float(S), kappa, abs(float(A)), abs(float(1 - A)))
        else:
            out["kappa"][j], out["log"][j], out["bound"][j] = math.inf, math.nan, math.nan
    res = {k: v[cinv].reshape(shape) for k, v in out.items()}
    res["distinct"] = len(ucombo)
    return res


def term_bound(S, kappa, abs_a, abs_oma, rel_ulps=None):
    """The largest |fast term - log S| of a float32 evaluation of a term with real sum S > 0 and condition number kappa (module
    docstring); inf where the relative error of s may reach 1."""
    under = ETA * ((1 + abs_oma) + (1 + abs_a) + (1 + abs_a) + abs_a * abs_a) * (1 + 2.0 ** -20)
    eps = GAMMA6 * kappa + under / S
    if not eps < 1:
        return math.inf
    through_log = -math.log1p(-eps)
    prim = float(fast_log_error(max(S * (1 - eps), 2.0 ** -149), S * (1 + eps) + 2.0 ** -149, rel_ulps))
    return through_log + prim + REF_ERR * (1 + abs(math.log(S)))


_real = {}


def real_of(shape):
    """real_terms of the `finite` case of a shape, as (m, n, K) arrays: computed once, shared, read-only."""
    if shape not in _real:
        c = sc.case_of("finite", shape)
        r = real_terms(c["L"][:, 0::2, None], c["L"][:, 1::2, None], c["A"][:, None, :])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _real[shape] = r
    return _real[shape]


# the terms of `finite` whose real sum is NOT positive (compared by class, not by bound): computed in exact rational arithmetic
NOT_POSITIVE = {"grid": (8728, 235612), "block": (54960, 4981340), sc.RAGGED: (378, 235612)}
# ... and those with a positive real sum below the float32 subnormals (1e-60, 1e-80), where the underflow term leaves no finite bound:
# the reference and the float32 mode both have a sum of +0 there, and such a term is held to the oracle's class
UNBOUNDED = {"grid": 1629, "block": 10491, sc.RAGGED: 36}

# ---- the class table -------------------------------------------------------------------------------------------------------------------
RESULT_CLASSES = ("finite log", "-inf", "NaN", "+inf")
_RESULT_OF = np.array([0, 0, 0, 1, 1, 2, 2, 3, 2, 2], dtype=np.int8)        # score_cases.S_CLASSES -> what the log of such a sum is


def class_table(case, fast_s=None):
    """dict(terms, same, by_sum {(reference's class of s, float32 mode's): terms} over the terms whose classes of s differ,
    by_result {...} over those whose RESULT classes differ -- the log of the one is finite, -inf, NaN or +inf and of the other is
    not).  fast_s: the float32 mode's sums, when they were not formed by fast_sums_of (a mutation)."""
    ref = sc.classify(sc.sums_of(case))
    fast = sc.classify(fast_sums_of(case) if fast_s is None else fast_s)
    by_sum, by_result = {}, {}
    for r, f in zip(*(x[ref != fast].tolist() for x in (ref, fast))):
        key = (sc.S_CLASSES[r], sc.S_CLASSES[f])
        by_sum[key] = by_sum.get(key, 0) + 1
    rr, fr = _RESULT_OF[ref], _RESULT_OF[fast]
    for r, f in zip(*(x[rr != fr].tolist() for x in (rr, fr))):
        key = (RESULT_CLASSES[r], RESULT_CLASSES[f])
        by_result[key] = by_result.get(key, 0) + 1
    return dict(terms=int(ref.size), same=int((ref == fast).sum()), by_sum=by_sum, by_result=by_result)


def g2_float32(case):
    """g2 as the parent of this file formed it: (1.0f - g0) - g1 in float32 (the first of the mutations)."""
    g0, g1 = case["L"][:, 0::2, None], case["L"][:, 1::2, None]
    return (F32(1.0) - g0) - g1


# ---- the command line's clamp ----------------------------------------------------------------------------------------------------------
def clamp_frequencies(n):
    """The bounds the command line clamps a fitted frequency of n individuals to, 1 / (2 (n + 1)) and its complement, as float32, and
    their float32 neighbours inside."""
    lo, hi = F32(1.0 / (2 * (n + 1))), F32(1.0 - 1.0 / (2 * (n + 1)))
    return np.array([lo, np.nextafter(lo, F32(1)), hi, np.nextafter(hi, F32(0))], dtype=F32)


def valid_pairs():
    """Likelihood pairs with g0, g1 >= 0 and (1 - g0) - g1 >= 0: those of the `finite` families that are, and 4000 six-digit ones."""
    fam = [p for name in sorted(set(sc.IND_CYCLE["finite"])) for p in sc.PAIR_FAMILIES[name]]
    rng = np.random.default_rng(20260313)
    x = np.sort(rng.random((4000, 2)), axis=1)
    rnd = np.stack([np.round(x[:, 0], 6), np.round(x[:, 1] - x[:, 0], 6)], axis=1)
    rnd[:400, 0] = np.round(rnd[:400, 0] * 1e-3, 6)                          # nearly everything on g1, on g2 ...
    rnd[400:800, 1] = np.round(rnd[400:800, 1] * 1e-3, 6)
    p = np.concatenate((np.array(fam, dtype=np.float64), rnd)).astype(F32)
    d = p.astype(np.float64)
    return p[(d[:, 0] >= 0) & (d[:, 1] >= 0) & ((1.0 - d[:, 0]) - d[:, 1] >= 0)]


# ======================================================================================================================================
# The float32 EM sweeps (csrc/em_kernels.hip: term_fast in em_sweep_kernel<FAST> and em_sweep_group_kernel<FAST>; EMBatch(mode=MODE_FAST),
# WGSASSIGN_EM_MODE=fast) on the enumerated cells of tests/em_cases.py.
#
# THE RESTATEMENT.  fast_update: for one SNP and the individuals of a fit in slab column order,
#     omf = 1 - f;  p0 = (g0 * omf) * omf;  p1 = (g1 * (2 f)) * omf;  p2 = (g2 * f) * f          g2 = g2_rounded(g0, g1)
#     s = (p0 + p1) + p2;  num = p1 + 2 p2;  d = 2 s;  k = 2^32 if |d| < 2^-126 else 1
#     tmp = tmp + (num * k) * fast_rcp(d * k)                                                    serially, from +0
#     f_new = tmp / (float)n_eff
# in IEEE float32, fast_rcp (csrc/fast_math.h: v_rcp_f32) handed in as a function.
#
# THE REFERENCE.  real_update: F = (1 / n) sum_i Num_i / (2 S_i) in real arithmetic from the float32 inputs, with fractions.Fraction on
# the distinct (pair, frequency) products.  A (fit, site) is compared by bound when every one of its terms has S > 0.
#
# THE BOUND.  update_bound, with u = 2^-24 and P0, P1, P2 the real products of a term:
#   * p1 and p2 carry three roundings each (omf or g2, two products; 2 f and 2 p2 are exact), p0 four, so the numerator, one addition
#     more, is off by at most gamma_4 (|P1| + 2 |P2|) and the sum, two additions more, by gamma_6 sum_j |P_j|, plus 2^-150 per
#     product that can underflow;
#   * the scalings by k and by 2 are exact; fast_rcp is within FAST_RCP_REL_ULPS ulps, i.e. 2^-23 times that, of the reciprocal of
#     its NORMAL argument (the scaling keeps it normal; results stay normal while d * k < 2^126), and the product with it rounds once
#     more: rho = (1 + FAST_RCP_REL_ULPS 2^-23)(1 + u) - 1;
#   * so a term's quotient q^ is within  e_i = [ dN / (2 S) + |q| eps ] / (1 - eps) (1 + rho) + |q| rho + 2^-150  of q = Num / (2 S),
#     eps = dS / S (no bound where eps >= 1);
#   * the serial float32 sum of n addends is within gamma_(n-1) sum |q^_i| of their real sum, and the divide adds u |F| + 2^-150.
# ======================================================================================================================================
import em_cases as ec  # noqa: E402

GAMMA4 = 4 * U / (1 - 4 * U) + 2.0 ** -50
RHO = (1 + FAST_RCP_REL_ULPS * 2.0 ** -23) * (1 + U) - 1


def fast_quotients(g0, g1, f, rcp, scale=True, g2=None):
    """(q^ float32, distinct reciprocal arguments): the addend of term_fast for float32 g0, g1, f (broadcast)."""
    g0, g1, f = np.broadcast_arrays(*(np.asarray(x, dtype=F32) for x in (g0, g1, f)))
    g2 = g2_rounded(g0, g1) if g2 is None else np.asarray(g2, dtype=F32)
    one, two = F32(1.0), F32(2.0)
    with np.errstate(all="ignore"):
        omf, f2 = one - f, two * f
        p0 = (g0 * omf) * omf
        p1 = (g1 * f2) * omf
        p2 = (g2 * f) * f
        s = (p0 + p1) + p2
        num = p1 + two * p2
        d = two * s
        k = np.where(np.abs(d) < F32(TINY), F32(2.0 ** 32), one).astype(F32) if scale else np.ones_like(d)
        r, distinct = through(rcp, d * k)
        q = (num * k) * r
    assert q.dtype == F32
    return q, distinct


def fast_update(L_pop, f_old, rcp, skip=None, **how):
    """(m,) float32: one float32-mode update of a fit from L_pop (m, 2 c), its individuals in slab column order, without column `skip`."""
    q, _ = fast_quotients(L_pop[:, 0::2], L_pop[:, 1::2], np.asarray(f_old, dtype=F32)[:, None], rcp, **how)
    tmp = np.zeros(L_pop.shape[0], dtype=F32)
    cols = [c for c in range(q.shape[1]) if c != skip]
    with np.errstate(all="ignore"):
        for c in cols:
            tmp = tmp + q[:, c]
        return tmp / F32(len(cols))


def rcp_correct(x):
    with np.errstate(all="ignore"):
        return (1.0 / np.asarray(x, dtype=F32).astype(np.float64)).astype(F32)


def rcp_perturbed(sign):
    """A reciprocal as wrong as the measurement allows on normal arguments with normal results."""
    def prim(x):
        x64 = np.asarray(x, dtype=F32).astype(np.float64)
        with np.errstate(all="ignore"):
            t = 1.0 / x64
            ok = np.isfinite(t) & (np.abs(x64) >= TINY) & (np.abs(t) >= TINY)
            err = FAST_RCP_REL_ULPS * ulp32(np.where(ok, t, 1.0))
            v = (t + sign * err).astype(F32)
            v = np.where(np.abs(v.astype(np.float64) - t) > err, np.nextafter(v, t.astype(F32)), v)
        return np.where(ok, v, rcp_correct(x))
    return prim


def real_quotients(g0, g1, f):
    """For finite float32 g0, g1, f (broadcast): dict of float64 arrays -- q (Num / (2 S), correctly rounded; NaN where S <= 0), sign (of
    S), err (the bound e_i of a float32 evaluation of the term; inf where there is none), distinct."""
    g0, g1, f = np.broadcast_arrays(*(np.asarray(x, dtype=F32) for x in (g0, g1, f)))
    shape = g0.shape
    key = (np.ascontiguousarray(g0).view(np.uint32).astype(np.uint64).ravel() << np.uint64(32)) | np.ascontiguousarray(g1).view(np.uint32).astype(np.uint64).ravel()
    upair, pinv = np.unique(key, return_inverse=True)
    uf, finv = np.unique(np.ascontiguousarray(f).view(np.uint32).ravel(), return_inverse=True)
    ucombo, cinv = np.unique(pinv.astype(np.int64) * len(uf) + finv, return_inverse=True)
    out = {k: np.empty(len(ucombo)) for k in ("q", "sign", "err")}
    pair_f = [(Fraction(float(np.uint32(p >> np.uint64(32)).view(F32))), Fraction(float(np.uint32(p & np.uint64(0xFFFFFFFF)).view(F32)))) for p in upair]
    f_f = [Fraction(float(x)) for x in uf.view(F32)]
    for j, c in enumerate(ucombo.tolist()):
        (G0, G1), Fq = pair_f[c // len(uf)], f_f[c % len(uf)]
        P = (G0 * (1 - Fq) ** 2, 2 * G1 * Fq * (1 - Fq), (1 - G0 - G1) * Fq ** 2)
        S, Num = P[0] + P[1] + P[2], P[1] + 2 * P[2]
        out["sign"][j] = (S > 0) - (S < 0)
        if S > 0:
            q = Num / (2 * S)
            out["q"][j] = float(q)
            out["err"][j] = quotient_bound(float(S), float(abs(P[0]) + abs(P[1]) + abs(P[2])), float(abs(P[1]) + 2 * abs(P[2])), abs(float(q)), abs(float(Fq)), abs(float(1 - Fq)))
        else:
            out["q"][j], out["err"][j] = math.nan, math.inf
    res = {k: v[cinv].reshape(shape) for k, v in out.items()}
    res["distinct"] = len(ucombo)
    return res


def quotient_bound(S, Sabs, Nabs, q_abs, abs_f, abs_omf):
    """e_i of the derivation above; inf where the float32 sum may be off by all of S."""
    under_s = ETA * ((1 + abs_omf) + (1 + abs_omf) + (1 + abs_f) + abs_f * abs_f) * (1 + 2.0 ** -20)
    under_n = ETA * ((1 + abs_omf) + 2 * (1 + abs_f) + 2 * abs_f * abs_f) * (1 + 2.0 ** -20)
    eps = (GAMMA6 * Sabs + under_s) / S
    if not eps < 1:
        return math.inf
    d_num = GAMMA4 * Nabs + under_n
    return (d_num / (2 * S) + q_abs * eps) / (1 - eps) * (1 + RHO) + q_abs * RHO + ETA + REF_ERR * q_abs


def update_bound(q, err):
    """(m,) the bound of one float32-mode update against the real-arithmetic one, from the real quotients q (m, n) of its terms and their
    bounds err (m, n): the terms' own errors, the serial float32 sum of n addends, the final divide."""
    n = q.shape[1]
    gamma_n = (n - 1) * U / (1 - (n - 1) * U) if n > 1 else 0.0
    with np.errstate(all="ignore"):
        mags = (np.abs(q) + err).sum(axis=1)
        F = np.abs(q.sum(axis=1)) / n
        return (err.sum(axis=1) + gamma_n * mags) / n * (1 + U) + U * F + ETA + REF_ERR * F


_em_real = {}


def em_real_of(k, skip=None):
    """(F (m,) the real-arithmetic first update of population k of em_cases' `finite` grid from its enumerated frequencies, without slab
    column `skip`; bound (m,); compared (m,) bool: every term of the site has S > 0 and a bound).  Computed once, shared."""
    key = (k, skip)
    if key not in _em_real:
        grid = ec.grid_of("finite")
        mem = grid["members"][k] if skip is None else np.delete(grid["members"][k], skip)
        r = real_quotients(grid["L"][:, 2 * mem], grid["L"][:, 2 * mem + 1], grid["f_old"][k][:, None])
        compared = (r["sign"] > 0).all(axis=1) & np.isfinite(r["err"]).all(axis=1)
        q, err = np.where(compared[:, None], r["q"], 0.0), np.where(compared[:, None], r["err"], 0.0)
        _em_real[key] = (q.sum(axis=1) / len(mem), update_bound(q, err), compared)
    return _em_real[key]


# (compared (fit, site), all of them, enumerated cells that qualify) of em_cases' `finite` grid: computed in exact rational arithmetic
EM_COMPARED = (6539, 9220, 6688)
