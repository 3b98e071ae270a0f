"""Enumerated inputs for the ORDER of np.sum over a contiguous float32 array, and a Python twin of that order, for the sums that
--get_assignment_z_score continues from site window to site window on the device (csrc/zscore_kernels.hip: zsum_chunk_kernel,
zsum_close_kernel; csrc/zscore_api.hip: wgs_zsum_push, wgs_zsum_finish).  NumPy and the standard library only.

THE ORDER.  np.sum(a) and np.sum(a, dtype=np.float32) of a contiguous float32 array add the sums of consecutive CHUNK = 8192 element
chunks (np.getbufsize()) serially to a float32 that starts at +0.0; a chunk goes through NumPy's pairwise routine (`pairwise`):
n < 8 serial from 0; n <= 128 eight strided accumulators closed as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the
remainder serially; otherwise split at n / 2 rounded down to a multiple of 8.  A full chunk is therefore a balanced tree over 64
leaves of 128 elements, whatever the array's length: the sum can be continued from push to push (`Continued`, what the device does)
with the running float32 and the fewer than 8192 elements of the open chunk as its state.  tests/test_zsum_cases_cpu.py holds both to
np.sum of the installed NumPy bit for bit.

THE INPUTS follow tests/order_cases.py: three magnitude classes -- big [16, 32), mid [8, 16), small [2^-19, 2^-13) -- in runs of 1 to
300 elements, every mantissa random, all of one sign (per-site log-likelihoods are): nearly every float32 addition rounds, so another
order is another number.  SPECIALS: NaN, +-inf, -0.0 only (np.sum gives +0.0), and cancellation to +0.0.

THE WRONG ORDERS a plausible bug would compute: one pairwise tree over the whole array, the plain serial sum, and chunks that
restart at every push (the chunk edges counted from the push's first element instead of the array's)."""
import numpy as np

F32 = np.float32
CHUNK = 8192
CPU_LENGTHS = tuple(range(300)) + (1000, 1023, 1025, 4097, 8191, 8192, 8193, 16384, 16385, 24577, 100003, 300007)
GPU_LENGTHS = (0, 1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 16384, 16385, 24577, 3 * 8192 + 5003)
GROUP = 5                                  # individuals of one device state: five DIFFERENT lengths
CUTS = ("one", "1000", "8191", "8192", "8193", "empty", "8191+1")
CLASS_RANGE = ((16.0, 32.0), (8.0, 16.0), (2.0 ** -19, 2.0 ** -13))
SEED = 20240611
# (length, seed) of the arrays the orders are told apart on: final roundings coincide often (the last few additions decide), so the
# seeds are those at which np.sum ITSELF differs from every wrong order -- found by trying seeds 1, 2, ... against NumPy, not against
# the device.  At 16384 elements one pairwise tree IS np.sum's order (two full chunks), whatever the data.
ORDER_SEEDS = {8193: (3, 6), 16384: (2, 3), 16385: (1, 11), 24577: (12, 14), 3 * 8192 + 5003: (4, 6), 100003: (2, 4), 300007: (1, 2)}


def values(n, seed):
    """n float32 of the three classes in runs, negative."""
    rng = np.random.default_rng([SEED, int(seed), int(n)])
    cls = np.empty(n, dtype=np.int64)
    at = 0
    while at < n:
        run = int(rng.integers(1, 301))
        cls[at:at + run] = rng.integers(0, 3)
        at += run
    lo = np.array([r[0] for r in CLASS_RANGE])[cls]
    x = -(lo * (1.0 + rng.random(n)))                     # [lo, 2 lo): the class's binade(s)
    return np.ascontiguousarray(x.astype(F32))


def specials():
    """name -> float32 array: what np.sum must be matched on beyond finite sums (NaN for NaN)."""
    n = CHUNK + 777
    base = values(n, 99)
    nan = base.copy()
    nan[CHUNK // 2] = np.nan
    pinf = base.copy()
    pinf[5] = np.inf
    ninf = base.copy()
    ninf[CHUNK + 3] = -np.inf
    both = pinf.copy()
    both[CHUNK + 9] = -np.inf                              # +inf in the running value, -inf in the tail: NaN
    mzero = np.full(n, -0.0, dtype=F32)
    mzero_short = np.full(5, -0.0, dtype=F32)
    cancel = np.tile(np.array([1.5, -1.5], dtype=F32) * F32(2.0 ** 20), n // 2 + 1)[:n - 1]      # every accumulator of one sign: exact
    return {"nan": nan, "+inf": pinf, "-inf": ninf, "inf-inf": both, "-0.0": mzero, "-0.0 short": mzero_short, "cancel": cancel}


# ---- the order ---------------------------------------------------------------------------------------------------------------------------
def pairwise(a):
    """NumPy's pairwise_sum for float32 (one call: a chunk of at most 8192 elements inside np.sum, or a whole array in WRONG_ORDERS)."""
    n = a.size
    if n < 8:
        res = F32(0.0)
        for x in a:
            res = F32(res + x)
        return res
    if n <= 128:
        r = a[:8].astype(F32)
        whole = n - n % 8
        for i in range(8, whole, 8):
            r = r + a[i:i + 8]
        res = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
        for x in a[whole:]:
            res = F32(res + x)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F32(pairwise(a[:n2]) + pairwise(a[n2:]))


def full_chunk(a):
    """A full chunk as the device reduces it: 64 leaves of 128, then the balanced tree level by level -- `pairwise` of 8192 elements,
    written the other way round."""
    assert a.size == CHUNK
    r = a.reshape(64, 16, 8)[:, 0, :].astype(F32)
    for i in range(1, 16):
        r = r + a.reshape(64, 16, 8)[:, i, :]
    node = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    while node.size > 1:
        node = node[0::2] + node[1::2]
    return F32(node[0])


def numpy_order(a):
    """The claim: np.sum(a) of a contiguous float32 array."""
    with np.errstate(invalid="ignore", over="ignore"):
        res = F32(0.0)
        for c in range(0, a.size, CHUNK):
            res = F32(res + pairwise(a[c:c + CHUNK]))
        return res


class Continued:
    """The device's state machine for one (individual, array): push after push, then finish (the host closes the ragged chunk with
    np.sum of the tail -- here with the twin, so that the CPU test checks the whole route against np.sum)."""

    def __init__(self):
        self.run, self.tail = F32(0.0), np.empty(0, dtype=F32)

    def push(self, x):
        with np.errstate(invalid="ignore", over="ignore"):
            buf = np.concatenate((self.tail, np.asarray(x, dtype=F32)))
            nfull = buf.size // CHUNK
            for c in range(nfull):
                self.run = F32(self.run + full_chunk(buf[c * CHUNK:(c + 1) * CHUNK]))
            self.tail = buf[nfull * CHUNK:]

    def finish(self, tail_sum=numpy_order):
        with np.errstate(invalid="ignore", over="ignore"):
            return F32(self.run + tail_sum(self.tail)) if self.tail.size else self.run


def close(run, tail):
    """What zscore.py does with a downloaded state: run + np.sum(tail), nothing for an empty tail."""
    with np.errstate(invalid="ignore", over="ignore"):
        return F32(F32(run) + np.sum(tail)) if tail.size else F32(run)


# ---- the cuts of an array of n elements into pushes ---------------------------------------------------------------------------------------
def cut(n, how):
    """The lengths of the pushes (they add up to n)."""
    def every(step):
        out = [step] * (n // step)
        return out + ([n % step] if n % step or not out else [])
    if how == "one":
        return [n]
    if how in ("1000", "8191", "8192", "8193"):
        return every(int(how))
    if how == "empty":
        return [n // 2, 0, n - n // 2]
    if how == "8191+1":                                    # the open chunk stands at 8191, then one element closes it
        first = min(n, CHUNK - 1)
        second = min(n - first, 1)
        return [first, second, n - first - second]
    raise ValueError(how)


def pieces(a, how):
    out, at = [], 0
    for k in cut(a.size, how):
        out.append(a[at:at + k])
        at += k
    assert at == a.size
    return out


# ---- the wrong orders ----------------------------------------------------------------------------------------------------------------------
def whole_tree(a):
    with np.errstate(invalid="ignore", over="ignore"):
        return F32(F32(0.0) + pairwise(a))


def serial(a):
    with np.errstate(invalid="ignore", over="ignore"):
        return F32(np.cumsum(a, dtype=F32)[-1]) if a.size else F32(0.0)


def restart_at_push(a, how="1000"):
    """Every push summed chunk by chunk from ITS first element onto the running value."""
    with np.errstate(invalid="ignore", over="ignore"):
        res = F32(0.0)
        for p in pieces(a, how):
            for c in range(0, p.size, CHUNK):
                res = F32(res + pairwise(p[c:c + CHUNK]))
        return res


WRONG_ORDERS = {"one pairwise tree over the whole array": whole_tree, "the plain serial sum": serial,
                "chunks restart at every push (pushes of 1000)": restart_at_push}


def same(a, b):
    """Bit for bit, and NaN for NaN."""
    a, b = F32(a), F32(b)
    return bool((np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes())


# ---- the device groups: five individuals of different lengths in one state, three arrays each ------------------------------------------------
def groups():
    """[(lengths of the five individuals)]: GPU_LENGTHS dealt so that every group mixes short and long arrays."""
    L = list(GPU_LENGTHS)
    return [tuple(L[g::len(L) // GROUP]) for g in range(len(L) // GROUP)]


def group_arrays(lengths):
    """arrays[j][a]: the three arrays of individual j (length lengths[j]); beyond 8192 elements the first two are the arrays of
    ORDER_SEEDS, on which np.sum differs from every wrong order."""
    def seed(j, a, n):
        return ORDER_SEEDS[n][a] if n in ORDER_SEEDS and a < 2 else 100 + 10 * j + a
    return [[values(n, seed(j, a, n)) for a in range(3)] for j, n in enumerate(lengths)]


def pushes_of(arrays, how):
    """The pushes of a group as the device takes them: a list of (kept (count,) int64, host (3, all) float32); individuals whose cut has
    fewer pushes than the longest one's push nothing at the end."""
    cuts = [pieces(arr[0], how) for arr in arrays]
    rounds = max(len(c) for c in cuts)
    at = [0] * len(arrays)
    out = []
    for r in range(rounds):
        kept = np.array([c[r].size if r < len(c) else 0 for c in cuts], dtype=np.int64)
        host = np.empty((3, int(kept.sum())), dtype=F32)
        o = 0
        for j, arr in enumerate(arrays):
            for a in range(3):
                host[a, o:o + kept[j]] = arr[a][at[j]:at[j] + kept[j]]
            o += int(kept[j])
            at[j] += int(kept[j])
        out.append((kept, host))
    return out
