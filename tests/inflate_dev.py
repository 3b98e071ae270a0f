"""What the device-inflate tests share (tests/test_gpu_inflate.py, tests/test_gpu_inflate_streams.py): zlib as an encoder, and the
driver of the `wgs_debug_inflate` hook -- streams at a chosen input alignment, output slots between guard bytes."""
import ctypes
import zlib

import numpy as np

GUARD = 64
PAD_BYTE = 0x5A         # between streams that are moved to an alignment: not zero, as in a file (a trailer, the next header)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=-15):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return co.compress(data) + co.flush()


class Launch:
    """One launch of the inflate kernel: `out` is the whole output buffer (zeroed by the hook before the kernel runs), slot i at
    out_off[i] with `guard` bytes before and after it."""

    def __init__(self, streams, sizes, in_align=None, guard=0):
        from wgsassign_amd import _lib, device
        ctx = device.get_context()
        n = len(streams)
        in_len = np.array([len(s) for s in streams], dtype=np.uint32)
        if in_align is None:
            comp = b"".join(streams)
            in_off = np.concatenate([[0], np.cumsum(in_len[:-1], dtype=np.uint64)]).astype(np.uint64) if n else np.zeros(0, np.uint64)
        else:
            # every stream starts at in_align (mod 8): BGZF members start behind an 18-byte header, at any alignment
            parts, at, offs = [], 0, []
            for s in streams:
                pad = (in_align - at) % 8
                parts.append(bytes([PAD_BYTE]) * pad)
                offs.append(at + pad)
                parts.append(s)
                at += pad + len(s)
            comp = b"".join(parts)
            in_off = np.array(offs, dtype=np.uint64)
        isize = np.array(sizes, dtype=np.uint32)
        ends = np.cumsum(isize.astype(np.uint64) + np.uint64(guard), dtype=np.uint64)
        out_off = (ends - isize.astype(np.uint64)).astype(np.uint64) if n else np.zeros(0, np.uint64)
        total = int(ends[-1]) + guard if n else 0
        out = np.zeros(max(total, 1), dtype=np.uint8)
        status = np.full(max(n, 1), 9, dtype=np.uint8)
        cbuf = np.frombuffer(comp + b"\0", dtype=np.uint8).copy()
        ms = ctypes.c_float()
        _lib.check(_lib.load().wgs_debug_inflate(ctx.handle, cbuf.ctypes.data, len(comp), in_off.ctypes.data, in_len.ctypes.data,
                                                 out_off.ctypes.data, isize.ctypes.data, n, out.ctypes.data, total, status.ctypes.data,
                                                 ctypes.byref(ms)))
        self.out, self.out_off, self.isize, self.status, self.ms, self.in_off, self.guard = out, out_off, isize, status[:n], ms.value, in_off, guard

    def slots(self):
        return [self.out[int(o):int(o) + int(s)].tobytes() for o, s in zip(self.out_off, self.isize)]


def device_inflate(streams, sizes, in_align=None, guard=0):
    r = Launch(streams, sizes, in_align, guard)
    return r.slots(), r.status, r.ms


def check_launch(cases, in_align, guard=GUARD, limit=12):
    """Runs cases [(stream, isize, expected bytes | None, label)] as ONE launch (64 consecutive cases are one wavefront) and
    returns what is wrong, as a list of strings: a case with expected bytes must come out with status 0 and those bytes, a case
    without must be refused (whatever its slot holds), and every guard byte must still be zero -- the data never holds a zero."""
    r = Launch([c[0] for c in cases], [c[1] for c in cases], in_align, guard)
    want = np.zeros_like(r.out)
    got = r.out.copy()
    wrong = []
    for i, (_, isize, expected, label) in enumerate(cases):
        o = int(r.out_off[i])
        if expected is None:
            got[o:o + isize] = 0
            if r.status[i] == 0:
                wrong.append("%s: accepted (status 0), must be refused" % label)
        else:
            assert len(expected) == isize, label
            want[o:o + isize] = np.frombuffer(expected, dtype=np.uint8)
            if r.status[i] != 0:
                wrong.append("%s: refused (status %d), is valid" % (label, r.status[i]))
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        slot = np.searchsorted(r.out_off, at, side="right") - 1
        seen = set()
        for a, s in zip(at.tolist(), slot.tolist()):
            inside = s >= 0 and a < int(r.out_off[s]) + int(r.isize[s])
            key = (s, inside)
            if key in seen:
                continue
            seen.add(key)
            if inside:
                wrong.append("%s: byte %d of %d is %d, expected %d" % (cases[s][3], a - int(r.out_off[s]), int(r.isize[s]), got[a], want[a]))
            else:
                wrong.append("guard byte written %d bytes behind the slot of %s" % (a - int(r.out_off[s]) - int(r.isize[s]), cases[max(s, 0)][3]))
    return ["in_off %% 8 = %s, %d streams: %d wrong" % (in_align, len(cases), len(wrong))] + wrong[:limit] if wrong else []
