"""Lifetimes of the C ABI's objects (commit 640d6da): a matrix destroyed before the EM batches and scores made from it, a second
destroy, objects released by Python's cycle collector in whatever order it picks, and objects still alive at interpreter exit.

The library keeps a registry of live children (csrc/api.hip: wgs_live_*): destroying a matrix destroys its EM batches and scores,
destroying a frequency set destroys its scores, and destroying any of those afterwards is a no-op (include/wgsassign_hip.h).  Each
scenario runs once, in a fresh Python process, so that a regression fails one test rather than the pytest process."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_PRELUDE = r'''
import faulthandler
import sys
faulthandler.enable()
sys.path[:0] = [@ROOT@, @TESTS@]
import numpy as np
import synth
from oracle import oracle as orc
from wgsassign_amd import device
m, n, K = 10_000, 40, 2
L, IDs = synth.make_beagle(m, n, K, seed=17)
pops = np.unique(IDs[:, 1])
group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
_, af_o, _, iters_o = orc.fit_reference_af(L, IDs, t=4)
'''

_THROUGH_CTYPES = _PRELUDE + r'''
import ctypes
from wgsassign_amd import _lib
from wgsassign_amd._lib import MODE_EXACT, check, f32p, i32p
lib = _lib.load()
ctx = device.get_context()


def beagle():
    h = ctypes.c_void_p()
    check(lib.wgs_beagle_create(ctx.handle, m, n, i32p(group_of), K, 0, ctypes.byref(h)))
    check(lib.wgs_beagle_upload_rows(h, f32p(L), 0, m))
    return h


def em_batch(b, groups, skips):
    h = ctypes.c_void_p()
    g, s = np.array(groups, dtype=np.int32), np.array(skips, dtype=np.int32)
    check(lib.wgs_em_create(b, len(g), i32p(g), i32p(s), MODE_EXACT, ctypes.byref(h)))
    return h


def score(b, a):
    h = ctypes.c_void_p()
    check(lib.wgs_score_create(b, a, None, 0, n, ctypes.byref(h)))
    return h


def in_use(b):
    """wgs_beagle_set_rows refuses a matrix that has live EM batches or scores (at the same size it changes nothing)."""
    rc = lib.wgs_beagle_set_rows(b, m)
    assert rc == 0 or "in use" in _lib.last_error(), _lib.last_error()
    return rc != 0


a = ctypes.c_void_p()
check(lib.wgs_afset_create(ctx.handle, m, K, ctypes.byref(a)))
check(lib.wgs_afset_upload(a, f32p(np.ascontiguousarray(af_o))))
# a matrix with a leave-one-out EM batch (one step taken) and a score (summed) made from it
b = beagle()
em = em_batch(b, [0, 0, 1], [0, 7, 25])
check(lib.wgs_em_step(em, None))
sc = score(b, a)
out = np.zeros((n, K))
check(lib.wgs_score_sums(sc, MODE_EXACT, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
assert in_use(b)
assert lib.wgs_beagle_set_rows(b, m - 64) != 0 and "in use" in _lib.last_error(), _lib.last_error()
# the matrix takes both with it; destroying them afterwards, and the batch a second time, does nothing (nothing is created between)
lib.wgs_beagle_destroy(b)
lib.wgs_em_destroy(em)
lib.wgs_score_destroy(sc)
lib.wgs_em_destroy(em)
check(lib.wgs_ctx_sync(ctx.handle))
print("parent before children: ok", flush=True)
# a frequency set destroyed while a score over it and another, live matrix exists: the score goes, the matrix stays usable
b2 = beagle()
sc2 = score(b2, a)
assert in_use(b2)
lib.wgs_afset_destroy(a)
assert not in_use(b2)                      # the registry no longer lists a score over b2
lib.wgs_score_destroy(sc2)
check(lib.wgs_ctx_sync(ctx.handle))
print("frequency set before its score: ok", flush=True)
# afterwards: a new matrix and fit equal the oracle
b3 = beagle()
em3 = em_batch(b3, [0, 1], [-1, -1])
iters = np.zeros(K, dtype=np.int32)
check(lib.wgs_em_fit(em3, 200, 1e-4, m, None, 0.0, i32p(iters)))
assert list(iters) == list(iters_o), (iters, iters_o)
counts = np.bincount(group_of, minlength=K)
for k in range(K):
    lo = 1 / (2 * (int(counts[k]) + 1))
    check(lib.wgs_em_clamp(em3, k, np.float32(lo), np.float32(1 - lo)))
    f = np.empty(m, dtype=np.float32)
    check(lib.wgs_em_get_f(em3, k, f32p(f)))
    assert f.tobytes() == np.ascontiguousarray(af_o[:, k]).tobytes(), k
lib.wgs_em_destroy(em3)
lib.wgs_beagle_destroy(b3)
lib.wgs_beagle_destroy(b2)
print("OK", flush=True)
'''

_THROUGH_PYTHON = _PRELUDE + r'''
import gc


def make_and_fail():
    b = device.DeviceBeagle.from_host(L, group_of, K)
    em = device.EMBatch(b, [0, 0, 1], [0, 7, 25])
    em.step()
    afs = device.AFSet.from_host(np.ascontiguousarray(af_o))
    sc = device.Score(b, afs)
    sc.sums()
    raise RuntimeError("a failed check with the device objects in its frame")


def caller():
    try:
        make_and_fail()
    except RuntimeError as e:
        kept = e                   # the traceback holds this frame, whose `kept` holds the traceback: a reference cycle
        return kept


gc.disable()
err = caller()
del err
assert len(device._live) == 4      # only the cycle holds the matrix, its EM batch, the frequency set and the score ...
gc.collect()                       # ... which the collector releases, in its own order
assert len(device._live) == 0
print("collected: ok", flush=True)
# the same objects once more, left alive for the interpreter's exit (device.py: _close_all)
b = device.DeviceBeagle.from_host(L, group_of, K)
em = device.EMBatch(b, [0, 1])
iters = em.run(200, 1e-4)
assert list(iters) == list(iters_o), (iters, iters_o)
afs = device.AFSet.from_host(np.ascontiguousarray(af_o))
sc = device.Score(b, afs)
sc.sums()
print("OK", flush=True)
'''


@pytest.mark.parametrize("scenario", ["through_ctypes", "through_python"])
def test_objects_outlive_or_follow_their_parents(tmp_path, scenario):
    script = tmp_path / ("lifetime_%s.py" % scenario)
    body = _THROUGH_CTYPES if scenario == "through_ctypes" else _THROUGH_PYTHON
    script.write_text(body.replace("@ROOT@", repr(ROOT)).replace("@TESTS@", repr(os.path.join(ROOT, "tests"))))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=180, cwd=ROOT)
    tail = "exit status %d\nstdout:\n%s\nstderr:\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, tail
    assert r.stdout.strip().splitlines()[-1] == "OK", tail
    assert "Segmentation fault" not in r.stderr and "Fatal Python error" not in r.stderr, tail
