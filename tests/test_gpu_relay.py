"""GPU: the relay that hands running values from SNP shard to SNP shard (csrc/common.h: wgs_relay), through every library call built
on it.  Three ranks share the one GPU over the socket transport (the harness of tests/test_gpu_multirank.py) -- three, because only
a middle rank both receives and sends.  m = 3 x 8192 + 100 sites: every shard starts on the 8192-site alignment and the last is
ragged; 12 individuals in 3 populations, 3 partitions; the guard floor at 1e9, so that every convergence test of every fit is
decided by the chain.  Individual HOLLOW has depth 0 throughout the middle shard: the middle rank hands its class sums and its chain
carry on untouched.  Every output is compared bit for bit with a one-process run over the whole matrix, and every relayed call's
collectives are counted (wgs_comm_stats before and after): `world` broadcasts per relay, of the bytes the call's shapes imply."""
import os
import pickle
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

WORLD, M, N, K, P, HOLLOW = 3, 3 * 8192 + 100, 12, 3, 3, 5

_WORKER = r'''
import contextlib, ctypes, io, os, pickle, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import synth_depth
from wgsassign_amd import _lib, device, emMAF, zscore
from wgsassign_amd._lib import check, f32p, i32p
from wgsassign_amd.comm import SocketComm, shard_range
rank, world, out_path = int(sys.argv[1]), {world}, sys.argv[2]
m, n, K, P, hollow = {m}, {n}, {K}, {P}, {hollow}
device.EMBatch.GUARD = 1e9                                  # every convergence test goes to the exact chain
comm = SocketComm(rank, world, "127.0.0.1", {port}, timeout=60.0)
L, AD, IDs, _ = synth_depth.make_depth(m, n, K, seed=19, depth=1.5, sizes=(4, 4, 4))
cuts = [shard_range(m, r, world)[0] for r in range(world)] + [m]
assert cuts == [0, 8192, 16384, m]
AD = AD.copy()
AD[cuts[1]:cuts[2], 2 * hollow:2 * hollow + 2] = 0         # depth 0 never survives the key filter: nothing kept in the middle shard
lo, hi = cuts[rank], cuts[rank + 1]
pops = np.unique(IDs[:, 1])
group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
ctx = device.Context(0)
comm.attach(ctx)
lib = _lib.load()

def stats():
    st = (ctypes.c_int64 * 4)()
    check(lib.wgs_comm_stats(comm.handle, st))
    return np.array(st[:])                                  # all-reduces, broadcasts, payload bytes, host round trips

log = []                                                    # (relayed call, what it added to the communicator's counts)
def counted(name):
    fn = getattr(lib, name)
    def call(*a):
        before = stats()
        rc = fn(*a)
        log.append((name, (stats() - before).tolist()))
        return rc
    setattr(lib, name, call)

def classes(depth, handle):
    cnt = np.zeros((n, zscore.N_CLASSES), dtype=np.int32)
    sums = np.zeros((n, zscore.N_CLASSES, 3), dtype=np.float32)
    if handle is None:
        first, over = np.zeros((n, zscore.N_CLASSES), dtype=np.int32), np.zeros(n, dtype=np.int32)
        check(lib.wgs_zscore_classes(depth.handle, 0, n, i32p(cnt), f32p(sums), i32p(first), i32p(over)))
    else:
        first, over = np.zeros((n, zscore.N_CLASSES), dtype=np.int64), np.zeros((world, n), dtype=np.int32)
        check(lib.wgs_zscore_classes_sharded(depth.handle, 0, n, handle, i32p(cnt), f32p(sums),
                                             first.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), i32p(over)))
    seen = cnt > 0
    return cnt, np.where(seen, first, -1).astype(np.int64), np.where(seen[:, :, None], sums, np.float32(0)), over

def everything(Lp, ADp, site0, c):
    """Every relayed call over the rows given: the whole matrix (c None), or this rank's shard."""
    res, said = {{}}, []
    with contextlib.redirect_stdout(io.StringIO()):
        b = device.DeviceBeagle.from_host(np.ascontiguousarray(Lp), group_of, K, site0=site0, ctx=ctx)
        _, af, iters = emMAF.emMAF_populations(None, IDs, 200, 1e-4, beagle=b, comm=c)
        res["af"], res["iters"], res["fit_stats"] = af, np.asarray(iters), emMAF.emMAF_populations.last_stats[:2]
        afs = device.AFSet.from_host(np.ascontiguousarray(af), ctx=ctx)
        res["sums"], _ = device.assign(b, afs, comm=c)
        res["parts"] = device.partition_sums_exact(b, afs, None, P, c)
        depth = zscore.DepthTable(b, np.ascontiguousarray(ADp), chunk_rows=1000)
        res["cnt"], res["first"], res["csums"], over = classes(depth, c.handle if c is not None else None)
        assert not over.any()
        details = []
        res["z"] = zscore.reference_z_scores(b, depth, IDs, group_of, 200, 1e-4, 0, False, 0, n, say=said.append, details=details, comm=c)
        res["masked_iters"] = [int(s.rsplit(" ", 1)[1]) for s in said if s.startswith("EM (MAF) converged")]
        res["keep"] = [d["keep"] for d in details]
        res["it"] = [d["it"] for d in details]
        depth.close(); afs.close(); b.close()
    return res

whole = everything(L, AD, 0, None)
for name in ("wgs_em_fit", "wgs_score_totals_all", "wgs_score_chains_walk_all", "wgs_zscore_classes_sharded", "wgs_em_fit_masked_sharded"):
    counted(name)
mine = everything(L[lo:hi], AD[lo:hi], lo, comm)
same = dict(af=mine["af"].tobytes() == np.ascontiguousarray(whole["af"][lo:hi]).tobytes(),
            iters=mine["iters"].tolist() == whole["iters"].tolist(),
            masked_iters=mine["masked_iters"] == whole["masked_iters"])
for k in ("sums", "parts", "cnt", "first", "csums"):
    same[k] = mine[k].dtype == whole[k].dtype and mine[k].tobytes() == whole[k].tobytes()
if rank == 0:
    same["z"] = mine["z"].dtype == whole["z"].dtype and mine["z"].tobytes() == whole["z"].tobytes()
    same["keep"] = all(np.array_equal(a, b) for a, b in zip(mine["keep"], whole["keep"])) and len(mine["keep"]) == n
    same["it"] = mine["it"] == whole["it"]
else:
    same["z"] = mine["z"] is None
with open(out_path, "wb") as fh:
    pickle.dump(dict(same=same, log=log, iters=whole["iters"].tolist(), fit_stats=mine["fit_stats"], masked_iters=whole["masked_iters"],
                     keep_hollow=whole["keep"][hollow], wire=stats().tolist()), fh)
print("WIRE rank %d: all-reduces, broadcasts, payload bytes, host round trips = %s" % (rank, stats().tolist()), flush=True)
comm.barrier(); comm.close()
'''


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    """The three ranks, run once: what each of them left."""
    from wgsassign_amd.comm import free_port_pair
    tmp = tmp_path_factory.mktemp("relay")
    script = tmp / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, port=free_port_pair(), world=WORLD, m=M, n=N, K=K, P=P, hollow=HOLLOW))
    env = dict(os.environ, WGSASSIGN_DEVICE="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(tmp / ("rank%d.pkl" % r))], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True, env=env) for r in range(WORLD)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, o[-3000:])
        print([ln for ln in o.splitlines() if ln.startswith("WIRE")][0])
    return [pickle.load(open(tmp / ("rank%d.pkl" % r), "rb")) for r in range(WORLD)]


@pytest.mark.parametrize("what", ["af", "iters", "sums", "parts", "cnt", "first", "csums", "masked_iters", "z", "keep", "it"])
def test_three_shards_give_the_bits_of_one_process(ranks, what):
    """Fitted frequencies and iteration counts, the n x K sums, the partition sums, the class counts, first sites and sums, the
    iterations of the masked fits and the z-scores (with the kept sites behind them): on every rank what one process computes."""
    for r, got in enumerate(ranks):
        if what in got["same"]:
            assert got["same"][what], "rank %d: %s differs from the one-process run" % (r, what)
    assert what in ranks[0]["same"]


def test_the_case_is_the_one_described(ranks):
    got = ranks[0]
    assert all(it > 0 for it in got["iters"]) and len(got["masked_iters"]) == N       # every fit converged: by a chain, given the guard
    keep = got["keep_hollow"]
    assert (keep < 8192).any() and (keep >= 16384).any() and not ((keep >= 8192) & (keep < 16384)).any()


def test_every_relay_is_world_broadcasts_of_its_payload(ranks):
    """Per relayed call [all-reduces, broadcasts, payload bytes] added to the communicator, on every rank.  A relay is one broadcast
    per rank of its payload; what else a call issues is named with it."""
    iters, masked = ranks[0]["iters"], ranks[0]["masked_iters"]
    nk = N * 253                                            # the class sweep's closing all-reduce: counts | per rank (first sites | over)
    for r, got in enumerate(ranks):
        sweeps, chain_relays = got["fit_stats"]
        want = [
            # one all-reduce of 2 K sums per sweep enqueued and the empty one that closes the fit; one relay per batch of chains, and
            # every fit's every iteration is one float32 carry in one of them
            ("wgs_em_fit", [sweeps + 1, WORLD * chain_relays, sweeps * 2 * K * 8 + WORLD * 4 * sum(iters)]),
            ("wgs_score_totals_all", [0, WORLD, WORLD * N * K * 8]),                      # --get_pop_like: the float64 totals
            ("wgs_score_totals_all", [0, WORLD, WORLD * N * K * 8]),                      # the partition sums: totals first ...
            ("wgs_score_chains_walk_all", [0, WORLD, WORLD * N * P * K * 4]),             # ... then the float32 chains
            ("wgs_zscore_classes_sharded", [1, WORLD, WORLD * N * 256 * 3 * 4 + (nk + WORLD * (nk + N)) * 8]),
            ("wgs_zscore_classes_sharded", [1, WORLD, WORLD * N * 256 * 3 * 4 + (nk + WORLD * (nk + N)) * 8]),   # inside the z-scores
            # one relay per iteration until the last fit has converged, a carry per fit still running
            ("wgs_em_fit_masked_sharded", [0, WORLD * max(masked), WORLD * 4 * sum(masked)]),
        ]
        print("rank %d: %s" % (r, got["log"]))
        assert [(name, d[:3]) for name, d in got["log"]] == want, "rank %d" % r
        assert got["wire"] == ranks[0]["wire"]
