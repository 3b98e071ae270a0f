#!/usr/bin/env python3
"""Times the two z-score options on device-resident data and prints ONE JSON line.

    python tools/bench_zscore.py [--shapes 1000000x200x5,2000000x500x8] [--inds 200] [--step-timeout 600] [--deep-share 0.001] [--ranks 2]

Per shape m x n x K: the matrix is generated on the device (wgs_beagle_synth, depth 1.5), the depth table on the host (Poisson 1.5
split binomially; no file I/O anywhere in the timed part), then --get_assignment_z_score and --get_reference_z_score of the
first --inds individuals with --single_read_threshold off.  Reported per flavour: wall seconds, and inside them the depth-class sweep,
the mask sweep, the masked fits and the statistic sweep; for comparison the bytes each sweep has to read once (slabs + depth
table).  Every shape runs in a child process of its own under a time limit, and a shape that fails ends the run: nothing further
is started on the card.

--deep-share S (off by default; the output without it is unchanged) adds one leg, "deep": the first shape once more with the share S
of the table's cells overwritten by deep sites -- depth uniform in 22..30, alternative count uniform in 0..depth, so that with a few
hundred deep sites per individual some depths have all their classes and are kept (deep table on the device) and the others are
dropped; the likelihoods stay independent of the depth, as in the other legs.  Its "deep_list_s" is the part of the class phase
spent listing the deep sites and building their dictionary.

--ranks N (off by default) adds one leg, "ranks": the first shape once more with its SNPs cut into N shards, one per rank, ALL ON THIS
ONE CARD over the socket transport, as the multi-rank tests run.  The ranks share the GPU, so the leg shows what the hops between the
shards cost beside the one-process figure of the same run -- not a speed-up.  Its phases are rank 0's and include what it waited for
the other ranks (the class sweep goes from shard to shard)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_shape(m, n, K, inds, deep_share=0.0, rank=0, world=1, port=0):
    import numpy as np
    from wgsassign_amd import zscore
    from wgsassign_amd.comm import SocketComm, shard_range
    from wgsassign_amd.device import AFSet, DeviceBeagle, get_context
    ctx = get_context()
    comm = SocketComm(rank, world, port=port).attach(ctx) if world > 1 else None
    lo, hi = shard_range(m, rank, world)
    rng = np.random.default_rng(1)
    group_of = (np.arange(n) * K // n).astype(np.int32)
    IDs = np.array([("Ind%d" % i, "pop%02d" % g) for i, g in enumerate(group_of)], dtype=str)
    pops = np.unique(IDs[:, 1])
    b = DeviceBeagle(hi - lo, n, group_of, K, site0=lo)        # (the generator is keyed by the global site: the shards of one matrix)
    b.synth(7, 1.5)
    depth = zscore.DepthTable(b)
    step = max(1, (64 << 20) // (8 * n))
    deep_rng, n_deep = np.random.default_rng(2), 0
    for r in range(0, m, step):
        rows = min(step, m - r)
        D = rng.poisson(1.5, size=(rows, n))
        Aa = rng.binomial(D, 0.5)
        AD = np.empty((rows, 2 * n), dtype=np.int32)
        AD[:, 0::2], AD[:, 1::2] = D - Aa, Aa
        if deep_share > 0:
            at = np.nonzero(deep_rng.random((rows, n)) < deep_share)
            dd = deep_rng.integers(22, 31, size=len(at[0]))
            da = deep_rng.integers(0, dd + 1)
            AD[at[0], 2 * at[1]], AD[at[0], 2 * at[1] + 1] = dd - da, da
            n_deep += len(dd)
        a, z = max(r, lo), min(r + rows, hi)                   # every rank draws the whole table and keeps its rows
        if a < z:
            depth.upload_rows(AD[a - r:z - r], a - lo)
    afs = AFSet.from_host(np.ascontiguousarray(rng.uniform(0.05, 0.95, size=(m, K)).astype(np.float32)[lo:hi]))
    inds = min(inds, n)
    out = dict(shape=[m, n, K], individuals=inds, device=ctx.info(), slab_bytes=b.nbytes(), depth_bytes=2 * m * n)
    if deep_share > 0:
        out.update(deep_share=deep_share, deep_sites_per_individual=round(n_deep / n, 1))
    quiet = lambda *_: None
    for name in ("assignment", "reference"):
        phases = {}
        lib_classes, lib_keep, lib_stats, lib_deep = zscore.AD_summary, zscore.get_L_keep, zscore.KeepSet.stats, zscore.deep_classes

        def timed(key, fn):
            def run(*a, **kw):
                t = time.perf_counter()
                r = fn(*a, **kw)
                ctx.sync()
                phases[key] = phases.get(key, 0.0) + time.perf_counter() - t
                return r
            return run
        zscore.AD_summary, zscore.get_L_keep = timed("class_sweep_s", lib_classes), timed("mask_sweep_s", lib_keep)
        zscore.KeepSet.stats = timed("stat_sweep_and_download_s", lib_stats)
        if deep_share > 0:
            zscore.deep_classes = timed("deep_dictionary_s", lib_deep)
        if comm is not None:
            comm.barrier()
        t0 = time.perf_counter()
        if name == "assignment":
            zscore.assignment_z_scores(b, depth, IDs, pops, afs, 0, False, 0, inds, say=quiet, comm=comm)
        else:
            zscore.reference_z_scores(b, depth, IDs, group_of, 200, 1e-4, 0, False, 0, inds, say=quiet, comm=comm)
        ctx.sync()
        phases["wall_s"] = time.perf_counter() - t0
        zscore.AD_summary, zscore.get_L_keep, zscore.KeepSet.stats, zscore.deep_classes = lib_classes, lib_keep, lib_stats, lib_deep
        out[name] = {k: round(v, 4) for k, v in phases.items()}
    if comm is not None:
        out.update(ranks=world, shard=[lo, hi])
        comm.barrier()
        comm.close()
    if rank == 0:
        print(json.dumps(out))


def ranks_leg(shape, inds, world, step_timeout):
    """The first shape over `world` ranks on this card: rank 0's JSON, or None with the failure printed."""
    from wgsassign_amd.comm import free_port_pair
    port = free_port_pair()
    procs = [subprocess.Popen(["timeout", "-k", "10", str(step_timeout), sys.executable, os.path.abspath(__file__), "--child", shape, "--inds",
                               str(inds), "--child-rank", str(r), "--child-world", str(world), "--child-port", str(port)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = [p.communicate() for p in procs]
    if any(p.returncode != 0 for p in procs):
        print(json.dumps({"bench": "zscore", "failed": "%s over %d ranks" % (shape, world), "rc": [p.returncode for p in procs],
                          "stderr": "".join(o[1][-400:] for o in outs)}))
        return None
    return json.loads(outs[0][0].strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000x200x5,2000000x500x8")
    ap.add_argument("--inds", type=int, default=10**9)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--child", default=None)
    ap.add_argument("--deep-share", type=float, default=0.0, help="add a leg with this share of deep sites (e.g. 0.001) on the first shape")
    ap.add_argument("--child-deep-share", type=float, default=0.0)
    ap.add_argument("--ranks", type=int, default=1, help="add a leg with the first shape cut into this many SNP shards, all on this card")
    ap.add_argument("--child-rank", type=int, default=0)
    ap.add_argument("--child-world", type=int, default=1)
    ap.add_argument("--child-port", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        m, n, K = (int(x) for x in a.child.split("x"))
        return one_shape(m, n, K, a.inds, a.child_deep_share, a.child_rank, a.child_world, a.child_port)
    results, legs = [], [(shape, 0.0) for shape in a.shapes.split(",")]
    if a.deep_share > 0:
        legs.append((legs[0][0], a.deep_share))
    for shape, share in legs:
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", shape,
                            "--inds", str(a.inds), "--child-deep-share", str(share)], capture_output=True, text=True)
        if r.returncode != 0:
            print(json.dumps({"bench": "zscore", "failed": shape, "rc": r.returncode, "stderr": r.stderr[-400:], "results": results}))
            return 1
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = {"bench": "zscore", "results": results}
    if a.deep_share > 0:
        line = {"bench": "zscore", "results": results[:-1], "deep": results[-1]}
    if a.ranks > 1:
        line["ranks"] = ranks_leg(legs[0][0], a.inds, a.ranks, a.step_timeout)
        if line["ranks"] is None:
            return 1
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
