"""One rank of a z-score run over SNP shards, for tests/test_gpu_zscore_sharded.py: the ranks share the one GPU and talk over
SocketComm, as the ranks of tests/test_gpu_multirank.py do.  Also the one place where the inputs of those tests are defined, so that
the ranks and the test that judges them build the same arrays.  Test infrastructure.

    python zscore_shard_worker.py CASE RANK WORLD PORT OUT [BATCH]

Rank 0 leaves what the drivers returned -- per run (z, details, printed lines) -- in OUT (a pickle of NumPy arrays).  A rank that
finds the ranks out of step ends with status 76, as the command line does."""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth_deep      # noqa: E402
import synth_depth     # noqa: E402
import zscore_cases    # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BLOCKS_M, BLOCKS_CUT = 20011, 10007          # neither a multiple of 64 nor of 4096
DEEP_ROLES, DEEP_SIZES = ("none", "dropped", "kept", "single", "dropped", "none"), (3, 2, 1)
EMPTY_IND = 3


def run(flavour, thr=0, srt=False, lo=None, hi=None, batch=64):
    return dict(flavour=flavour, thr=thr, srt=srt, lo=lo, hi=hi, batch=batch)


def even_cuts(m, world):
    from wgsassign_amd.comm import shard_range
    return [shard_range(m, r, world)[0] for r in range(1, world)]


def recorded_cases(batch):
    """Every run of tests/golden/zscore.npz: [(inputs, run)] in the order of the records."""
    from test_zscore_cpu import case_inputs, runs
    gold = np.load(os.path.join(GOLDEN, "zscore.npz"), allow_pickle=False)
    return [(case_inputs(gold, spec["case"]), run(spec["flavour"], spec["thr"], spec["srt"], spec["ind_start"], spec["ind_end"], batch))
            for _, spec in runs(gold)]


def odd_inputs():
    return synth_depth.make_depth(5003, 13, 3, seed=77, depth=2.5, jitter=0.01, sizes=(5, 2, 6))


def empty_inputs(cut):
    """The odd shapes with individual EMPTY_IND at depth 0 from `cut` on: it keeps nothing there (depth 0 never survives the key filter)."""
    L, AD, IDs, A = odd_inputs()
    AD = AD.copy()
    AD[cut:, 2 * EMPTY_IND:2 * EMPTY_IND + 2] = 0
    return L, AD, IDs, A


def blocks_inputs():
    return synth_depth.make_depth(BLOCKS_M, 6, 2, seed=5, depth=1.5, sizes=(2, 4))


def deep_inputs():
    """synth_deep's main case of 20011 sites, and for every deep individual the cells of its deep sites 4095 and 4096 once more at the
    two sites next to the cut: BLOCKS_CUT - 1 and BLOCKS_CUT."""
    L, AD, IDs, A, deep = synth_deep.make_deep(BLOCKS_M, 6, 3, 11, DEEP_ROLES, sizes=DEEP_SIZES)
    L, AD = L.copy(), AD.copy()
    for i in (1, 2, 4):
        for src, dst in ((4095, BLOCKS_CUT - 1), (4096, BLOCKS_CUT)):
            L[dst, 2 * i:2 * i + 2] = L[src, 2 * i:2 * i + 2]
            AD[dst, 2 * i:2 * i + 2] = AD[src, 2 * i:2 * i + 2]
    return L, AD, IDs, A


def jobs(case, world, batch):
    """[(inputs, cuts, run)] of a case."""
    if case == "recorded":
        return [(inp, even_cuts(inp[0].shape[0], world), r) for inp, r in recorded_cases(batch)]
    if case == "odd":
        inp = odd_inputs()
        cuts = even_cuts(5003, world)
        return [(inp, cuts, run("assignment", thr=3, lo=2, hi=11, batch=4)), (inp, cuts, run("reference", thr=3, lo=2, hi=11, batch=4)),
                (inp, cuts, run("assignment", srt=True))]
    if case == "empty":
        cuts = even_cuts(5003, world)
        return [(empty_inputs(cuts[0]), cuts, run("reference", lo=2, hi=6, batch=4))]
    if case == "blocks":
        return [(blocks_inputs(), [BLOCKS_CUT], run("reference", lo=1, hi=4))]
    if case == "deep":
        inp = deep_inputs()
        return [(inp, [BLOCKS_CUT], run("assignment", lo=1, hi=4, batch=2)), (inp, [BLOCKS_CUT], run("reference", lo=1, hi=4, batch=2))]
    if case == "classes":                                  # every depth class up to 21 reads, the cut inside a tile
        inp = zscore_cases.every_class()[:4]
        cuts = [zscore_cases.CLASSES_CUT]
        return [(inp, cuts, run("assignment", batch=3)), (inp, cuts, run("reference", batch=2))]
    if case == "outofstep":
        inp, r = recorded_cases(64)[0]
        return [(inp, even_cuts(inp[0].shape[0], world), dict(r, flavour="assignment", batch=None))]
    raise ValueError(case)


def device_run(comm, inputs, cuts, spec):
    """This rank's shard of `inputs` through the drivers; what they returned."""
    from wgsassign_amd import zscore
    from wgsassign_amd.device import AFSet, DeviceBeagle
    L, AD, IDs, A = inputs
    bounds = [0] + list(cuts) + [L.shape[0]]
    lo, hi = bounds[comm.rank], bounds[comm.rank + 1]
    pops = np.unique(IDs[:, 1])
    group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
    i_lo, i_hi = zscore.ind_range(L.shape[1] // 2, spec["lo"], spec["hi"])
    Ls = np.ascontiguousarray(L[lo:hi])
    if spec["flavour"] == "reference":
        b = DeviceBeagle.from_host(Ls, group_of, len(pops), site0=lo)
    else:
        b = DeviceBeagle.from_host(Ls, site0=lo)
    depth = zscore.DepthTable(b, np.ascontiguousarray(AD[lo:hi]), chunk_rows=1000)
    details, lines = [], []
    if spec["flavour"] == "reference":
        z = zscore.reference_z_scores(b, depth, IDs, group_of, 200, 1e-4, spec["thr"], spec["srt"], i_lo, i_hi, batch=spec["batch"],
                                      say=lines.append, details=details, comm=comm)
    else:
        afs = AFSet.from_host(np.ascontiguousarray(A[lo:hi]))
        z = zscore.assignment_z_scores(b, depth, IDs, pops, afs, spec["thr"], spec["srt"], i_lo, i_hi, batch=spec["batch"],
                                       say=lines.append, details=details, comm=comm)
        afs.close()
    depth.close()
    b.close()
    return z, details, [ln for ln in lines if not ln.startswith("EM (MAF)")]


def main(argv):
    case, rank, world, port, out = argv[0], int(argv[1]), int(argv[2]), int(argv[3]), argv[4]
    batch = int(argv[5]) if len(argv) > 5 else 64
    from wgsassign_amd.comm import COMM_DIVERGED, CollectiveMismatch, SocketComm
    from wgsassign_amd.device import get_context
    comm = SocketComm(rank, world, port=port, timeout=60.0).attach(get_context())
    results = []
    try:
        for inputs, cuts, spec in jobs(case, world, batch):
            if case == "outofstep":
                spec = dict(spec, batch=3 + rank)              # the ranks disagree about the batches
            results.append(device_run(comm, inputs, cuts, spec))
    except CollectiveMismatch as e:
        print("rank %d: %s" % (rank, e), file=sys.stderr, flush=True)
        os._exit(COMM_DIVERGED)
    if rank == 0:
        with open(out, "wb") as fh:
            pickle.dump(results, fh)
    else:
        assert all(z is None and not d for z, d, _ in results), "only rank 0 returns z-scores and details"
    comm.barrier()
    comm.close()


if __name__ == "__main__":
    main(sys.argv[1:])
