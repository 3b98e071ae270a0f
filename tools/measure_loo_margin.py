#!/usr/bin/env python3
"""How far a leave-one-out re-fit's stopping iteration lies from that of its population's full fit, on the resident --loo: the
   distribution of t*_i - t*_pop(i) from which glassy.LOO_MARGIN (the first horizon of a windowed re-fit) is
   chosen.   python tools/measure_loo_margin.py [out.json] [snps inds pops ...]   (default: the two BASELINE shapes)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wgsassign_amd import device, glassy  # noqa: E402


def measure(m, n, K, depth, seed=20260313, maf_iter=200, tole=1e-4):
    ctx = device.get_context()
    group_of = np.minimum(np.arange(n) // (n // K), K - 1).astype(np.int32)
    counts = np.bincount(group_of, minlength=K)
    b = device.DeviceBeagle(m, n, group_of, K)
    b.synth(seed, depth)
    ctx.sync()
    em = device.EMBatch(b, np.arange(K, dtype=np.int32))
    pop_iters = em.run(maf_iter, tole)
    af = np.stack([(em.clamp(k, int(counts[k])), em.get_f(k))[1] for k in range(K)], axis=1)
    em.close()
    tm = {}
    glassy.loo_device(b, b, af, group_of, maf_iter, tole, 1, verbose=False, timings=tm, need_parts=False)
    b.close()
    it = np.asarray(tm["iters"]).astype(int)
    pop = np.where(pop_iters > 0, pop_iters, maf_iter).astype(int)[group_of]
    diff = np.where(it > 0, it, maf_iter) - pop
    values, freq = np.unique(diff, return_counts=True)
    return {"snps": m, "individuals": n, "populations": K, "depth": depth, "population_stops": [int(x) for x in pop_iters],
            "refit_stops_min_max": [int(it.min()), int(it.max())], "difference_counts": {str(int(v)): int(c) for v, c in zip(values, freq)},
            "largest_difference": int(diff.max())}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    shapes = [tuple(int(x) for x in sys.argv[i:i + 3]) for i in range(2, len(sys.argv) - 2, 3)] or [(2_000_000, 500, 8), (5_000_000, 180, 5)]
    rows = [measure(m, n, K, depth) for m, n, K in shapes for depth in (0.5, 2.0, 8.0)]
    res = {"shapes": rows, "largest_difference": max(r["largest_difference"] for r in rows), "margin_in_use": glassy.LOO_MARGIN}
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
