#!/usr/bin/env python3
"""Generate tests/golden/zscore_deep.npz from the REAL reference on inputs with sites deeper than 21 reads.

Run as make_golden_zscore.py is run: build the reference in a scratch copy (python3 setup.py build_ext --inplace) and run this
file with that copy on PYTHONPATH.  One small case (tests/synth_deep.py: 1500 sites, 6 individuals in populations of 3 / 2 / 1):
an individual without deep sites, two whose deep depths are incomplete and therefore dropped, one with every class of the depths
22 and 23 (both kept: AD_index grows to (24, 24) and the loops of zscore_cy run to 23), one with single sites at (255, 255),
(200, 0) and (0, 37).  Both flavours; the reference flavour stops before the population of one.

Everything written is data: the generator's arguments and the digest of the inputs, what the reference's functions returned per
individual (the arrays zscore.npz holds), and the stdout lines and output files of the two CLI runs.
"""
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import synth_deep  # noqa: E402
import synth_depth  # noqa: E402
from make_golden_zscore import cli, one  # noqa: E402  (supplies np.math and imports the reference)

GEN = dict(m=1500, n=6, K=3, seed=21, roles=("none", "dropped", "kept", "single", "dropped", "none"), sizes=(3, 2, 1), per_class=3)
RUNS = [("assignment", None, None), ("reference", None, 5)]


def main():
    arrays = {}
    L, AD, IDs, A, deep = synth_deep.make_deep(**GEN)
    pops = np.unique(IDs[:, 1])
    arrays["case_deep_gen"] = np.array(repr(GEN))
    arrays["case_deep_digest"] = np.array(synth_depth.digest(L, AD, A))
    with tempfile.TemporaryDirectory() as td:
        paths = synth_depth.write_inputs(os.path.join(td, "deep"), L, AD, IDs, A)
        for r, (flavour, lo, hi) in enumerate(RUNS):
            arrays["run%d" % r] = np.array(repr(dict(case="deep", flavour=flavour, thr=0, srt=False, ind_start=lo, ind_end=hi)))
            for i in range(lo or 0, L.shape[1] // 2 if hi is None else hi):
                for k, v in one(L, AD, IDs, pops, A, i, flavour, 0, False).items():
                    arrays["run%d_i%d_%s" % (r, i, k)] = v
            rc, out, err, text = cli(td, "run%d" % r, paths, flavour, 0, False, lo, hi)
            assert rc == 0, err
            lines = [ln for ln in out.splitlines() if re.match(r"(Finished individual|z_mu|z_var|z_obs|Loci used|Z-score|Saved \d+)", ln)]
            arrays["run%d_stdout" % r] = np.array("\n".join(lines).replace(td + os.sep, ""))
            arrays["run%d_file" % r] = np.array(text)
            print("run", r, flavour, "->", text.split(), "index", [arrays["run%d_i%d_index" % (r, i)].shape for i in range(5)])
    path = os.path.join(HERE, "zscore_deep.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
