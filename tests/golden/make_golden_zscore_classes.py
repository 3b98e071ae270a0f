#!/usr/bin/env python3
"""Generate tests/golden/zscore_classes.npz from the REAL reference on inputs that hold every depth class up to 21 reads.

Run as make_golden_zscore.py is run: build the reference in a scratch copy (python3 setup.py build_ext --inplace) and run this
file with that copy on PYTHONPATH, from a working directory other than this repository's root (whose own WGSassign package
would take the reference's place in the CLI runs).  One small case (tests/zscore_cases.py: every_class at 1600 sites, three sites per class): four
individuals in two populations, one of each population with all 253 pairs of the depths 0 .. 21 -- every depth 1 .. 21 is kept,
AD_index grows to (22, 22) and the loops of zscore_cy run to 21.  Both flavours.

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
import synth_depth  # noqa: E402
import zscore_cases  # noqa: E402
from make_golden_zscore import cli, one  # noqa: E402  (supplies np.math and imports the reference)

GEN = dict(m=1600, per_class=3, seed=3)
RUNS = [("assignment", None, None), ("reference", None, None)]


def main():
    arrays = {}
    L, AD, IDs, A, _ = zscore_cases.every_class(**GEN)
    pops = np.unique(IDs[:, 1])
    arrays["case_classes_gen"] = np.array(repr(GEN))
    arrays["case_classes_digest"] = np.array(synth_depth.digest(L, AD, A))
    with tempfile.TemporaryDirectory() as td:
        paths = synth_depth.write_inputs(os.path.join(td, "classes"), L, AD, IDs, A)
        for r, (flavour, lo, hi) in enumerate(RUNS):
            arrays["run%d" % r] = np.array(repr(dict(case="classes", flavour=flavour, thr=0, srt=False, ind_start=lo, ind_end=hi)))
            for i in range(lo or 0, L.shape[1] // 2 if hi is None else hi):
                for k, v in one(L, AD, IDs, pops, A, i, flavour, 0, False).items():
                    arrays["run%d_i%d_%s" % (r, i, k)] = v
            rc, out, err, text = cli(td, "run%d" % r, paths, flavour, 0, False, lo, hi)
            assert rc == 0, err
            lines = [ln for ln in out.splitlines() if re.match(r"(Finished individual|z_mu|z_var|z_obs|Loci used|Z-score|Saved \d+)", ln)]
            arrays["run%d_stdout" % r] = np.array("\n".join(lines).replace(td + os.sep, ""))
            arrays["run%d_file" % r] = np.array(text)
            print("run", r, flavour, "->", text.split(), "index", [arrays["run%d_i%d_index" % (r, i)].shape for i in range(4)])
    path = os.path.join(HERE, "zscore_classes.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
