#!/usr/bin/env python3
"""Generate tests/golden/zstat_cases.npz from the REAL reference on the enumerated terms of tests/zstat_cases.py.

Run as make_golden_fisher_cases.py is run: build the reference in a scratch copy (python3 setup.py build_ext --inplace) and run this
file with that copy on PYTHONPATH, from a working directory other than this repository's root (whose own WGSassign package would
take the reference's place).

The grid: per individual zscore_cy.expected_W_l and zscore_cy.variance_W_l, called directly into zeroed arrays exactly as
zscore.py:81-120 calls them, with the builders' L, L_keep (zstat_cases.recorded_slots of the term sites), A[L_keep], AD, AD_factorial,
AD_like and AD_index.  The reference has no tiers: deep and dense depths are recorded alike.
The pipeline case: zstat_cases.boundary_frequencies through the assignment flavour, function by function (make_golden_zscore.one)
and through the CLI.  Its likelihoods and depths are those of zscore_classes.npz, so the dictionary, L_keep and the tables are
asserted to be the ones recorded there and only what the frequencies change is written.

Everything written is data: the generators' arguments, the digests of the inputs and what the reference returned.
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
import zstat_cases as zs  # noqa: E402
from make_golden_zscore import cli, one  # noqa: E402  (supplies np.math and imports the reference)
from WGSassign import zscore, zscore_cy  # noqa: E402

assert os.path.dirname(os.path.abspath(zscore.__file__)) != os.path.join(os.path.dirname(os.path.dirname(HERE)), "WGSassign"), \
    "this is the repository's own WGSassign package, not the reference"

SAME_AS_CLASSES = ("keys", "counts", "means", "AD_array", "keep", "fac", "like", "index")
RECORDED = ("wobs", "wl", "var", "sums")


def main():
    arrays = {}
    g = zs.shared_grid()
    slots = zs.recorded_slots(g, **zs.GOLDEN_GEN)
    L, AD, index = g["L"].copy(), g["AD"].copy(), g["index"].astype(np.int32)      # (copies: the shared grid is read-only)
    unused = np.zeros((1, 4), dtype=np.int32)                  # AD_array: an argument neither function reads
    out = [[], [], []]
    for i in range(len(g["variant"])):
        keep = np.ascontiguousarray(g["sites"][slots[i]], dtype=np.int32)
        A = np.ascontiguousarray(g["A"][keep, i])
        fac, like = g["fac"][i].copy(), g["like"][i].copy()
        wobs, wl, var = (np.zeros(len(keep), dtype=np.float32) for _ in range(3))
        zscore_cy.expected_W_l(L, keep, A, AD, unused, fac, like, index, 1, i, wobs, wl)
        zscore_cy.variance_W_l(L, keep, A, AD, unused, fac, like, index, 1, i, var, wl)
        for o, a in zip(out, (wobs, wl, var)):
            o.append(a)
    arrays["grid_gen"] = np.array(repr(zs.GOLDEN_GEN))
    arrays["grid_digest"] = np.array(zs.digest(g))
    arrays["grid_count"] = np.array([len(s) for s in slots], dtype=np.int32)
    for name, o in zip(("wobs", "wl", "var"), out):
        arrays["grid_" + name] = np.concatenate(o)
    print("grid:", len(slots), "individuals,", int(arrays["grid_count"].sum()), "terms, not finite:",
          [int((~np.isfinite(arrays["grid_" + k])).sum()) for k in ("wobs", "wl", "var")])

    L, AD, IDs, A = zs.boundary_frequencies(**zs.PIPELINE_GEN)
    pops = np.unique(IDs[:, 1])
    classes = np.load(os.path.join(HERE, "zscore_classes.npz"), allow_pickle=False)
    arrays["pipeline_gen"] = np.array(repr(zs.PIPELINE_GEN))
    arrays["pipeline_digest"] = np.array(synth_depth.digest(L, AD, A))
    with tempfile.TemporaryDirectory() as td:
        paths = synth_depth.write_inputs(os.path.join(td, "boundary"), L, AD, IDs, A)
        for i in range(L.shape[1] // 2):
            with np.errstate(all="ignore"):
                got = one(L, AD, IDs, pops, A, i, "assignment", 0, False)
            for k in SAME_AS_CLASSES:
                assert got[k].tobytes() == classes["run0_i%d_%s" % (i, k)].tobytes(), (i, k)
            for k in RECORDED:
                arrays["pipeline_i%d_%s" % (i, k)] = got[k]
        rc, text_out, err, text = cli(td, "run", paths, "assignment", 0, False, None, None)
        assert rc == 0, err
        lines = [ln for ln in text_out.splitlines() if re.match(r"(Finished individual|z_mu|z_var|z_obs|Loci used|Z-score|Saved \d+)", ln)]
        arrays["pipeline_stdout"] = np.array("\n".join(lines).replace(td + os.sep, ""))
        arrays["pipeline_file"] = np.array(text)
        print("pipeline ->", text.split(), "sites with W_l_obs = -inf:",
              [int(np.isneginf(arrays["pipeline_i%d_wobs" % i]).sum()) for i in range(L.shape[1] // 2)])
    path = os.path.join(HERE, "zstat_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
