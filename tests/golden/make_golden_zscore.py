#!/usr/bin/env python3
"""Generate tests/golden/zscore.npz from the REAL reference (zscore.py, zscore_cy.pyx, the two z-score blocks of WGSassign.py).

Run where the reference is available only, in the manner of make_golden.py: build the reference in a scratch copy
(python3 setup.py build_ext --inplace) and run this file with that copy on PYTHONPATH.  NumPy 2 has no np.math, which
zscore.get_factorials uses; it is supplied here before the reference is imported.

Everything written is data: the seeds and digests of the inputs (regenerated through tests/synth_depth.py) and what the
reference returned -- zscore.AD_summary (keys, counts, means, AD_array), get_L_keep, get_factorials, get_expected_W_l,
get_var_W_l, the sums and z, the iteration at which each subset fit converged, and the stdout lines and output files of the CLI.
"""
import contextlib
import io
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

np.math = math

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import synth_depth  # noqa: E402

from WGSassign import emMAF, zscore  # noqa: E402

# name -> generator arguments, options.  (a) likelihoods a pure function of the key, (b) perturbed: the 0.01 filter drops sites,
# (c) a threshold that removes keys and whole depths, (d) three populations of 4, 2 and 3 individuals
CASES = {
    "a": dict(gen=dict(m=1200, n=9, K=3, seed=101, depth=1.5, jitter=0.0, sizes=(4, 2, 3)), thr=0),
    "b": dict(gen=dict(m=1200, n=9, K=3, seed=202, depth=1.5, jitter=0.02, sizes=(4, 2, 3)), thr=0),
    "c": dict(gen=dict(m=1200, n=9, K=3, seed=303, depth=1.5, jitter=0.0, sizes=(4, 2, 3)), thr=25),
}
RUNS = [  # (case, flavour, single_read_threshold, ind_start, ind_end)
    ("a", "assignment", True, None, None), ("a", "assignment", False, None, None), ("a", "reference", False, None, None),
    ("a", "reference", True, 3, 7), ("b", "assignment", False, None, None), ("b", "reference", False, 2, 6),
    ("c", "assignment", False, None, None), ("c", "reference", False, 4, 9),
]
MAF_ITER, MAF_TOLE = 200, 1e-4


def one(L, AD, IDs, pops, A, i, flavour, thr, srt):
    d, arr = zscore.AD_summary(L, AD, i, thr, srt)
    keys = np.array(list(d.keys()), dtype=np.int64).reshape(-1, 2)
    counts = np.array([v[0] for v in d.values()], dtype=np.int64)
    means = np.array([v[1] for v in d.values()], dtype=np.float32)
    keep, nk = zscore.get_L_keep(L, AD, d, arr, i)
    fac, like, idx = zscore.get_factorials(arr, d, 0.01)
    it = -1
    if flavour == "assignment":
        k = np.argwhere(pops == IDs[i, 1])[0][0]
        af = np.ascontiguousarray(A[keep, :][:, k].reshape(-1))
    else:
        others = np.argwhere(IDs[:, 1] == IDs[i, 1])
        others = others[others != i]
        cols = np.sort(np.concatenate((others * 2, others * 2 + 1)), axis=0).reshape(-1)
        L_pop = np.ascontiguousarray(L[keep, :][:, cols])
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            af = emMAF.emMAF(L_pop, MAF_ITER, MAF_TOLE, 1)
        found = re.findall(r"converged at iteration: (\d+)", buf.getvalue())
        it = int(found[0]) if found else 0
        lo = 1 / (2 * (L_pop.shape[1] // 2 + 1))
        af[af < lo] = lo
        af[af > 1 - lo] = 1 - lo
    wobs, wl = zscore.get_expected_W_l(L, keep, af, AD, arr, fac, like, idx, 1, i)
    wobs_arr = np.zeros(keep.shape[0], dtype=np.float32)
    from WGSassign import zscore_cy
    zscore_cy.expected_W_l(L, keep, af, AD, arr, fac, like, idx, 1, i, wobs_arr, np.zeros(keep.shape[0], dtype=np.float32))
    var = zscore.get_var_W_l(L, keep, af, AD, arr, fac, like, idx, wl, 1, i)
    z_mu, z_var = np.sum(wl), np.sum(var)
    z = (wobs - z_mu) / np.sqrt(z_var)
    return dict(keys=keys, counts=counts, means=means, AD_array=arr, keep=keep, fac=fac, like=like, index=idx, A=af, wobs=wobs_arr,
                wl=wl, var=var, sums=np.array([wobs, z_mu, z_var, z], dtype=np.float32), it=np.int32(it))


def cli(td, tag, paths, flavour, thr, srt, lo, hi):
    out = os.path.join(td, tag)
    cmd = [sys.executable, "-c", "import numpy, math; numpy.math = math; from WGSassign import WGSassign; WGSassign.main()",
           "--beagle", paths["beagle"], "--pop_af_IDs", paths["ids"], "--pop_names", paths["names"], "--ind_ad_file", paths["ad"],
           "--out", out, "--get_%s_z_score" % flavour]
    if flavour == "assignment":
        cmd += ["--pop_af_file", paths["af"]]
    if thr:
        cmd += ["--allele_count_threshold", str(thr)]
    if srt:
        cmd += ["--single_read_threshold"]
    if lo is not None:
        cmd += ["--ind_start", str(lo)]
    if hi is not None:
        cmd += ["--ind_end", str(hi)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONWARNINGS="ignore"))
    name = out + (".z_ind.txt" if flavour == "assignment" else ".reference_z_ind.txt")
    text = open(name).read() if os.path.exists(name) else ""
    return r.returncode, r.stdout, r.stderr, text


def main():
    arrays = {}
    with tempfile.TemporaryDirectory() as td:
        data = {}
        for name, c in CASES.items():
            L, AD, IDs, A = synth_depth.make_depth(**c["gen"])
            data[name] = (L, AD, IDs, A, synth_depth.write_inputs(os.path.join(td, name), L, AD, IDs, A))
            arrays["case_%s_gen" % name] = np.array(repr(c["gen"]))
            arrays["case_%s_digest" % name] = np.array(synth_depth.digest(L, AD, A))
        for r, (name, flavour, srt, lo, hi) in enumerate(RUNS):
            L, AD, IDs, A, paths = data[name]
            thr = CASES[name]["thr"]
            pops = np.unique(IDs[:, 1])
            first, last = (0 if lo is None else lo), (L.shape[1] // 2 if hi is None else hi)
            arrays["run%d" % r] = np.array(repr(dict(case=name, flavour=flavour, thr=thr, srt=srt, ind_start=lo, ind_end=hi)))
            for i in range(first, last):
                for k, v in one(L, AD, IDs, pops, A, i, flavour, thr, srt).items():
                    arrays["run%d_i%d_%s" % (r, i, k)] = v
            rc, out, err, text = cli(td, "run%d" % r, paths, flavour, thr, srt, lo, hi)
            assert rc == 0, err
            lines = [ln for ln in out.splitlines() if re.match(r"(Finished individual|z_mu|z_var|z_obs|Loci used|Z-score|Saved \d+)", ln)]
            arrays["run%d_stdout" % r] = np.array("\n".join(lines).replace(td + os.sep, ""))
            arrays["run%d_file" % r] = np.array(text)
            print("run", r, name, flavour, srt, lo, hi, "->", text.split()[:4], "loci", [int(arrays["run%d_i%d_keep" % (r, i)].shape[0])
                                                                                    for i in range(first, last)][:4])
        # (e) the assertions: a threshold nothing survives; a matrix with a single class of depth 1
        L, AD, IDs, A, paths = data["a"]
        for tag, kw in (("none", dict(thr=100000, srt=False, lo=None, hi=None)), ("start0", dict(thr=0, srt=False, lo=0, hi=None))):
            rc, out, err, _ = cli(td, "fail_" + tag, paths, "assignment", **kw)
            assert rc != 0
            arrays["fail_%s_message" % tag] = np.array(err.strip().splitlines()[-1])
        AD1 = AD.copy()
        AD1[:, 0::2] = 1
        AD1[:, 1::2] = 0
        p1 = synth_depth.write_inputs(os.path.join(td, "one"), L, AD1, IDs, A)
        rc, out, err, _ = cli(td, "fail_one", p1, "assignment", thr=0, srt=True, lo=None, hi=None)
        assert rc != 0
        arrays["fail_one_message"] = np.array(err.strip().splitlines()[-1])
    path = os.path.join(HERE, "zscore.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
