#!/usr/bin/env python3
"""--get_pop_like from a BGZF file, resident against windowed: one JSON line.

    python tools/bench_windowed.py [--snps 1000000 --inds 200 --pops 5] [--windows 4] [--repeats 3]
                                   [--parent-root DIR] [--out profiles/windowed_bench.json]
    python tools/bench_windowed.py --fit [...] [--out profiles/windowed_fit_bench.json]      # the same for --get_reference_af
    python tools/bench_windowed.py --loo [...] [--out profiles/windowed_loo_bench.json]      # the same for --get_reference_af --loo
    python tools/bench_windowed.py --loo-ds [...] [--out profiles/windowed_loo_ds_bench.json]  # ... with --loo_downsampled_beagle
    python tools/bench_windowed.py --ne [...] [--out profiles/windowed_ne_obs_bench.json]    # the same for --get_reference_af --ne_obs
    python tools/bench_windowed.py --z [...] [--out profiles/z_windowed.json]                # the same for --get_assignment_z_score
    python tools/bench_windowed.py --zref [...] [--out profiles/zref_windowed.json]          # the same for --get_reference_z_score

The file comes from tools/beagle_files.py (seeded, seconds to write).  Every end-to-end figure is the wall time of one
`python -m wgsassign_amd.WGSassign --get_pop_like` process -- interpreter start, HIP initialisation, ingest, scoring, the text
file -- with the index of the Beagle file cached (one run per variant warms it up and is not counted).  The variants alternate
inside every repeat, so what else the machine does meanwhile hits them alike; median and range are reported.
  resident_s          this tree, the matrix resident (WGSASSIGN_WINDOW_SITES not set);
  parent_resident_s   the same command in the tree given by --parent-root (a built checkout of the parent commit), else null;
  windowed_s          this tree, WGSASSIGN_WINDOW_SITES chosen so that --windows windows are used.
The sweep times are device events around the scoring kernels, taken in THIS process on the same file: the resident sweep
(device.assign) and the sum of the per-window sweeps (glassy.assignLL_windowed), median of the repeats after one warm-up.
The outputs of all variants are compared byte for byte.
--fit measures --get_reference_af instead (the fit in windows, in rounds over the file): the same three whole-process figures, and from
one emMAF.emMAF_windowed in this process the rounds, the seconds of every round and the EM iterations round 1 ran against the
iterations the fits needed.  What to expect there: rounds x the windowed scoring run's cost, plus round 1's extra sweeps.
--loo measures --get_reference_af --loo (the windowed fit, then the leave-one-out run in the same windows;
WGSASSIGN_LOO_WINDOW_SITES): the three whole-process figures, and from one emMAF.emMAF_windowed + glassy.loo_windowed in this process
the rounds, the seconds of every round, the first horizons' iterations against the iterations the re-fits needed, and the resident
re-fit and scoring seconds of glassy.loo_device on the same file.  What to expect there: rounds x the windowed pass, plus the resident
re-fit time x (iterations run / iterations needed), plus the per-window launches.
--loo-ds measures --get_reference_af --loo --loo_downsampled_beagle (both files in windows of kept sites;
WGSASSIGN_LOO_DS_WINDOW_SITES): the downsampled file holds the first four fifths of the reference file's sites under another seed, so
the reference file's mask drops its last fifth; --windows counts windows of KEPT sites.  The whole-process figures resident against
windowed, and from glassy.loo_windowed in this process the rounds, their seconds and how often the downsampled file was read.
--ne measures --get_reference_af --ne_obs (the windowed fit, then one pass for the Fisher information; WGSASSIGN_NE_WINDOW_SITES): the
three whole-process figures, and from fisher.fisher_obs_windowed in this process the fused sweep's time per window between events
(fisher_window_kernel).  What the resident path spends in its three kernels over the same sites (fisher_pop_kernel,
fisher_ind_sites_kernel, pairwise_leaf_kernel) has no events of its own: `--ne --probe` runs the resident functions and the windowed
pass once and nothing else, to be run under `rocprofv3 --kernel-trace --stats --output-format csv`, and `--ne --kernel-stats CSV` adds
that trace's per-kernel totals to the result.
--z measures --get_assignment_z_score (two passes over the Beagle file and the depth file in windows; WGSASSIGN_Z_WINDOW_SITES): the
whole-process figures with a plain-text depth file beside the BGZF Beagle file, their ratio windowed / resident, and from one
zscore.assignment_z_scores_windowed in this process the seconds of each pass, the depth ingest's text bytes per pass against the
file's, and the bytes that crossed to the host.  No time target is set: the number to record is that ratio.
What to expect: the device's share of an ingest (BGZF inflate, tokeniser) and the sweeps use the context's one stream and every push
waits for it, so for a BGZF file the device work of consecutive windows is strictly serial; what overlaps a window's sweep is only
the producer thread's reading of the next window (for plain gzip also its inflate).  The windowed run therefore costs the resident
run plus, per window, a reader opened through the index, an ingest created, and the launches and synchronisations of one sweep.
--zref measures --get_reference_z_score (pass A, the fit rounds of the masked leave-one-out fits and the final round, each a pass over
both files; WGSASSIGN_ZREF_WINDOW_SITES): the whole-process figures, their ratio windowed / resident with the pass count, and from one
zscore.reference_z_scores_windowed in this process the seconds of every pass, the fit rounds, the horizons used, and the bytes that
crossed to the host.  The resident run's stopping iterations (minimum, median, maximum, and how many fits were exhausted) are read
from its printed lines: the first horizon (zscore.ZREF_FIRST_HORIZON) is to be set from that record.  What to expect:
(1 + fit rounds + 1) passes x the cost of one windowed pass, plus the resident fit time x (iterations run / iterations needed)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402


def cli_seconds(root, beagle, af, out, env_extra, fit=False, loo=False, ne=False, z=None, zref=None, loo_ds=None):
    """af: the frequency file of --get_pop_like, or with fit (or loo, or ne) the ID file of --get_reference_af.  z: the further
    arguments of --get_assignment_z_score (ID, names and depth files), which then stands in place of --get_pop_like.  zref: all the
    arguments of --get_reference_z_score (af is not looked at).  loo_ds: the file of --loo_downsampled_beagle (with loo).  cli_seconds.stdout: what the last command printed."""
    env = dict(os.environ)
    env.pop("WGSASSIGN_WINDOW_SITES", None)
    env.pop("WGSASSIGN_LOO_WINDOW_SITES", None)
    env.pop("WGSASSIGN_LOO_DS_WINDOW_SITES", None)
    env.pop("WGSASSIGN_NE_WINDOW_SITES", None)
    env.pop("WGSASSIGN_Z_WINDOW_SITES", None)
    env.pop("WGSASSIGN_ZREF_WINDOW_SITES", None)
    env.update(env_extra)
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    what = (["--pop_af_IDs", af, "--get_reference_af"] + (["--loo"] if loo else []) + (["--loo_downsampled_beagle", loo_ds] if loo_ds else []) +
            (["--ne_obs"] if ne else []) if fit or loo or ne
            else ["--get_reference_z_score"] + list(zref) if zref is not None
            else ["--pop_af_file", af, "--get_assignment_z_score"] + list(z) if z is not None
            else ["--pop_af_file", af, "--get_pop_like"])
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "wgsassign_amd.WGSassign", "--beagle", beagle] + what + ["--out", out],
                       cwd=os.path.dirname(out), env=env, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("the command line failed in %s:\n%s" % (root, r.stderr[-2000:]))
    cli_seconds.stdout = r.stdout
    return dt, r.stderr


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "runs": len(xs)}


def fit_leg(a, m, n, K, W):
    """--get_reference_af resident against windowed; one JSON-able dict."""
    import beagle_files
    from wgsassign_amd import device, emMAF
    res = {"bench": "windowed_reference_af", "snps": m, "inds": n, "pops": K, "window_sites": W, "windows": a.windows}
    with tempfile.TemporaryDirectory() as td:
        os.environ["WGSASSIGN_INDEX_DIR"] = td
        bg, ids = os.path.join(td, "x.beagle.gz"), os.path.join(td, "ids.txt")
        beagle_files.write_lowdepth_bgzf(bg, n, m, seed=5)
        IDs = np.array([["Ind%d" % i, "pop%d" % (i * K // n)] for i in range(n)])
        np.savetxt(ids, IDs, fmt="%s", delimiter="\t")
        res["file_mb"] = round(os.path.getsize(bg) / 1e6, 1)
        variants = [("resident_s", ROOT, {})]
        if a.parent_root:
            variants.insert(0, ("parent_resident_s", os.path.abspath(a.parent_root), {}))
        variants.append(("windowed_s", ROOT, {"WGSASSIGN_WINDOW_SITES": str(W)}))
        times = {name: [] for name, _, _ in variants}
        for rep in range(a.repeats + 1):
            for name, root, env in variants:
                dt, err = cli_seconds(root, bg, ids, os.path.join(td, name), env, fit=True)
                if rep:
                    times[name].append(dt)
                if name == "windowed_s" and ("rounds of %d windows" % a.windows) not in err:
                    raise RuntimeError("the windowed run did not use %d windows: %s" % (a.windows, err[-300:]))
        files = {name: open(os.path.join(td, name + ".pop_af.npy"), "rb").read() for name, _, _ in variants}
        res["outputs_identical"] = len(set(files.values())) == 1
        for name in ("parent_resident_s", "resident_s", "windowed_s"):
            res[name] = spread(times[name]) if name in times else None
        ctx = device.get_context()
        res["device"] = ctx.info()["name"].strip()
        for rep in range(2):
            _, iters = emMAF.emMAF_windowed(bg, IDs, 200, 1e-4, W, ctx=ctx)
        st = emMAF.emMAF_windowed.stats
        res.update(rounds=st["rounds"], round_seconds=[round(x, 3) for x in st["round_seconds"]], iterations=[int(i) for i in iters],
                   iterations_round1=st["iterations_round1"], iterations_needed=st["iterations_needed"],
                   chain_iterations=st["chain_iterations"], largest_matrix_bytes=st["largest_matrix_bytes"])
    return res


def loo_leg(a, m, n, K, W):
    """--get_reference_af --loo resident against windowed; one JSON-able dict."""
    import beagle_files
    from wgsassign_amd import device, emMAF, glassy, reader_cy
    res = {"bench": "windowed_loo", "snps": m, "inds": n, "pops": K, "window_sites": W, "windows": a.windows}
    with tempfile.TemporaryDirectory() as td:
        os.environ["WGSASSIGN_INDEX_DIR"] = td
        bg, ids = os.path.join(td, "x.beagle.gz"), os.path.join(td, "ids.txt")
        beagle_files.write_lowdepth_bgzf(bg, n, m, seed=5)
        IDs = np.array([["Ind%d" % i, "pop%d" % (i * K // n)] for i in range(n)])
        np.savetxt(ids, IDs, fmt="%s", delimiter="\t")
        res["file_mb"] = round(os.path.getsize(bg) / 1e6, 1)
        variants = [("resident_s", ROOT, {})]
        if a.parent_root:
            variants.insert(0, ("parent_resident_s", os.path.abspath(a.parent_root), {}))
        variants.append(("windowed_s", ROOT, {"WGSASSIGN_LOO_WINDOW_SITES": str(W)}))
        times = {name: [] for name, _, _ in variants}
        for rep in range(a.repeats + 1):
            for name, root, env in variants:
                dt, err = cli_seconds(root, bg, ids, os.path.join(td, name), env, loo=True)
                if rep:
                    times[name].append(dt)
                if name == "windowed_s" and ("leave-one-out in" not in err or ("rounds of %d windows" % a.windows) not in err):
                    raise RuntimeError("the windowed run did not use %d windows: %s" % (a.windows, err[-300:]))
        files = {name: open(os.path.join(td, name + ".pop_af.npy"), "rb").read() + open(os.path.join(td, name + ".pop_like_LOO.tsv"), "rb").read()
                 for name, _, _ in variants}
        res["outputs_identical"] = len(set(files.values())) == 1
        for name in ("parent_resident_s", "resident_s", "windowed_s"):
            res[name] = spread(times[name]) if name in times else None
        ctx = device.get_context()
        res["device"] = ctx.info()["name"].strip()
        pops = np.unique(IDs[:, 1])
        group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
        for rep in range(2):
            af, pop_iters = emMAF.emMAF_windowed(bg, IDs, 200, 1e-4, W, ctx=ctx)
            ll, _, iters = glassy.loo_windowed(bg, af, IDs, 200, 1e-4, W, 1, need_parts=False, pop_iters=pop_iters, ctx=ctx)
        st = glassy.loo_windowed.stats
        res.update(fit_rounds=emMAF.emMAF_windowed.stats["rounds"], fit_round_seconds=[round(x, 3) for x in emMAF.emMAF_windowed.stats["round_seconds"]],
                   rounds=st["rounds"], round_seconds=[round(x, 3) for x in st["round_seconds"]], extension_rounds=st["extension_rounds"],
                   population_iterations=[int(i) for i in pop_iters], iterations_min_max=[int(iters.min()), int(iters.max())],
                   iterations_round1=st["iterations_round1"], iterations_needed=st["iterations_needed"],
                   chain_iterations=st["chain_iterations"], largest_matrix_bytes=st["largest_matrix_bytes"], margin=glassy.LOO_MARGIN)
        beagle, _, _, _ = reader_cy.stream_to_device(bg, group_of, K, ctx=ctx, names="ends")
        for rep in range(2):
            tm = {}
            ll_r, _ = glassy.loo_device(beagle, beagle, np.array(af), group_of, 200, 1e-4, 1, verbose=False, timings=tm, need_parts=False)
        beagle.close()
        res.update(resident_refit_seconds=round(tm.get("em_seconds", 0.0), 4), resident_score_seconds=round(tm.get("score_seconds", 0.0), 4),
                   resident_iterations_enqueued=tm.get("em_iterations_enqueued"), totals_bit_identical=bool(ll.tobytes() == ll_r.tobytes()))
    return res


def loo_ds_leg(a, m, n, K):
    """--get_reference_af --loo --loo_downsampled_beagle resident against windowed; one JSON-able dict.  m: the reference file's sites;
    four fifths of them are kept."""
    import beagle_files
    from wgsassign_amd import device, emMAF, glassy, windows
    kept = m * 4 // 5
    W = ((kept + a.windows - 1) // a.windows + windows.ALIGN - 1) // windows.ALIGN * windows.ALIGN
    if a.window_sites:
        W = a.window_sites // windows.ALIGN * windows.ALIGN
    nwin = windows.window_count(kept, W)
    res = {"bench": "windowed_loo_downsampled", "snps": m, "kept_snps": kept, "inds": n, "pops": K, "window_sites": W, "windows": nwin}
    with tempfile.TemporaryDirectory() as td:
        os.environ["WGSASSIGN_INDEX_DIR"] = td
        bg, ds, ids = os.path.join(td, "x.beagle.gz"), os.path.join(td, "d.beagle.gz"), os.path.join(td, "ids.txt")
        beagle_files.write_lowdepth_bgzf(bg, n, m, seed=5)
        beagle_files.write_lowdepth_bgzf(ds, n, kept, seed=6)
        IDs = np.array([["Ind%d" % i, "pop%d" % (i * K // n)] for i in range(n)])
        np.savetxt(ids, IDs, fmt="%s", delimiter="\t")
        res.update(file_mb=round(os.path.getsize(bg) / 1e6, 1), downsampled_file_mb=round(os.path.getsize(ds) / 1e6, 1))
        variants = [("resident_s", ROOT, {}), ("windowed_s", ROOT, {"WGSASSIGN_LOO_DS_WINDOW_SITES": str(W)})]
        times = {name: [] for name, _, _ in variants}
        for rep in range(a.repeats + 1):
            for name, root, env in variants:
                dt, err = cli_seconds(root, bg, ids, os.path.join(td, name), env, loo=True, loo_ds=ds)
                if rep:
                    times[name].append(dt)
                if name == "windowed_s" and ("rounds of %d windows of %d kept sites" % (nwin, W)) not in err:
                    raise RuntimeError("the windowed run did not use %d windows: %s" % (nwin, err[-300:]))
        files = {name: open(os.path.join(td, name + ".pop_af.npy"), "rb").read() +
                 open(os.path.join(td, name + ".pop_like_LOO_downsampled.tsv"), "rb").read() for name, _, _ in variants}
        res["outputs_identical"] = len(set(files.values())) == 1
        for name in ("resident_s", "windowed_s"):
            res[name] = spread(times[name])
        res["windowed_over_resident"] = round(res["windowed_s"]["median"] / res["resident_s"]["median"], 3)
        ctx = device.get_context()
        res["device"] = ctx.info()["name"].strip()
        keep = np.arange(m) < kept
        for rep in range(2):
            af, pop_iters = emMAF.emMAF_windowed(bg, IDs, 200, 1e-4, W, ctx=ctx, keep=keep)
            glassy.loo_windowed(bg, af, IDs, 200, 1e-4, W, 1, need_parts=False, pop_iters=pop_iters, ctx=ctx, keep=keep, scored_path=ds)
        st = glassy.loo_windowed.stats
        res.update(fit_rounds=emMAF.emMAF_windowed.stats["rounds"], rounds=st["rounds"], round_seconds=[round(x, 3) for x in st["round_seconds"]],
                   extension_rounds=st["extension_rounds"], scored_passes=st["scored_passes"], matrices=st["matrices"],
                   largest_matrix_bytes=st["largest_matrix_bytes"])
    return res


NE_KERNELS = ("fisher_window_kernel", "fisher_pop_kernel", "fisher_ind_sites_kernel", "pairwise_leaf_kernel", "pairwise_combine_kernel",
              "fisher_stream_combine_kernel")
NE_OUTPUTS = (".pop_af.npy", ".fisher_obs.npy", ".ne_obs.npy", ".ne_obs.txt", ".ne_ind.txt")


def ne_files(td, n, m, K):
    import beagle_files
    bg, ids = os.path.join(td, "x.beagle.gz"), os.path.join(td, "ids.txt")
    beagle_files.write_lowdepth_bgzf(bg, n, m, seed=5)
    IDs = np.array([["Ind%d" % i, "pop%d" % (i * K // n)] for i in range(n)])
    np.savetxt(ids, IDs, fmt="%s", delimiter="\t")
    return bg, ids, IDs


def ne_passes(bg, IDs, W, K, ctx, repeats):
    """The resident functions and the windowed pass on the same file and frequencies, `repeats` times each; (all four results equal,
    the windowed pass's stats)."""
    from wgsassign_amd import emMAF, fisher, reader_cy
    af, _ = emMAF.emMAF_windowed(bg, IDs, 200, 1e-4, W, ctx=ctx)
    pops = np.unique(IDs[:, 1])
    group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
    beagle, _, _, _ = reader_cy.stream_to_device(bg, group_of, K, ctx=ctx, names="ends")
    for rep in range(repeats):
        f_r, ne_r = fisher.fisher_obs(None, af, IDs, 1, beagle=beagle)
        ind_r = fisher.fisher_obs_ind(None, af, IDs, 1, beagle=beagle)
    beagle.close()
    for rep in range(repeats):
        f_w, ne_w, mean_w, ind_w = fisher.fisher_obs_windowed(bg, af, IDs, W, ctx=ctx)
    same = all(np.asarray(x).tobytes() == y.tobytes() for x, y in ((f_w, f_r), (ne_w, ne_r), (mean_w, np.mean(ne_r, axis=0)), (ind_w, ind_r)))
    return same, fisher.fisher_obs_windowed.stats


def kernel_totals(csv_path):
    """{kernel: [calls, total ms]} of the --ne kernels from a rocprofv3 *_kernel_stats.csv."""
    import csv
    out = {}
    with open(csv_path) as fh:
        for row in csv.DictReader(fh):
            for k in NE_KERNELS:
                if k in row["Name"]:
                    out[k] = [int(row["Calls"]), round(float(row["TotalDurationNs"]) / 1e6, 4)]
    return out


def ne_leg(a, m, n, K, W):
    """--get_reference_af --ne_obs resident against windowed; one JSON-able dict."""
    from wgsassign_amd import device
    res = {"bench": "windowed_ne_obs", "snps": m, "inds": n, "pops": K, "window_sites": W, "windows": a.windows}
    with tempfile.TemporaryDirectory() as td:
        os.environ["WGSASSIGN_INDEX_DIR"] = td
        bg, ids, IDs = ne_files(td, n, m, K)
        ctx = device.get_context()
        if a.probe:
            same, _ = ne_passes(bg, IDs, W, K, ctx, 1)
            return {"bench": "windowed_ne_obs_probe", "results_bit_identical": bool(same)}
        res["file_mb"] = round(os.path.getsize(bg) / 1e6, 1)
        variants = [("resident_s", ROOT, {})]
        if a.parent_root:
            variants.insert(0, ("parent_resident_s", os.path.abspath(a.parent_root), {}))
        variants.append(("windowed_s", ROOT, {"WGSASSIGN_NE_WINDOW_SITES": str(W)}))
        times = {name: [] for name, _, _ in variants}
        for rep in range(a.repeats + 1):
            for name, root, env in variants:
                dt, err = cli_seconds(root, bg, ids, os.path.join(td, name), env, ne=True)
                if rep:
                    times[name].append(dt)
                if name == "windowed_s" and ("Fisher information in %d windows" % a.windows) not in err:
                    raise RuntimeError("the windowed run did not use %d windows: %s" % (a.windows, err[-300:]))
        files = {name: b"".join(open(os.path.join(td, name + suffix), "rb").read() for suffix in NE_OUTPUTS) for name, _, _ in variants}
        res["outputs_identical"] = len(set(files.values())) == 1
        for name in ("parent_resident_s", "resident_s", "windowed_s"):
            res[name] = spread(times[name]) if name in times else None
        res["device"] = ctx.info()["name"].strip()
        res["kernels_id"] = (device._lib.load().wgs_kernels_id() or b"").decode()
        same, st = ne_passes(bg, IDs, W, K, ctx, 2)
        res.update(results_bit_identical=bool(same), fused_sweep_ms_per_window=[round(x, 4) for x in st["sweep_ms"]],
                   fused_sweeps_ms=round(sum(st["sweep_ms"]), 4), windowed_pass_seconds=round(st["seconds"], 3),
                   largest_matrix_bytes=st["largest_matrix_bytes"])
    if a.kernel_stats:
        # one resident run and one windowed pass under the kernel trace (--probe): the resident trio against the fused sweep
        k = kernel_totals(a.kernel_stats)
        res["traced_kernels_calls_ms"] = k
        trio = [k.get(x, [0, 0.0])[1] for x in ("fisher_pop_kernel", "fisher_ind_sites_kernel", "pairwise_leaf_kernel")]
        fused = k.get("fisher_window_kernel", [0, None])[1]
        # (the windowed pass's own row route over the file's last, shorter chunk runs two of the trio's kernels, too: a fraction of a
        # chunk against the resident path's whole file)
        res["traced_resident_trio_ms"] = round(sum(trio), 4)
        res["traced_fused_ms"] = fused
    return res


def z_leg(a, m, n, K, W):
    """--get_assignment_z_score resident against windowed; one JSON-able dict."""
    import beagle_files
    import bench_depth_ingest
    from wgsassign_amd import device, zscore
    res = {"bench": "windowed_assignment_z_score", "snps": m, "inds": n, "pops": K, "window_sites": W, "windows": a.windows}
    with tempfile.TemporaryDirectory() as td:
        os.environ["WGSASSIGN_INDEX_DIR"] = td
        bg, ids, names, af = (os.path.join(td, x) for x in ("x.beagle.gz", "ids.txt", "names.txt", "x.pop_af.npy"))
        beagle_files.write_lowdepth_bgzf(bg, n, m, seed=5)
        IDs = np.array([["Ind%d" % i, "pop%d" % (i * K // n)] for i in range(n)])
        np.savetxt(ids, IDs, fmt="%s", delimiter="\t")
        pops = np.unique(IDs[:, 1])
        np.savetxt(names, pops, fmt="%s")
        np.save(af, np.random.default_rng(5).uniform(0.05, 0.95, size=(m, K)).astype(np.float32))
        paths, depth_text_bytes, _ = bench_depth_ingest.write_files(td, m, n, ("text",), False)
        ad = paths["text"]
        res.update(file_mb=round(os.path.getsize(bg) / 1e6, 1), depth_file_mb=round(depth_text_bytes / 1e6, 1))
        more = ["--pop_af_IDs", ids, "--pop_names", names, "--ind_ad_file", ad]
        variants = [("resident_s", ROOT, {})]
        if a.parent_root:
            variants.insert(0, ("parent_resident_s", os.path.abspath(a.parent_root), {}))
        variants.append(("windowed_s", ROOT, {"WGSASSIGN_Z_WINDOW_SITES": str(W)}))
        times = {name: [] for name, _, _ in variants}
        for rep in range(a.repeats + 1):
            for name, root, env in variants:
                dt, err = cli_seconds(root, bg, af, os.path.join(td, name), env, z=more)
                if rep:
                    times[name].append(dt)
                if name == "windowed_s" and ("passes over %d windows" % a.windows) not in err:
                    raise RuntimeError("the windowed run did not use %d windows: %s" % (a.windows, err[-300:]))
        files = {name: open(os.path.join(td, name + ".z_ind.txt"), "rb").read() for name, _, _ in variants}
        res["outputs_identical"] = len(set(files.values())) == 1
        for name in ("parent_resident_s", "resident_s", "windowed_s"):
            res[name] = spread(times[name]) if name in times else None
        res["windowed_over_resident"] = round(res["windowed_s"]["median"] / res["resident_s"]["median"], 3)
        ctx = device.get_context()
        res["device"] = ctx.info()["name"].strip()
        A = np.load(af, mmap_mode="r")
        for rep in range(2):
            zscore.assignment_z_scores_windowed(bg, ad, A, IDs, pops, window_sites=W, say=lambda *_: None, ctx=ctx)
        st = zscore.assignment_z_scores_windowed.stats
        res.update(rounds=st["rounds"], pass_a_seconds=[round(x, 3) for x in st["seconds_a"]], pass_b_seconds=[round(x, 3) for x in st["seconds_b"]],
                   depth_text_bytes=depth_text_bytes, depth_text_bytes_per_pass=[int(d["text_bytes"]) for d in st["depth_a"] + st["depth_b"]],
                   downloaded_bytes=int(st["downloaded_bytes"]))
    return res


def zref_leg(a, m, n, K, W):
    """--get_reference_z_score resident against windowed; one JSON-able dict."""
    import beagle_files
    from wgsassign_amd import device, zscore
    res = {"bench": "windowed_reference_z_score", "snps": m, "inds": n, "pops": K, "window_sites": W, "windows": a.windows}
    with tempfile.TemporaryDirectory() as td:
        os.environ["WGSASSIGN_INDEX_DIR"] = td
        bg, ids, names = (os.path.join(td, x) for x in ("x.beagle.gz", "ids.txt", "names.txt"))
        beagle_files.write_lowdepth_bgzf(bg, n, m, seed=5)
        IDs = np.array([["Ind%d" % i, "pop%d" % (i * K // n)] for i in range(n)])
        np.savetxt(ids, IDs, fmt="%s", delimiter="\t")
        pops = np.unique(IDs[:, 1])
        group_of = np.searchsorted(pops, IDs[:, 1]).astype(np.int32)
        np.savetxt(names, pops, fmt="%s")
        # the read counts behind the Beagle file's likelihoods: the masked fits need kept sites, which unrelated depths do not give
        ad = os.path.join(td, "ad.txt")
        depth_text_bytes = beagle_files.write_lowdepth_depths(ad, n, m, seed=5)
        res.update(file_mb=round(os.path.getsize(bg) / 1e6, 1), depth_file_mb=round(depth_text_bytes / 1e6, 1))
        argv = ["--pop_af_IDs", ids, "--pop_names", names, "--ind_ad_file", ad]
        variants = [("resident_s", ROOT, {})]
        if a.parent_root:
            variants.insert(0, ("parent_resident_s", os.path.abspath(a.parent_root), {}))
        variants.append(("windowed_s", ROOT, {"WGSASSIGN_ZREF_WINDOW_SITES": str(W)}))
        times = {name: [] for name, _, _ in variants}
        resident_lines = []
        for rep in range(a.repeats + 1):
            for name, root, env in variants:
                dt, err = cli_seconds(root, bg, None, os.path.join(td, name), env, zref=argv)
                print("%s: %.1f s" % (name, dt), file=sys.stderr, flush=True)
                if rep:
                    times[name].append(dt)
                if name == "resident_s":
                    resident_lines = cli_seconds.stdout.splitlines()
                if name == "windowed_s" and ("passes over %d windows" % a.windows) not in err:
                    raise RuntimeError("the windowed run did not use %d windows: %s" % (a.windows, err[-300:]))
        files = {name: open(os.path.join(td, name + ".reference_z_ind.txt"), "rb").read() for name, _, _ in variants}
        res["outputs_identical"] = len(set(files.values())) == 1
        for name in ("parent_resident_s", "resident_s", "windowed_s"):
            res[name] = spread(times[name]) if name in times else None
        res["windowed_over_resident"] = round(res["windowed_s"]["median"] / res["resident_s"]["median"], 3)
        # the resident run's stopping iterations, from its own lines: what the first horizon is to be set from
        stops = [int(ln.rsplit(" ", 1)[1]) for ln in resident_lines if ln.startswith("EM (MAF) converged at iteration: ")]
        res["resident_stopping_iterations"] = ({"min": min(stops), "median": statistics.median(stops), "max": max(stops), "fits": len(stops),
                                                "exhausted": n - len(stops)} if stops else {"fits": 0, "exhausted": n})
        ctx = device.get_context()
        res["device"] = ctx.info()["name"].strip()
        for rep in range(2):
            zscore.reference_z_scores_windowed(bg, ad, IDs, group_of, 200, 1e-4, window_sites=W, say=lambda *_: None, ctx=ctx)
        st = zscore.reference_z_scores_windowed.stats
        res.update(rounds=st["rounds"], passes=st["passes"], fit_rounds=st["fit_rounds"], horizons=st["horizons"], first_horizon=st["first_horizon"],
                   pass_a_seconds=[round(x, 3) for x in st["seconds_a"]], fit_round_seconds=[[round(x, 3) for x in r] for r in st["seconds_fit"]],
                   final_round_seconds=[[round(x, 3) for x in r] for r in st["seconds_final"]], downloaded_bytes=int(st["downloaded_bytes"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zref", action="store_true", help="measure --get_reference_z_score (the reference z-scores in windows)")
    ap.add_argument("--z", action="store_true", help="measure --get_assignment_z_score (the z-scores in windows)")
    ap.add_argument("--ne", action="store_true", help="measure --get_reference_af --ne_obs (the Fisher information in windows)")
    ap.add_argument("--probe", action="store_true", help="with --ne: only run the resident functions and the windowed pass once (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="with --ne: a rocprofv3 *_kernel_stats.csv of a --ne --probe run, added to the result")
    ap.add_argument("--loo", action="store_true", help="measure --get_reference_af --loo (the leave-one-out run in windows)")
    ap.add_argument("--loo-ds", action="store_true", help="measure --get_reference_af --loo --loo_downsampled_beagle (two files in windows)")
    ap.add_argument("--fit", action="store_true", help="measure --get_reference_af (the fit in windows) instead of --get_pop_like")
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--inds", type=int, default=200)
    ap.add_argument("--pops", type=int, default=5)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--window-sites", type=int, default=0, help="the window itself (a multiple of 8192) instead of --windows")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import beagle_files
    from wgsassign_amd import device, glassy, reader_cy, windows
    m, n, K = a.snps, a.inds, a.pops
    if a.loo_ds:
        line = json.dumps(loo_ds_leg(a, m, n, K))
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return
    per_window = (m + a.windows - 1) // a.windows
    W = (per_window + windows.ALIGN - 1) // windows.ALIGN * windows.ALIGN          # rounded UP to whole chunks of 8192
    if a.window_sites:                                                             # (--z: windows of 262144 sites by default)
        W = a.window_sites // windows.ALIGN * windows.ALIGN
        a.windows = windows.window_count(m, W)
    elif a.z or a.zref:
        W = 262144
        a.windows = windows.window_count(m, W)
    if windows.window_count(m, W) != a.windows:
        raise SystemExit("%d sites cannot be cut into %d windows of a multiple of %d sites" % (m, a.windows, windows.ALIGN))
    if a.fit or a.loo or a.ne or a.z or a.zref:
        line = json.dumps(zref_leg(a, m, n, K, W) if a.zref else z_leg(a, m, n, K, W) if a.z else ne_leg(a, m, n, K, W) if a.ne else loo_leg(a, m, n, K, W) if a.loo
                          else fit_leg(a, m, n, K, W))
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return
    res = {"bench": "windowed_pop_like", "snps": m, "inds": n, "pops": K, "window_sites": W, "windows": a.windows,
           "kernels_id": None, "device": None}
    with tempfile.TemporaryDirectory() as td:
        os.environ["WGSASSIGN_INDEX_DIR"] = td
        bg, af = os.path.join(td, "x.beagle.gz"), os.path.join(td, "x.pop_af.npy")
        t0 = time.perf_counter()
        beagle_files.write_lowdepth_bgzf(bg, n, m, seed=5)
        A = np.random.default_rng(5).uniform(0.02, 0.98, size=(m, K)).astype(np.float32)
        np.save(af, A)
        res["file_mb"] = round(os.path.getsize(bg) / 1e6, 1)
        res["write_s"] = round(time.perf_counter() - t0, 1)
        variants = [("resident_s", ROOT, {})]
        if a.parent_root:
            variants.insert(0, ("parent_resident_s", os.path.abspath(a.parent_root), {}))
        variants.append(("windowed_s", ROOT, {"WGSASSIGN_WINDOW_SITES": str(W)}))
        times = {name: [] for name, _, _ in variants}
        for rep in range(a.repeats + 1):                  # (the first repeat warms up: index cache, page cache, code objects)
            for name, root, env in variants:
                dt, err = cli_seconds(root, bg, af, os.path.join(td, name), env)
                if rep:
                    times[name].append(dt)
                if name == "windowed_s" and ("scored in %d windows" % a.windows) not in err:
                    raise RuntimeError("the windowed run did not use %d windows: %s" % (a.windows, err[-300:]))
        texts = {name: open(os.path.join(td, name + ".pop_like.txt"), "rb").read() for name, _, _ in variants}
        res["outputs_identical"] = len(set(texts.values())) == 1
        for name in ("parent_resident_s", "resident_s", "windowed_s"):
            res[name] = spread(times[name]) if name in times else None
        # the sweeps alone, in this process
        ctx = device.get_context()
        res["device"] = ctx.info()["name"].strip()
        res["kernels_id"] = (device._lib.load().wgs_kernels_id() or b"").decode()
        resident_ms, windowed_ms, each = [], [], None
        beagle, _, _, _ = reader_cy.stream_to_device(bg, ctx=ctx, names="ends")
        afs = device.AFSet.from_host(A, ctx=ctx)
        for rep in range(a.repeats + 1):
            out_r, _ = device.assign(beagle, afs)
            if rep and device.assign.last_ms >= 0:
                resident_ms.append(device.assign.last_ms)
        afs.close()
        beagle.close()
        for rep in range(a.repeats + 1):
            out_w = glassy.assignLL_windowed(bg, A, W, ctx=ctx)
            if rep:
                each = [round(x, 3) for x in glassy.assignLL_windowed.stats["sweep_ms"]]
                if min(each) >= 0:            # (-1: a sweep's time was not to be had while the class codes' memory was being allocated)
                    windowed_ms.append(sum(glassy.assignLL_windowed.stats["sweep_ms"]))
        res["totals_bit_identical"] = bool(np.array_equal(out_r, out_w))
        res["resident_sweep_ms"] = spread(resident_ms) if resident_ms else None
        res["windowed_sweeps_ms"] = spread(windowed_ms) if windowed_ms else None
        res["window_sweep_ms_last_repeat"] = each
        res["largest_matrix_bytes"] = glassy.assignLL_windowed.stats["largest_matrix_bytes"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
