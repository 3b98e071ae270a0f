#!/usr/bin/env python3
"""Seconds from an allele-depth file's path to the resident depth table: the streamed path (zscore.DepthTable.from_file: tokenised
on the device) against the parent path (zscore.read_depths = np.loadtxt, then DepthTable(beagle, AD)), same process, same files,
page cache warm for both.  Prints one JSON line.

    python tools/bench_depth_ingest.py [--shapes 1000000x200,2000000x500] [--formats text,gzip,bgzf] [--repeats 3] [--no-parent]

Per shape: Poisson(1.5) depths written as text, gzip and BGZF (and the matching ANGSD counts file as gzip, unless --no-counts);
(a) the parent path once per format, (b) from_file `repeats` times per format (the first run is the warm-up and is reported
separately), (c) counts mode.  --time-kernel: the tokeniser kernel's own milliseconds and the text bytes per second they imply, in a run of
its own (HIP events around every launch cost a synchronisation per chunk).
"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def text_blocks(m, cols, seed, lam, rows=20000):
    """The table's text in blocks of `rows` lines, without formatting numbers one by one: tens digit (dropped when 0), ones digit,
    tab -- the last column's separator is the newline.  Yields (bytes, values)."""
    rng = np.random.default_rng(seed)
    for r0 in range(0, m, rows):
        v = np.minimum(rng.poisson(lam, size=(min(rows, m - r0), cols)), 99).astype(np.uint8)
        t = np.zeros(v.shape + (3,), dtype=np.uint8)
        t[:, :, 0] = np.where(v >= 10, 48 + v // 10, 0)
        t[:, :, 1] = 48 + v % 10
        t[:, :, 2] = 9
        t[:, -1, 2] = 10
        flat = t.reshape(-1)
        yield flat[flat != 0].tobytes(), v


def write_files(tmp, m, n, formats, counts):
    import beagle_files
    paths = {}
    outs = {}
    if "text" in formats:
        paths["text"] = os.path.join(tmp, "ad.txt")
        outs["text"] = open(paths["text"], "wb")
    if "gzip" in formats:
        paths["gzip"] = os.path.join(tmp, "ad.txt.gz")
        outs["gzip"] = gzip.open(paths["gzip"], "wb", compresslevel=1)
    if "bgzf" in formats:
        paths["bgzf"] = os.path.join(tmp, "ad.bgzf.gz")
        outs["bgzf"] = open(paths["bgzf"], "wb")
    nbytes = 0
    for data, _ in text_blocks(m, 2 * n, 1, 0.75):          # Poisson(1.5) reads per individual over the two alleles
        nbytes += len(data)
        for k, fh in outs.items():
            if k == "bgzf":
                for i in range(0, len(data), 60000):
                    fh.write(beagle_files.bgzf_member(data[i:i + 60000], 1))
            else:
                fh.write(data)
    if "bgzf" in outs:
        outs["bgzf"].write(beagle_files.bgzf_member(b"", 1))
    for fh in outs.values():
        fh.close()
    majmin = None
    if counts:
        paths["counts"] = os.path.join(tmp, "ad.counts.gz")
        rng = np.random.default_rng(2)
        majmin = np.empty((m, 2), dtype=np.uint8)
        majmin[:, 0] = rng.integers(0, 4, size=m)
        majmin[:, 1] = (majmin[:, 0] + rng.integers(1, 4, size=m)) % 4
        with gzip.open(paths["counts"], "wb", compresslevel=1) as fh:
            fh.write(b"h\t" * (4 * n) + b"\n")
            for data, _ in text_blocks(m, 4 * n, 3, 0.375):
                fh.write(data)
    return paths, nbytes, majmin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000x200,2000000x500")
    ap.add_argument("--formats", default="text,gzip,bgzf")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--no-counts", action="store_true")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--time-kernel", action="store_true",
                    help="HIP events around every launch of the tokeniser (a synchronisation per chunk: the wall times of such a run are not the path's)")
    args = ap.parse_args()
    if args.time_kernel:
        os.environ["WGSASSIGN_INGEST_TIME_KERNEL"] = "1"        # read once per process, at the first launch
    from wgsassign_amd import zscore
    from wgsassign_amd.device import DeviceBeagle, get_context
    ctx = get_context()
    result = dict(bench="depth_ingest", device=ctx.info()["name"], shapes=[])
    formats = args.formats.split(",")
    for shape in args.shapes.split(","):
        m, n = (int(x) for x in shape.split("x"))
        with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
            paths, nbytes, majmin = write_files(tmp, m, n, formats, not args.no_counts)
            b = DeviceBeagle(m, n)
            rec = dict(m=m, n=n, text_bytes=nbytes, formats={})
            for fmt in formats:
                f = dict(file_bytes=os.path.getsize(paths[fmt]))
                open(paths[fmt], "rb").read(1)
                times = []
                for _ in range(args.repeats + 1):
                    t0 = time.perf_counter()
                    t = zscore.DepthTable.from_file(b, paths[fmt])
                    ctx.sync()
                    times.append(time.perf_counter() - t0)
                    stats = t.ingest_stats
                    t.close()
                f["from_file_first_s"] = times[0]
                f["from_file_s"] = sorted(times[1:])
                f["from_file_median_s"] = float(np.median(times[1:]))
                f["host_peak_bytes"], f["chunks"], f["members_on_device"] = stats["host_peak_bytes"], stats["chunks"], stats["members_on_device"]
                if args.time_kernel:
                    f["tokenise_kernel_ms"] = stats["tokenise_ms"]
                    f["tokenise_text_GBps"] = nbytes / max(stats["tokenise_ms"], 1e-9) / 1e6
                if not args.no_parent:
                    t0 = time.perf_counter()
                    AD = zscore.read_depths(paths[fmt])
                    t1 = time.perf_counter()
                    t = zscore.DepthTable(b, AD)
                    ctx.sync()
                    f["parent_s"] = time.perf_counter() - t0
                    f["parent_loadtxt_s"] = t1 - t0
                    f["speedup"] = f["parent_s"] / f["from_file_median_s"]
                    t.close()
                    del AD
                rec["formats"][fmt] = f
            if majmin is not None:
                times = []
                for _ in range(args.repeats + 1):
                    t0 = time.perf_counter()
                    t = zscore.DepthTable.from_file(b, paths["counts"], counts=True, majmin=majmin)
                    ctx.sync()
                    times.append(time.perf_counter() - t0)
                    t.close()
                rec["counts_gzip"] = dict(file_bytes=os.path.getsize(paths["counts"]), first_s=times[0], median_s=float(np.median(times[1:])))
            b.close()
            result["shapes"].append(rec)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
