"""`python -m wgsassign_amd.allele_counts COUNTS MAJMIN [--out FILE]`: the counterpart of the reference's allele_counts_beagle.py.

ANGSD's -dumpCounts 4 output (COUNTS: one header line, then A C G T reads per individual and site) and the sites' major and minor
alleles (MAJMIN: one header line, the selectors 0..3 in the columns at positions 1 and 2) become the (m, 2n) table of --ind_ad_file:
per individual the reads of the major and of the minor allele.  The counts are tokenised on the GPU into a depth table
(zscore.stream_table) and written chunk by chunk from wgs_depth_download_rows, with the bytes np.savetxt(..., fmt="%d") writes;
the output is gzipped when its name ends in .gz, as np.savetxt does.  The site count comes from MAJMIN, the individuals from the
first line of COUNTS.
"""
import argparse
import ctypes
import gzip
import os

import numpy as np

from . import _lib, zscore
from ._lib import check, i32p


def convert(counts, majmin, out=None, chunk_rows=None, chunk_bytes=None):
    from .device import get_context
    out = out or counts + ".majmin.counts.txt.gz"
    sel = zscore.read_majmin(majmin)
    m = sel.shape[0]
    lib = _lib.load()
    r = ctypes.c_void_p()
    check(lib.wgs_reader_open_table(os.fsencode(counts), 1, 1, ctypes.byref(r)))
    cols = lib.wgs_reader_table_columns(r)
    lib.wgs_reader_close(r)
    n = cols // 4
    if n < 1:
        raise ValueError("%s: the first data line has %d columns, an individual needs four" % (counts, cols))
    ctx = get_context()
    h = ctypes.c_void_p()
    check(lib.wgs_depth_create_shape(ctx.handle, m, n, ctypes.byref(h)))
    try:
        stats = zscore.stream_table(h, m, counts, counts=True, majmin=sel, chunk_bytes=chunk_bytes)
        step = chunk_rows or max(1, (16 << 20) // (8 * n))
        with (gzip.open(out, "wb") if out.endswith(".gz") else open(out, "wb")) as fh:
            for row0 in range(0, m, step):
                rows = np.empty((min(step, m - row0), 2 * n), dtype=np.int32)
                check(lib.wgs_depth_download_rows(h, i32p(rows), row0, rows.shape[0]))
                np.savetxt(fh, rows, fmt="%d")
    finally:
        lib.wgs_depth_destroy(h)
    return out, m, n, stats


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m wgsassign_amd.allele_counts", description=__doc__.split("\n\n")[0])
    ap.add_argument("counts", metavar="COUNTS", help="ANGSD -dumpCounts 4 output (.counts.gz)")
    ap.add_argument("majmin", metavar="MAJMIN", help="major and minor allele per site (0..3), one header line")
    ap.add_argument("--out", metavar="FILE", help="output (default: COUNTS.majmin.counts.txt.gz)")
    args = ap.parse_args(argv)
    out, m, n, _ = convert(args.counts, args.majmin, args.out)
    print("Saved major/minor allele counts of %d sites and %d individuals as %s" % (m, n, out))


if __name__ == "__main__":
    main()
