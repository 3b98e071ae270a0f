#!/usr/bin/env python3
"""Generate tests/golden/allele_counts.npz from the REAL reference script WGSassign/allele_counts_beagle.py.

Run where the reference is available only, in the manner of make_golden_zscore.py:

    python tests/golden/make_golden_allele_counts.py /path/to/reference

The script is started from its own path as a child process on a generated ANGSD counts file (tests/synth_counts.py) and the
selector file that goes with it.  Everything written is data: the generator's arguments and the digest of what it made, the
selector table, the (m, 2n) array the script wrote, and the digest of the text inside its gzipped output file.
"""
import gzip
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import synth_counts  # noqa: E402

GEN = dict(m=301, n=9, seed=11, depth=1.5)


def main():
    script = os.path.join(sys.argv[1], "WGSassign", "allele_counts_beagle.py")
    counts, majmin = synth_counts.make_counts(**GEN)
    with tempfile.TemporaryDirectory() as tmp:
        cpath, mpath = os.path.join(tmp, "g.counts.gz"), os.path.join(tmp, "g.majmin.txt")
        synth_counts.write_counts(cpath, counts)
        synth_counts.write_majmin(mpath, majmin)
        subprocess.run([sys.executable, script, cpath, mpath], check=True)
        text = gzip.open(cpath + ".majmin.counts.txt.gz", "rb").read()
    out = np.loadtxt(text.decode().splitlines(), dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "allele_counts.npz"), gen=repr(GEN), counts_digest=hashlib.sha256(counts.tobytes()).hexdigest(),
                        majmin=majmin.astype(np.uint8), out=out, text_digest=hashlib.sha256(text).hexdigest())
    print("wrote allele_counts.npz:", out.shape, hashlib.sha256(text).hexdigest()[:16])


if __name__ == "__main__":
    main()
