#!/usr/bin/env python3
"""Generate tests/golden/fisher_cases.npz from the REAL reference on the two term grids and the signed-zero populations of
tests/fisher_cases.py (fisher_cases.GOLDEN).

Run as make_golden_zscore_classes.py is run: build the reference in a scratch copy (python3 setup.py build_ext --inplace) and run this
file with that copy on PYTHONPATH, from a working directory other than this repository's root (whose own WGSassign package would
take the reference's place).  Per input (`finite`, `hostile`, `zeros`) the reference's fisher.fisher_obs and fisher.fisher_obs_ind, and per
individual the two rows fisher_cy.fisher_obs_ind and fisher_cy.ne_obs_ind fill from zeros, exactly as fisher.py:53-57 calls them.

Everything written is data: the generator's arguments, the digest of the inputs and what the reference's functions returned.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fisher_cases  # noqa: E402
from WGSassign import fisher, fisher_cy  # noqa: E402

assert os.path.dirname(os.path.abspath(fisher.__file__)) != os.path.join(os.path.dirname(os.path.dirname(HERE)), "WGSassign"), \
    "this is the repository's own WGSassign package, not the reference"


def main():
    arrays = {}
    for variant, (builder, gen) in fisher_cases.GOLDEN.items():
        grid = getattr(fisher_cases, builder)(**gen)
        L, af, IDs = grid["L"], grid["af"], grid["IDs"]
        pops = np.unique(IDs[:, 1])
        m, n = L.shape[0], L.shape[1] // 2
        with np.errstate(all="ignore"):
            f_obs, ne_obs = fisher.fisher_obs(L, af.copy(), IDs, 2)
            ne_ind = fisher.fisher_obs_ind(L, af.copy(), IDs, 2)
        f_rows = np.zeros((n, m), dtype=np.float32)
        ne_rows = np.zeros((n, m), dtype=np.float32)
        for i in range(n):
            pop_i = int(np.argwhere(pops == IDs[i, 1])[0][0])
            fisher_cy.fisher_obs_ind(L, af, 1, i, pop_i, f_rows[i])
            fisher_cy.ne_obs_ind(f_rows[i], af, 1, pop_i, ne_rows[i])
        arrays[variant + "_gen"] = np.array(repr(gen))
        arrays[variant + "_digest"] = np.array(fisher_cases.digest(grid))
        for name, a in (("f_obs", f_obs), ("ne_obs", ne_obs), ("ne_ind", ne_ind), ("f_rows", f_rows), ("ne_rows", ne_rows)):
            assert a.dtype == np.float32
            arrays[variant + "_" + name] = a
        print(variant, "n", n, "m", m, "K", len(pops), "non-finite terms", int((~np.isfinite(f_rows)).sum()), "of", f_rows.size,
              "negative zeros in ne", int(((ne_rows == 0) & np.signbit(ne_rows)).sum()))
    path = os.path.join(HERE, "fisher_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
