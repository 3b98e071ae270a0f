#!/usr/bin/env python3
"""Generate tests/golden/rmse_cases.npz from the REAL reference on the enumerated convergence chains of tests/rmse_cases.py
(rmse_cases.golden_cases()).

Run as make_golden_em_cases.py is run: build the reference in a scratch copy (python3 setup.py build_ext --inplace) and run this file
with that copy on PYTHONPATH, from a working directory other than this repository's root (whose own WGSassign package would take the
reference's place).  Per case: emMAF_cy.rmse1d(a, b) -- the serial float32 sum from zero, divided by the length, the square root in
double.  rmse1d has no carry, so a case's own carry is not in it; the CPU test continues the chain from a carry with a plain loop.

Everything written is data: the cases' names, the digests of their inputs -- the inputs themselves are rebuilt by rmse_cases, the two
long ones from their seeds -- and what the reference's function returned.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rmse_cases  # noqa: E402
from WGSassign import emMAF, emMAF_cy  # noqa: E402

assert os.path.dirname(os.path.abspath(emMAF.__file__)) != os.path.join(os.path.dirname(os.path.dirname(HERE)), "WGSassign"), \
    "this is the repository's own WGSassign package, not the reference"


def main():
    cases = rmse_cases.golden_cases()
    with np.errstate(all="ignore"):
        values = np.array([emMAF_cy.rmse1d(np.array(c.a), np.array(c.b)) for c in cases], dtype=np.float64)
    arrays = {"names": np.array([repr(c) for c in cases]), "digests": np.array([rmse_cases.digest(c) for c in cases]), "rmse1d": values}
    print(len(cases), "cases; NaN", int(np.isnan(values).sum()), "inf", int(np.isinf(values).sum()), "zero", int((values == 0).sum()))
    path = os.path.join(HERE, "rmse_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
