#!/usr/bin/env python3
"""Generate tests/golden/score_cases.npz from the REAL reference on the enumerated scoring inputs of tests/score_cases.py
(score_cases.GOLDEN).

Run as make_golden_em_cases.py is run: build the reference in a scratch copy (python3 setup.py build_ext --inplace) and run this file
with that copy on PYTHONPATH, from a working directory other than this repository's root (whose own WGSassign package would take the
reference's place).  Per variant (`finite`, `hostile`), on one individual of every pair family and one population of every frequency
family of the `grid` case: glassy_cy.loglike into zeros for every (individual, population) -- the per-site values --, the same into a
non-zero start vector (ordinary, -inf, huge, NaN and +inf starts in turn) for score_cases.GOLDEN_START_CELLS, which is what
loglike_site_kernel mirrors, glassy.assignLL, and utils.partition_loglikes of the per-site vectors for P = 1, 3 and 64.

Everything written is data: the generator's arguments, the digest of the inputs and what the reference's functions returned.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import score_cases  # noqa: E402
from WGSassign import glassy, glassy_cy, utils  # noqa: E402

assert os.path.dirname(os.path.abspath(glassy.__file__)) != os.path.join(os.path.dirname(os.path.dirname(HERE)), "WGSassign"), \
    "this is the repository's own WGSassign package, not the reference"


def main():
    arrays = {}
    for name, gen in score_cases.GOLDEN.items():
        case, L, A, start = score_cases.golden_inputs(name)
        rec = score_cases.golden_record(glassy_cy.loglike, utils.partition_loglikes, name)
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            ll = glassy.assignLL(L, A.copy(), 1)
        arrays[name + "_gen"] = np.array(repr(gen))
        arrays[name + "_digest"] = np.array(score_cases.digest(case))
        arrays[name + "_assignLL"] = ll
        for key, val in rec.items():
            assert val.dtype == np.float32
            arrays[name + "_" + key] = val
        V = rec["loglike"]
        print(name, "individuals", gen["individuals"], "populations", gen["populations"], "m", L.shape[0], "per-site values", V.size, "NaN", int(np.isnan(V).sum()),
              "-inf", int(np.isneginf(V).sum()), "+inf", int(np.isposinf(V).sum()), "positive", int((V[np.isfinite(V)] > 0).sum()))
    path = os.path.join(HERE, "score_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
