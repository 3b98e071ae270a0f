#!/usr/bin/env python3
"""Generate tests/golden/em_cases.npz from the REAL reference on the enumerated EM inputs of tests/em_cases.py (em_cases.GOLDEN).

Run as make_golden_fisher_cases.py is run: build the reference in a scratch copy (python3 setup.py build_ext --inplace) and run this
file with that copy on PYTHONPATH, from a working directory other than this repository's root (whose own WGSassign package would
take the reference's place).  Per variant (`finite`, `hostile`), on the populations em_cases.GOLDEN_SIZES -- fewer than the GPU test's
em_cases.SIZES, to keep the file small -- emMAF_cy.emMAF_update after one and after two updates from the enumerated f_old, of every
population and of the five leave-one-out re-fits of the population of em_cases.GOLDEN_LOO; for `finite` also emMAF.emMAF from 0.25
(200 iterations, 1e-4) with the iteration it prints.  And one update of em_cases.negative_zero_sums (`zeros`).

Everything written is data: the generator's arguments, the digest of the inputs and what the reference's functions returned.
"""
import contextlib
import io
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import em_cases  # noqa: E402
from WGSassign import emMAF, emMAF_cy  # noqa: E402

assert os.path.dirname(os.path.abspath(emMAF.__file__)) != os.path.join(os.path.dirname(os.path.dirname(HERE)), "WGSassign"), \
    "this is the repository's own WGSassign package, not the reference"


def main():
    arrays = {}
    for name, gen in em_cases.GOLDEN.items():
        grid = em_cases.em_grid(**gen)
        L, sizes = grid["L"], gen["sizes"]
        with np.errstate(all="ignore"):
            ups = np.stack([em_cases.updates(emMAF_cy.emMAF_update, em_cases.columns(L, grid["members"][k]), grid["f_old"][k], 2)
                            for k in range(len(sizes))], axis=1)
            k = sizes.index(em_cases.GOLDEN_LOO)
            _, skips, cols = em_cases.loo_fits(grid, k, 5)
            mem = grid["members"][k]
            loo = np.stack([em_cases.updates(emMAF_cy.emMAF_update, em_cases.columns(L, mem[mem != i]), grid["f_old"][k], 2) for i in skips], axis=1)
        arrays[name + "_gen"] = np.array(repr(gen))
        arrays[name + "_digest"] = np.array(em_cases.digest(grid))
        arrays[name + "_updates"] = ups
        arrays[name + "_loo_cols"] = np.array(cols, dtype=np.int32)
        arrays[name + "_loo_updates"] = loo
        assert ups.dtype == loo.dtype == np.float32
        print(name, "populations", sizes, "m", L.shape[0], "NaN", int(np.isnan(ups[0]).sum()), "inf", int(np.isinf(ups[0]).sum()), "of", ups[0].size,
              "negative zeros", int(((ups[0] == 0) & np.signbit(ups[0])).sum()))
        if name == "finite":
            fits, iters = [], []
            for k in range(len(sizes)):
                out = io.StringIO()
                with contextlib.redirect_stdout(out):
                    fits.append(emMAF.emMAF(em_cases.columns(L, grid["members"][k]), 200, 1e-4, 1))
                found = re.search(r"converged at iteration: (\d+)", out.getvalue())
                iters.append(int(found.group(1)) if found else 0)
            arrays["finite_fit"] = np.stack(fits)
            arrays["finite_fit_iters"] = np.array(iters, dtype=np.int32)
            print("finite: iterations", iters)
    case = em_cases.negative_zero_sums()
    zeros = np.stack([em_cases.updates(emMAF_cy.emMAF_update, em_cases.columns(case["L"], case["members"][k]), case["f_old"][k], 1)
                      for k in range(len(case["sizes"]))], axis=1)
    arrays["zeros_digest"] = np.array(em_cases.digest(case))
    arrays["zeros_updates"] = zeros
    print("zeros: populations", case["sizes"], "negative zeros", int(((zeros == 0) & np.signbit(zeros)).sum()), "of", zeros.size)
    path = os.path.join(HERE, "em_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
