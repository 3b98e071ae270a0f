#!/usr/bin/env python3
"""Generate tests/golden/window_plans.json: what the window planners (wgsassign_amd/windows.py), the seven windowed_*_candidate
predicates and with_windows_hint (wgsassign_amd/WGSassign.py) answer on an enumerated grid.  Pure arithmetic: no GPU, no file read.

The file is a record of the code as it stands, not of the reference (which has no windows): it was written before the planners and
the command line's selectors were given their shared helpers, and running this file again must reproduce it byte for byte.
tests/test_window_plans_cpu.py recomputes every entry through records() and compares for equality.  To keep the file small it
holds per function the values alone, in the order in which arithmetic() enumerates the grid (the test names a differing entry by
the key arithmetic() gives it), and every MemoryError text once, in "messages": an entry that raised is ["MemoryError", its index].
plan_zref, a third of the planners' entries otherwise, is recorded for two of the three individual counts and splits.

    arithmetic   m x n x K x free below; per planner its own settings (the variable unset or "20000", the split of the individuals
                 over the populations, the partition count, --loo beside --ne_obs, the individuals of a z-score run).  An entry is the
                 returned value or ["MemoryError", message]; beside them z_batch / zref_batch at two window sizes and every
                 *_site_bytes, *_state_bytes and fits_resident* function at the same points.
    candidates   all 128 combinations of the seven option flags x world in {1, 2}, parsed from real flags by WGSassign.parser: the
                 seven answers as a string of 0 / 1 in the order of CANDIDATES.
    hints        with_windows_hint on the slab-allocation error for each keyword alone, for none, and on an unrelated error.
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from wgsassign_amd import WGSassign, windows  # noqa: E402

MIB, GIB = 1 << 20, 1 << 30
SITES = (8192, 10 ** 7, 3 * 10 ** 9)
SHAPES = [(n, K) for n in (2, 180, 1000) for K in (1, 8) if K <= n]
FREE = (64 * MIB, 16 * GIB, 288 * GIB)
PARTITIONS = (1, 7)
WINDOWS = (8192, 1 << 20)
FLAGS = ("get_reference_af", "loo", "ne_obs", "get_pop_like", "get_assignment_z_score", "get_reference_z_score", "loo_downsampled_beagle")
CANDIDATES = ("windowed_candidate", "windowed_fit_candidate", "windowed_loo_candidate", "windowed_loo_ds_candidate",
              "windowed_ne_candidate", "windowed_z_candidate", "windowed_zref_candidate")
SLAB_ERROR = "wgsassign_amd HIP call failed: api.hip:1: hipMalloc of 123 bytes for population slab 0 failed: out of memory"


def splits(n, K):
    """The individuals of every population: unknown, an even split, one population holding n - K + 1."""
    return (("unknown", None), ("even", [n // K + (i < n % K) for i in range(K)]), ("one_large", [n - K + 1] + [1] * (K - 1)))


def individuals(n):
    return (1, min(n, 64), n)


def thinned(settings):
    """The first and the last of a dimension's settings, for plan_zref alone."""
    return (settings[0], settings[-1])


def environs(name):
    return (("unset", {}), ("20000", {name: "20000"}))


def outcome(f, *args, **kwargs):
    try:
        return f(*args, **kwargs)
    except MemoryError as e:
        return ["MemoryError", str(e)]


def key(*parts):
    return "|".join(str(p) for p in parts)


def arithmetic():
    out = {}
    for n, K in SHAPES:
        out[key("site_bytes", n, K)] = windows.site_bytes(n, K)
        for count in individuals(n):
            out[key("z_state_bytes", count)] = windows.z_state_bytes(count)
            out[key("zref_state_bytes", count)] = windows.zref_state_bytes(count)
            out[key("z_site_bytes", n, K, count)] = windows.z_site_bytes(n, K, count)
        for split, counts in splits(n, K):
            out[key("fit_site_bytes", n, K, split)] = windows.fit_site_bytes(n, K, counts)
            out[key("ne_site_bytes", n, K, split)] = windows.ne_site_bytes(n, K, counts)
            for P in PARTITIONS:
                out[key("loo_site_bytes", n, K, split, P)] = windows.loo_site_bytes(n, K, counts, P)
                out[key("loo_ds_site_bytes", n, K, split, P)] = windows.loo_ds_site_bytes(n, K, counts, P)
            for count in individuals(n):
                out[key("zref_site_bytes", n, K, count, split)] = windows.zref_site_bytes(n, K, count, counts)
        for free in FREE:
            for W in WINDOWS:
                for count in individuals(n):
                    out[key("z_batch", W, n, K, count, free)] = windows.z_batch(W, n, K, count, free)
                    for split, counts in splits(n, K):
                        out[key("zref_batch", W, n, K, count, free, split)] = windows.zref_batch(W, n, K, count, free, counts=counts)
            for m in SITES:
                at = (m, n, K, free)
                out[key("fits_resident", *at)] = windows.fits_resident(m, n, K, free)
                for env, environ in environs(windows.ENV):
                    out[key("plan", *at, env)] = outcome(windows.plan, m, n, K, free, environ)
                for split, counts in splits(n, K):
                    out[key("fits_resident_fit", *at, split)] = windows.fits_resident_fit(m, n, K, free, counts)
                    out[key("fits_resident_loo_ds", *at, split)] = windows.fits_resident_loo_ds(m, n, K, free, counts)
                    out[key("plan_fit", *at, split)] = outcome(windows.plan_fit, m, n, K, free, {}, counts)
                    for P in PARTITIONS:
                        out[key("plan_loo", *at, split, P)] = outcome(windows.plan_loo, m, n, K, free, {}, counts, P)
                        out[key("plan_loo_ds", *at, split, P)] = outcome(windows.plan_loo_ds, m, n, K, free, {}, counts, P)
                        for loo in (False, True):
                            out[key("plan_ne", *at, split, P, loo)] = outcome(windows.plan_ne, m, n, K, free, {}, counts, loo, P)
                for count in individuals(n):
                    out[key("fits_resident_z", *at, count)] = windows.fits_resident_z(m, n, K, count, free)
                    for env, environ in environs(windows.ENV_Z):
                        out[key("plan_z", *at, count, env)] = outcome(windows.plan_z, m, n, K, count, free, environ)
                    for split, counts in splits(n, K):
                        out[key("fits_resident_zref", *at, count, split)] = windows.fits_resident_zref(m, n, K, count, free, counts)
                        if count not in thinned(individuals(n)) or split not in ("unknown", "even"):
                            continue
                        for env, environ in environs(windows.ENV_ZREF):
                            out[key("plan_zref", *at, count, split, env)] = outcome(windows.plan_zref, m, n, K, count, free,
                                                                                    environ=environ, counts=counts)
    return out


def candidates():
    out = {}
    for given in itertools.product((0, 1), repeat=len(FLAGS)):
        argv = ["--beagle", "x.beagle.gz"]
        for flag, on in zip(FLAGS, given):
            if on:
                argv += ["--" + flag] + (["d.beagle.gz"] if flag == "loo_downsampled_beagle" else [])
        args = WGSassign.parser.parse_args(argv)
        for world in (1, 2):
            out[key("".join(map(str, given)), world)] = "".join(str(int(bool(getattr(WGSassign, c)(args, world)))) for c in CANDIDATES)
    return out


def hints():
    out = {}
    keywords = ("candidate", "z_candidate", "zref_candidate", "loo_ds_candidate")
    for error in (RuntimeError(SLAB_ERROR), RuntimeError("something else")):
        for keyword in (None,) + keywords:
            hinted = WGSassign.with_windows_hint(error, **({keyword: True} if keyword else {}))
            out[key(str(error), keyword)] = [type(hinted).__name__, str(hinted), hinted is error]
    return out


def records():
    """What the file holds: arithmetic() per function as the list of its values in grid order, the MemoryError texts once."""
    by_function, messages = {}, []
    for k, value in arithmetic().items():
        if isinstance(value, list) and value[0] == "MemoryError":
            if value[1] not in messages:
                messages.append(value[1])
            value = ["MemoryError", messages.index(value[1])]
        by_function.setdefault(k.split("|", 1)[0], []).append(value)
    return {"flags": list(FLAGS), "candidate_functions": list(CANDIDATES), "arithmetic": by_function, "messages": messages,
            "candidates": candidates(), "hints": hints()}


def render(rec):
    """The file's text: compact separators, one line per section and per function of the arithmetic."""
    def dumps(x):
        return json.dumps(x, separators=(",", ":"), sort_keys=True)
    lines = ['"%s":%s' % (name, dumps(rec[name])) for name in sorted(rec) if name != "arithmetic"]
    functions = ",\n".join('"%s":%s' % (name, dumps(values)) for name, values in sorted(rec["arithmetic"].items()))
    return "{" + ",\n".join(lines + ['"arithmetic":{\n' + functions + "\n}"]) + "}\n"


def main():
    path = os.path.join(HERE, "window_plans.json")
    rec = records()
    with open(path, "w") as fh:
        fh.write(render(rec))
    values = list(arithmetic().items())
    for planner in ("plan", "plan_fit", "plan_loo", "plan_loo_ds", "plan_ne", "plan_z", "plan_zref"):
        got = [v for k, v in values if k.startswith(planner + "|")]
        errors = sum(1 for v in got if isinstance(v, list) and v and v[0] == "MemoryError")
        print("%-12s %4d entries: %4d resident, %4d windows, %4d MemoryError" %
              (planner, len(got), sum(1 for v in got if v is None), len(got) - errors - sum(1 for v in got if v is None), errors))
    print("wrote", path, os.path.getsize(path), "bytes;", len(values), "arithmetic entries,", len(rec["candidates"]), "candidate rows,",
          len(rec["hints"]), "hints")


if __name__ == "__main__":
    main()
