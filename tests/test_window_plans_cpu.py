"""The window planners, the seven windowed_*_candidate predicates and with_windows_hint against tests/golden/window_plans.json, the
record taken of them on an enumerated grid (tests/golden/make_golden_window_plans.py) before they were given their shared helpers:
every entry is recomputed by the generator's own records() and must be equal.  No GPU."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PLANNERS = ("plan", "plan_fit", "plan_loo", "plan_loo_ds", "plan_ne", "plan_z", "plan_zref")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_window_plans", os.path.join(GOLDEN, "make_golden_window_plans.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_every_recorded_entry_is_reproduced():
    with open(os.path.join(GOLDEN, "window_plans.json")) as fh:
        text = fh.read()
    want = json.loads(text)
    gen = _generator()
    got = json.loads(json.dumps(gen.records()))         # (tuples as the lists JSON makes of them)
    assert sorted(got) == sorted(want)

    def spelled(rec, value):
        return ["MemoryError", rec["messages"][value[1]]] if isinstance(value, list) and value[0] == "MemoryError" else value

    keys = {}
    for k in gen.arithmetic():
        keys.setdefault(k.split("|", 1)[0], []).append(k)
    assert sorted(got["arithmetic"]) == sorted(want["arithmetic"]) == sorted(keys)
    for function, names in keys.items():
        a, b = want["arithmetic"][function], got["arithmetic"][function]
        assert len(a) == len(b) == len(names), function
        wrong = [(k, spelled(want, x), spelled(got, y)) for k, x, y in zip(names, a, b) if spelled(want, x) != spelled(got, y)]
        assert not wrong, "%s: %d of %d entries differ, the first: %r" % (function, len(wrong), len(names), wrong[0])
    for section in ("candidates", "hints"):
        wrong = [(k, want[section][k], got[section].get(k)) for k in want[section] if got[section].get(k) != want[section][k]]
        assert not wrong, "%s: %d of %d entries differ, the first: %r" % (section, len(wrong), len(want[section]), wrong[0])
    assert got == want
    assert gen.render(gen.records()) == text            # ... and the file, byte for byte


def test_the_record_covers_what_it_says():
    with open(os.path.join(GOLDEN, "window_plans.json")) as fh:
        want = json.load(fh)
    for planner in PLANNERS:
        values = want["arithmetic"][planner]
        errors = [v for v in values if isinstance(v, list) and v[0] == "MemoryError"]
        windows = [v for v in values if v is not None and v not in errors]
        assert errors and windows and any(v is None for v in values), planner       # every planner reaches all three outcomes
        assert all(0 <= v[1] < len(want["messages"]) for v in errors)
    assert len(set(want["messages"])) == len(want["messages"])
    assert len(want["candidates"]) == 256 and all(len(v) == 7 for v in want["candidates"].values())
    assert sum(v.count("1") for v in want["candidates"].values()) == 8                # (--ne_obs with and without --loo: two rows)
    assert len(want["hints"]) == 10
