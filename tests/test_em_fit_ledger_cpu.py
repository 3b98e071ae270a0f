"""wgs_em_fit's bookkeeping on the CPU: csrc/em_fit_ledger.h is host-only, so tests/c_abi/em_fit_ledger_check.cpp drives EmFitLedger
as wgs_em_fit does against a model of the device (every single-fit script up to five iterations under every fusion setting, 2000
batches of five fits), under AddressSanitizer + UBSan.  The program also prints what em_classify and em_chain_converged say, and
this test holds them against the Python protocol's decide_converged and chain_diff (wgsassign_amd/device.py)."""
import math
import os
import struct
import subprocess

import numpy as np

from conftest import ROOT


def _carries():
    """(carry, n) of tests/test_host_logic_cpu.py's chains -- the 50 000-site pair of test_cumsum_standin_is_the_serial_chain and the
    6 * 10^7 squares of test_guard_band_covers_float32_stagnation, whose float32 sum stalls below the exact one -- and edge values."""
    rng = np.random.Generator(np.random.PCG64(1))
    a = rng.random(50_000, dtype=np.float32)
    d = a - (a + rng.normal(0, 1e-4, 50_000).astype(np.float32)).astype(np.float32)
    out = [(np.cumsum(d * d, dtype=np.float32)[-1], 50_000)]
    m = 60_000_000
    rng = np.random.Generator(np.random.PCG64(11))
    sq = (rng.standard_normal(m, dtype=np.float32) * np.float32(1.07e-4)) ** 2
    with np.errstate(all="ignore"):
        out.append((np.cumsum(sq, dtype=np.float32)[-1], m))
    out += [(np.float32(v), n) for v in (0.0, 1e-5, 1.0, np.inf, np.nan) for n in (1, 1000, 16_777_217, 60_000_000)]
    return out


def test_ledger_against_a_model_of_the_device_and_the_python_protocol(tmp_path):
    from wgsassign_amd.device import chain_diff, decide_converged
    exe = str(tmp_path / "em_fit_ledger_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-I", os.path.join(ROOT, "wgsassign_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "c_abi", "em_fit_ledger_check.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    args, want_chain = [], []
    for carry, n in _carries():
        with np.errstate(all="ignore"):
            diff = chain_diff(carry, n)
        toles = [1e-4, 0.0, float("nan")]
        if math.isfinite(diff) and diff > 0:          # `<` at its edge
            toles += [diff, math.nextafter(diff, math.inf), math.nextafter(diff, 0.0)]
        for tole in toles:
            args += ["%08x" % struct.unpack("<I", np.float32(carry).tobytes())[0], str(n), float(tole).hex()]
            want_chain.append(1 if diff < tole else 0)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("ledger: ") and lines[-1].endswith("agree with the reference's loop"), lines[-1]
    single, batches = (int(w) for w in lines[-1].split() if w.isdigit())
    assert single > 10_000 and batches == 2000

    # em_classify == decide_converged, edge for edge: +1 converged, -1 goes on, 0 needs the exact chain
    states = {0: -1, 1: 1, 2: 0}                      # EM_ACTIVE, EM_CONVERGED, EM_UNDECIDED
    classify = [l.split()[1:] for l in lines if l.startswith("classify ")]
    assert len(classify) >= 5 * 3 * 3 * 5
    seen = set()
    for m, tole, guard, s, state in classify:
        want = decide_converged(float.fromhex(s), int(m), float.fromhex(tole), float.fromhex(guard))
        assert states[int(state)] == want, (m, tole, guard, s, state, want)
        seen.add(want)
    assert seen == {-1, 0, 1}

    # em_chain_converged == chain_diff(...) < tole
    chain = [int(l.split()[-1]) for l in lines if l.startswith("chain ")]
    assert chain == want_chain and 0 in chain and 1 in chain
