"""CPU-only: everything the streamed reader (csrc/reader*.cpp) shows through the C ABI and csrc/reader_text.h, held byte for
byte to a trace recorded from the reader before it was split into units (tests/golden/reader_trace.txt).

tests/c_abi/reader_trace.cpp is a stand-alone program that links the reader's sources; its inputs are the committed files of
tests/golden/reader/ (written by make_fixtures.py there).  The trace covers the index in one pass and in 1, 2 and 3 parts, rows
from plain and indexed opens at 1, 2 and 7 threads, both hand-overs at their smallest chunk sizes, integer tables, damaged
files and every refusal -- with no timings, pointers or absolute paths in it."""
import glob
import os
import shutil
import subprocess

from conftest import GOLDEN, ROOT


def test_reader_reproduces_the_recorded_trace(tmp_path):
    csrc = os.path.join(ROOT, "wgsassign_amd", "csrc")
    exe = str(tmp_path / "reader_trace")
    cmd = ["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe,
           os.path.join(ROOT, "tests", "c_abi", "reader_trace.cpp")] + sorted(glob.glob(os.path.join(csrc, "reader*.cpp"))) + ["-lz", "-lpthread", "-ldl"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    work = tmp_path / "files"
    work.mkdir()
    names = sorted(f for f in os.listdir(os.path.join(GOLDEN, "reader")) if f.endswith((".gz", ".txt")))
    assert len(names) == 14
    for f in names:
        shutil.copy(os.path.join(GOLDEN, "reader", f), str(work / f))
    r = subprocess.run([exe] + names, cwd=str(work), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = open(os.path.join(GOLDEN, "reader_trace.txt")).read()
    if r.stdout != want:
        got, exp = r.stdout.split("\n"), want.split("\n")
        first = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        section = next((ln for ln in reversed(got[:first + 1]) if ln.startswith("==")), "")
        raise AssertionError("trace differs at line %d (%s):\n  got      %s\n  recorded %s" % (
            first + 1, section, got[first] if first < len(got) else "<end>", exp[first] if first < len(exp) else "<end>"))
