"""Builds a stand-alone program of tests/c_abi against the host-only headers of wgsassign_amd/csrc with AddressSanitizer + UBSan and
runs it as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILE = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def run(tmp_path, source, *args):
    """The finished run of tests/c_abi/<source> with `args`, built in tmp_path; a program that does not compile fails the test here."""
    exe = str(tmp_path / os.path.splitext(source)[0])
    r = subprocess.run(COMPILE + ["-I", os.path.join(ROOT, "wgsassign_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c_abi", source)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
