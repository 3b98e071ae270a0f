"""What the windowed streams refuse, and the handle base of the device objects, without a GPU: every message of
csrc/stream_checks.h against the record taken before the checks were folded into one header (tests/golden/stream_refusals.tsv), the
shared refusals driven for the score stream under the sanitizers, and the lifecycle of device.Handle on a stub that loads no
library."""
import gc
import os
import weakref

import sanitized
from wgsassign_amd import device


def test_messages_equal_the_record(tmp_path):
    """tests/c_abi/stream_refusals_dump.cpp prints rc and message of every case of its grid: byte for byte the record."""
    r = sanitized.run(tmp_path, "stream_refusals_dump.cpp")
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    with open(os.path.join(sanitized.ROOT, "tests", "golden", "stream_refusals.tsv"), "rb") as fh:
        want = fh.read()
    got = r.stdout.encode()
    assert want.startswith(b"# ") and len(want.splitlines()) > 500
    if got != want:
        for k, (a, b) in enumerate(zip(got.splitlines(), want.splitlines()), 1):
            assert a == b, "line %d" % k
    assert got == want


def test_score_stream_checks_under_the_sanitizers(tmp_path):
    """The window rule, the shape rule and `only X of Y sites were pushed` as wgs_score_stream_push and wgs_score_stream_finish call
    them: the `score` part of tests/c_abi/stream_checks_check.cpp, every window of files of up to 2^33 + 5 sites."""
    r = sanitized.run(tmp_path, "stream_checks_check.cpp", "score")
    assert r.returncode == 0 and r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 6_000_000, (r.stdout[-2000:], r.stderr[-3000:])


class Stub(device.Handle):
    """A handle whose destroy is a Python counter: no library is loaded."""

    log = []

    def __init__(self, name, *parents, children=False, fails=False):
        self.name, self.fails = name, fails
        self._own(name, *parents, children=children)

    def _release(self, h):
        Stub.log.append(h)
        if self.fails:
            raise RuntimeError("destroy failed")


class QuietStub(Stub):
    _at_exit = False


def test_handle_base_lifecycle(monkeypatch):
    monkeypatch.setattr(device, "_live", weakref.WeakSet())        # (a set of this test's own: device objects of other tests stay out)
    Stub.log.clear()
    parent, other = Stub("parent", children=True), Stub("other", children=True)
    a, b = Stub("a", parent), Stub("b", parent, other)
    quiet = QuietStub("quiet", parent)
    assert len(device._live) == 4 and quiet not in device._live       # a class that does not ask for it stays out
    assert parent.handle == "parent" and quiet in parent._children
    # children are closed before their parent, each once, also a child of two parents
    parent.close()
    assert Stub.log[-1] == "parent" and sorted(Stub.log[:-1]) == ["a", "b", "quiet"]
    assert a.handle is None and b.handle is None and parent.handle is None
    # a second close destroys nothing, nor does the other parent's close destroy the shared child again
    parent.close()
    a.close()
    other.close()
    assert Stub.log[4:] == ["other"] and len(Stub.log) == 5
    # __del__ survives a destroy that raises; close() itself lets the error through and keeps the handle
    bad = Stub("bad", fails=True)
    try:
        bad.close()
    except RuntimeError:
        pass
    else:
        raise AssertionError("close() swallowed the error")
    assert bad.handle == "bad"
    n = len(Stub.log)
    del bad
    gc.collect()
    assert len(Stub.log) == n + 1 and Stub.log[-1] == "bad"
    del parent, other, a, b, quiet
    gc.collect()
    assert len(device._live) == 0


def test_close_all_needs_no_order(monkeypatch):
    """device._close_all closes what is in _live in whatever order: a parent closes its children first, a closed child is skipped."""
    monkeypatch.setattr(device, "_live", weakref.WeakSet())        # (nothing but this test's objects is closed)
    Stub.log.clear()
    parent = Stub("parent", children=True)
    kids = [Stub("kid%d" % k, parent) for k in range(3)]
    device._close_all()
    assert Stub.log.count("parent") == 1 and all(Stub.log.count(k.name) == 1 for k in kids)
    assert all(Stub.log.index(k.name) < Stub.log.index("parent") for k in kids)
