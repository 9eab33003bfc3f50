"""The block driver's call trace (host only, no GPU).  csrc/gkg_block.hip computes nothing itself: what it does is the list of
library entry points it calls and their arguments.  tests/block_trace/block_trace.cpp compiles the driver with every callee
replaced by a recorder and walks a cross product of its branches (block, BatchNorm mode, prepared queries, graph form, outputs,
backward flags, the two support queries, split-K workspace, wanted parameter gradients); this test compares, per case, the number
of calls and a SHA-256 of the case's text with tests/block_trace/expected.txt — so a change to the driver's structure that is meant
to keep its launches leaves that file byte-identical.

    python tests/test_block_driver_call_trace_host.py <csrc directory>

prints the table for the driver in that directory (e.g. another checkout's gkgnet_amd/csrc): that is how expected.txt is made."""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "tests", "block_trace")
EXPECTED = os.path.join(HERE, "expected.txt")


def _hipcc():
    from gkgnet_amd import _build
    cc = _build._hipcc()
    return cc if (os.path.exists(cc) or shutil.which(cc)) else None


def trace(csrc: str, workdir: str) -> dict:
    """Build the recorder against the driver in ``csrc`` and run it -> {case name: the case's text (return code, calls, wq[])}."""
    exe = os.path.join(workdir, "block_trace")
    subprocess.check_call([_hipcc(), "--cuda-host-only", "-x", "hip", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "block_trace.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    cases = {}
    for chunk in out.split("== case ")[1:]:
        name, _, body = chunk.partition("\n")
        assert name not in cases, name
        cases[name] = body
    return cases


def table(cases: dict) -> str:
    """One line per case: name | number of calls | SHA-256 of its text."""
    lines = []
    for name, body in cases.items():
        n = sum(1 for ln in body.splitlines() if ln.startswith("gkg_") and not ln.startswith("gkg_fail "))
        lines.append("%s | %d | %s\n" % (name, n, hashlib.sha256(body.encode()).hexdigest()))
    return "".join(lines)


def test_block_driver_call_trace_matches_the_recorded_one():
    import pytest
    if _hipcc() is None:
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        cases = trace(os.path.join(ROOT, "gkgnet_amd", "csrc"), tmp)
    got = table(cases).splitlines()
    with open(EXPECTED) as fh:
        want = fh.read().splitlines()
    bad = [g.split(" | ")[0] for g, w in zip(got, want) if g != w]
    for name in bad[:3]:
        print("== case %s (actual trace)\n%s" % (name, cases[name]))
    assert not bad, "%d of %d cases differ from tests/block_trace/expected.txt, first: %s" % (len(bad), len(want), bad[0])
    assert len(got) == len(want), (len(got), len(want))
    # every case ran to its end, and the cross product is the size the cases' names say
    assert all(body.startswith("rc 0\n") or "\nrc 0\n" in body for body in cases.values())
    assert len(want) == 2 * (48 + 16) + (64 + 32) + 3 * (64 + 32)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        sys.stdout.write(table(trace(os.path.abspath(sys.argv[1]), tmp)))
