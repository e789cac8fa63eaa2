"""The resident-set audit where equal object keys decide, on a CPU: tests/native/audit_merge_test.cpp drives the host merge of the chunks'
candidates (csrc/audit_merge.hpp) and the CPU stand-in of dev_audit_select (tests/native/hostemu_audit.cpp) with key ranks that tie.  The
resident set itself cannot produce such keys -- a live object's key is its inventory path -- so tests/test_resident_audit.py never takes
the tie and overflow branches; the device kernels' copies of those branches are left to reading (they restate gk_topk_rows' rule)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "audit_merge_test.cpp"), os.path.join(ROOT, "tests", "native", "hostemu_audit.cpp")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_merge_and_stand_in(tmp_path, flags):
    """a stand-alone program with its own main, never loaded into Python: exit status 0, every case ok, no sanitizer report"""
    exe = tmp_path / "audit_merge_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + flags + ["-I", CSRC, "-o", str(exe)] + SOURCES, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines() == ["ok merge", "ok select_stand_in"], out.stdout[-3000:] + out.stderr[-3000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
