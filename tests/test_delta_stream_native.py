"""The pieces of the resident-set changes stream that need neither the engine nor a device, on a CPU: tests/native/delta_stream_test.cpp
compares the CPU stand-in of dev_delta_keep / dev_delta_index / dev_delta_entries (tests/native/hostemu_delta.cpp) with a bit-by-bit
reference over seeded random now / base / shown bitmaps -- review counts 1, 63, 64, 65, 130 and 16 500, row counts 1, 3, 5, 64, 65 and 70,
no baseline, a word changed only in the baseline, only in the shown mask, only in bits beyond the last review, pages that begin at a
nonzero word -- and drives the host-side diff of the sparse (slot, row) pairs (csrc/delta_stream.hpp).  tests/test_resident_changes.py
checks the whole path, on the stand-in and on the device, against the oracle."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "delta_stream_test.cpp"), os.path.join(ROOT, "tests", "native", "hostemu_delta.cpp")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_stand_in_and_pair_diff(tmp_path, flags):
    """a stand-alone program with its own main, never loaded into Python: exit status 0, every case ok, no sanitizer report"""
    exe = tmp_path / "delta_stream_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + flags + ["-I", CSRC, "-o", str(exe)] + SOURCES, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines() == ["ok stand_in", "ok pairs"], out.stdout[-3000:] + out.stderr[-3000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
