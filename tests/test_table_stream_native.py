"""The host side of a table's violation stream (gk_table_violations) on a CPU: tests/native/table_stream_test.cpp drives the pure cursor /
index / page-merge logic (csrc/table_stream.hpp) at its edges and compares the CPU stand-in of dev_tviol_index / dev_tviol_entries
(tests/native/hostemu_tviol.cpp) with a bit-by-bit reference over seeded random bitmaps -- one plan, three plan groups whose rows straddle
a mask word, eleven groups.  tests/test_table_violations.py checks the whole path, on the stand-in and on the device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "table_stream_test.cpp"), os.path.join(ROOT, "tests", "native", "hostemu_tviol.cpp")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_cursor_index_merge_and_stand_in(tmp_path, flags):
    """a stand-alone program with its own main, never loaded into Python: exit status 0, every case ok, no sanitizer report"""
    exe = tmp_path / "table_stream_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + flags + ["-I", CSRC, "-o", str(exe)] + SOURCES, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines() == ["ok cursor", "ok pages", "ok merge", "ok stand_in"], out.stdout[-3000:] + out.stderr[-3000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
