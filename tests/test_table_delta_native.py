"""The host side of a table's changes stream (gk_table_changes) on a CPU: tests/native/table_delta_test.cpp drives the pure logic
(csrc/table_delta.hpp) at its edges -- the key join (duplicates by occurrence, empty keys, disjoint sets, an empty side), the row map
(removed, added, reordered ids), cursors over both sides, pages at the side boundary, the host-known reviews and the page merge -- and
compares the CPU stand-in of dev_tchg_align / dev_tchg_index / dev_tchg_entries (tests/native/hostemu_tchg.cpp) with a bit-by-bit
reference over seeded random bitmaps and random permutations: one plan, three plan groups whose rows straddle a mask word, eleven groups,
five mask words, the gone side.  tests/test_table_changes.py checks the whole path, on the stand-in and on the device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "table_delta_test.cpp"), os.path.join(ROOT, "tests", "native", "hostemu_tchg.cpp")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_join_rows_cursor_pages_merge_and_stand_in(tmp_path, flags):
    """a stand-alone program with its own main, never loaded into Python: exit status 0, every case ok, no sanitizer report"""
    exe = tmp_path / "table_delta_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + flags + ["-I", CSRC, "-o", str(exe)] + SOURCES, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines() == ["ok join", "ok rows", "ok cursor", "ok pages", "ok merge", "ok stand_in"], out.stdout[-3000:] + out.stderr[-3000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
