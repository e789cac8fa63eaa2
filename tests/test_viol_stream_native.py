"""The host side of the resident-set violation stream on a CPU: tests/native/viol_stream_test.cpp drives the pure page / cursor / merge
/ shift logic (csrc/viol_stream.hpp) at its edges and compares the CPU stand-in of dev_viol_index / dev_viol_entries
(tests/native/hostemu_viol.cpp) with a bit-by-bit reference over seeded random bitmaps.  tests/test_resident_violations.py checks the
whole path, on the stand-in and on the device, against the oracle."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "viol_stream_test.cpp"), os.path.join(ROOT, "tests", "native", "hostemu_viol.cpp")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_page_logic_and_stand_in(tmp_path, flags):
    """a stand-alone program with its own main, never loaded into Python: exit status 0, every case ok, no sanitizer report"""
    exe = tmp_path / "viol_stream_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + flags + ["-I", CSRC, "-o", str(exe)] + SOURCES, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines() == ["ok pages", "ok cursor", "ok merge", "ok shift", "ok stand_in"], out.stdout[-3000:] + out.stderr[-3000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
