"""The host side of gk_table_verify / gk_resident_verify on a CPU: tests/native/verify_merge_test.cpp drives the merge of the plan groups'
and chunks' answers (csrc/verify_merge.hpp: row bases of three groups, review bases of two chunks, the sort, the truncation) and the CPU
stand-in of dev_verify_diff / dev_verify_flip (tests/native/hostemu_verify.cpp) against a bit-by-bit reference over seeded random bitmaps:
tail masks, reviews beyond the limits on either side, the caller's mask, a capacity smaller than the differences.
tests/test_kernel_verify.py runs the same entries through the engine, and the device kernel on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "verify_merge_test.cpp"), os.path.join(ROOT, "tests", "native", "hostemu_verify.cpp")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_merge_and_stand_in(tmp_path, flags):
    """a stand-alone program with its own main, never loaded into Python: exit status 0, every case ok, no sanitizer report"""
    exe = tmp_path / "verify_merge_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + flags + ["-I", CSRC, "-o", str(exe)] + SOURCES, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines() == ["ok stand_in", "ok merge"], out.stdout[-3000:] + out.stderr[-3000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
