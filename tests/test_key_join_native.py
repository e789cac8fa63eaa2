"""The host side of the device key join (GK_CHANGES_DEVICE_JOIN, gk_table_join) on a CPU: tests/native/key_join_test.cpp drives the pure
logic (csrc/key_join.hpp) at its edges -- kjoin_pack's record boundaries at key lengths 0, 11, 12, 13, 27, 28, 29, the zero padding and
the refusal of offsets that do not fit (a faked size); kjoin_hash under hash_bits 64 / 3 / 0; kjoin_resolve against a full delta_join of
the same sides with duplicates 2:1, 1:2, 3:2, 2:3 and empty keys among the flagged -- and compares the CPU stand-in's dev_kjoin
(tests/native/hostemu_kjoin.cpp) with delta_join over seeded random key sets of 0, 1, 63, 64, 65 and 257 reviews on either side, unique
and heavily duplicated, under all three hash widths, flagged sets and stats included.  tests/test_table_join.py checks the whole path, on
the stand-in and on the device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", x) for x in ("key_join_test.cpp", "hostemu_kjoin.cpp", "hostemu_tchg.cpp")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_pack_hash_resolve_and_stand_in(tmp_path, flags):
    """a stand-alone program with its own main, never loaded into Python: exit status 0, every case ok, no sanitizer report"""
    exe = tmp_path / "key_join_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + flags + ["-I", CSRC, "-o", str(exe)] + SOURCES, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines() == ["ok pack", "ok hash", "ok resolve", "ok stand_in"], out.stdout[-3000:] + out.stderr[-3000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
