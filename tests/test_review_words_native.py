"""csrc/review_words.hpp (which predicate classes a binding evaluates once, which global words they write) and the list filter, by the
stand-alone program tests/native/review_words_test.cpp: built plain and with AddressSanitizer + UndefinedBehaviorSanitizer, run both."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "review_words_test.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "asan-ubsan"])
def test_analysis_and_list_filter(tmp_path, flags):
    exe = tmp_path / "review_words_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-I", CSRC] + flags + ["-o", str(exe), SRC], check=True, timeout=300)
    env = {k: v for k, v in os.environ.items() if not k.startswith("GK_REVIEW_WORDS")}   # (the program checks the defaults of the switches)
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip() == "review words ok"
