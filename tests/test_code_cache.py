"""The cache of compiled plan kernels (csrc/code_cache.hpp) on a CPU: tests/native/code_cache_test.cpp drives code_cache_get with a
stub in place of the compiler.  Pinned here, because the caches already on users' disks depend on them: the file name
(gk_gfx950_rtc<version>_<fnv64>_<length>.co, FNV-1a with the PROJECT's offset basis), the 48-byte header ("GKCO\\x01\\0\\0\\0", the
source length as a host-order u64, the SHA-256 of the source) and the directory rule.  Checked besides: a wrong file under the right
name (another text's header, cut off, no ELF magic, a symbolic link) is replaced and never trusted, the LRU of 64, one compile for
eight threads asking for one text, the compile slots, and a compile that throws.

Not covered on any machine: a directory or file of ANOTHER owner (it takes a second user) and, because uid 0 passes every access()
check, the "not writable by us" branch -- both are two comparisons in cache_dir / read_whole, left to reading.

The digests expected here come from hashlib; the program's own SHA-256 is compared with them for lengths on both sides of the two
padding branches."""
import hashlib
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "native", "code_cache_test.cpp")

CASES = ["sha256_and_fnv", "cold_then_warm", "wrong_file_other_text", "wrong_file_truncated", "wrong_file_no_elf", "wrong_file_symlink",
         "directory_rule", "lru", "same_text_from_8_threads", "two_slots_16_threads", "stub_throws", "waiter_of_a_compile_that_throws"]
SHA_LENGTHS = [0, 3, 55, 56, 63, 64, 119, 120, 1000]
RTC = 7002   # the stub's "compiler version"


def fnv64(data, basis=1469598103934665603):
    h = basis
    for c in data:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _build_and_run(where, flags):
    where.mkdir()
    exe = where / "code_cache_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread"] + flags + ["-I", CSRC, "-o", str(exe), SOURCE], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith(("GK_", "XDG_"))}
    work = where / "work"
    work.mkdir()
    return subprocess.run([str(exe)], cwd=str(work), env=env, capture_output=True, text=True, timeout=300), work


def _assert_all_ok(out):
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and not [x for x in lines if x.startswith("FAIL")], out.stdout[-3000:] + out.stderr[-3000:]
    assert [x[3:] for x in lines if x.startswith("ok ")] == CASES, out.stdout[-3000:]
    return lines


def test_code_cache_with_a_stub_compiler(tmp_path):
    out, work = _build_and_run(tmp_path / "plain", [])
    lines = _assert_all_ok(out)
    # ---- the program's SHA-256 and FNV against hashlib and the pinned value
    sha = {int(x.split()[1]): x.split()[2] for x in lines if x.startswith("sha256 ")}
    assert sorted(sha) == SHA_LENGTHS
    for n in SHA_LENGTHS:
        text = bytes(ord("a") + i % 26 for i in range(n))
        assert sha[n] == hashlib.sha256(text).hexdigest(), n
    assert "fnv64 abc e16801510db89efd" in lines
    assert fnv64(b"abc") == 0xe16801510db89efd and fnv64(b"abc", 14695981039346656037) == 0xe71fa2190541574b   # the basis is the project's
    # ---- the file of the cold request: name, header and payload worked out here
    src = b"cold, then warm"
    name = "gk_gfx950_rtc%d_%016x_%d.co" % (RTC, fnv64(src), len(src))
    assert os.listdir(str(work / "cw")) == [name]
    data = (work / "cw" / name).read_bytes()
    assert data[:48] == b"GKCO\x01\0\0\0" + struct.pack("=Q", len(src)) + hashlib.sha256(src).digest()
    assert data[48:] == b"\x7fELF" + (b"%016x" % fnv64(src)) * 6
    # ---- a refused directory is said once, in one line
    refusals = [x for x in out.stderr.splitlines() if "is not a private directory" in x]
    for d in ("shared", "link", "plainfile"):
        path = os.path.join(os.path.realpath(str(work)), d)   # (the program names its directories by getcwd())
        assert len([x for x in refusals if "code-object cache %s " % path in x and x.endswith("disk cache off")]) == 1, out.stderr[-3000:]
    assert any("/shared " in x and "mode 770" in x for x in refusals)


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_code_cache_under_sanitizers(tmp_path, sanitizer):
    """the same stand-alone program (its own main, never loaded into Python), every case: exit status 0 and no report"""
    flags = ["-g", "-fsanitize=" + sanitizer] + (["-fno-sanitize-recover=all"] if sanitizer != "thread" else [])
    out, _ = _build_and_run(tmp_path / "san", flags)
    _assert_all_ok(out)
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
