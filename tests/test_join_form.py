"""The JOIN form of phase 2 (csrc/codegen.cpp conj_body): at sweep geometry (row groups of 128 reviews and more, two formula shares per
half) a value join whose body is a conjunction -- "some volume is present, not of kind k, and has the id this mount names" -- is ONE masked
compare per pair, ((w ^ (X << 8)) & (care | idmask << 8)) == want, and one test of X per outer element.  The existing small-table tests
run at 64-review groups and never reach it: these set the geometry themselves (GK_RPT=128 / 256 on the emulated plan-specialised
kernel, or `parts` = 2 handed to the generator)."""
import os
import subprocess
import sys

import pytest

import test_jit_source as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GK_JIT_")}
    env.update({k: str(v) for k, v in kw.items()})
    return env


def _util(what, rpt, **kw):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "join_form_util.py"), what], capture_output=True, text=True,
                         env=_env(GK_HOSTEMU_KERNEL="jit", GK_EMU_GRID=8, GK_RPT=rpt, **kw))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("rpt", [128, 256])
def test_tables_on_the_emulator_with_the_form_and_without(rpt):
    """(a) configs[2] and the 200-template corpus at both sweep geometries: the emulator compares every bitmap word with the per-review
    evaluation; (b) GK_JIT_JOIN=0 (the general form) gives the same violation / autoreject / match words"""
    on = _util("tables", rpt)
    off = _util("tables", rpt, GK_JIT_JOIN=0)
    assert on.count("\n") == 2 and on == off, (on, off)


@pytest.mark.parametrize("rpt", [128, 256])
def test_pattern_and_self_join_plans_on_the_emulator(rpt):
    """(a) the policy compiler's library patterns, root-scope comparisons, key string tests and self-joins (alias cursors, key
    relations: they keep the general form) against the oracle, evaluated on the emulated kernel at sweep geometry"""
    assert "patterns ok" in _util("patterns", rpt)


# ---- (c) known answers.  tests/native/join_form_gen.cpp: for each of three mounts (word, id X in a slot of its own), j = some volume
# (of 12; word = present | kind << 1 | id << 8 | parent ordinal << 24) with kind clear and the mount's id; violation = some present
# mount with j.  A case: (mounts, volumes, mount words, mount ids, volume words) -> (j per mount, violation)
def _vol(vid, kind=0, parent=0):
    return 1 | (kind << 1) | (vid << 8) | (parent << 24)


ABSENT = 0
CASES = [
    # an outer element whose value id is 0 ("no value"): equals nothing, not even a volume without an id
    ((3, 2, [1, 1, 1], [0, 0, 9], [_vol(0), _vol(9)] + [ABSENT] * 10), ([0, 0, 1], 1)),
    ((1, 1, [1, 0, 0], [0, 0, 0], [_vol(0)] + [ABSENT] * 11), ([0, 0, 0], 0)),
    # an inner element that is absent (a zero word inside the count, and the words beyond it), against ids 7 and 0
    ((2, 3, [1, 1, 0], [7, 0, 0], [ABSENT, ABSENT, _vol(8)] + [ABSENT] * 9), ([0, 0, 0], 0)),
    ((1, 0, [1, 0, 0], [7, 0, 0], [ABSENT] * 12), ([0, 0, 0], 0)),
    # ids that differ from the outer one in bit 0 only, in bit 15 only; the third mount's id is there
    ((3, 3, [1, 1, 1], [6, 0x0006, 0x8007], [_vol(7), _vol(0x8006), _vol(0x8007)] + [ABSENT] * 9), ([0, 0, 1], 1)),
    ((2, 2, [1, 1, 0], [6, 0x8006, 0], [_vol(7), _vol(0x0006 | 0x4000)] + [ABSENT] * 10), ([0, 0, 0], 0)),
    # bits above the id field (the parent ordinal) take no part; the kind bit does
    ((2, 2, [1, 1, 0], [9, 10, 0], [_vol(9, parent=5), _vol(10, kind=1, parent=255)] + [ABSENT] * 10), ([1, 0, 0], 1)),
    # twelve present volumes of which only the last matches; and the same with the kind bit set on it
    ((1, 12, [1, 0, 0], [40, 0, 0], [_vol(20 + i) for i in range(11)] + [_vol(40)]), ([1, 0, 0], 1)),
    ((1, 12, [1, 0, 0], [40, 0, 0], [_vol(20 + i) for i in range(11)] + [_vol(40, kind=1)]), ([0, 0, 0], 0)),
    # the join holds for an ABSENT mount's slot only: its derived bit is set (as in the general form), the violation is not
    ((3, 1, [1, 0, 1], [5, 6, 5], [_vol(6)] + [ABSENT] * 11), ([0, 1, 0], 0)),
    # the largest id
    ((1, 2, [1, 0, 0], [0xFFFE, 0, 0], [_vol(0x7FFE), _vol(0xFFFE)] + [ABSENT] * 10), ([1, 0, 0], 1)),
]


def _plan_text(tmp_path, parts, **kw):
    gen = tmp_path / "join_form_gen"
    if not gen.exists():
        subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-I", CSRC, "-o", str(gen), os.path.join(NATIVE, "join_form_gen.cpp"),
                        os.path.join(CSRC, "codegen.cpp")], check=True)
    return subprocess.run([str(gen), str(parts)], capture_output=True, text=True, check=True, env=_env(**kw)).stdout


def _run_cases(tmp_path, name, text):
    d = tmp_path / name
    d.mkdir()
    (d / "join_form_plan.inc").write_text(text)
    exe = d / "run"
    subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-I", str(d), "-I", CSRC, "-o", str(exe), os.path.join(NATIVE, "join_form_run.cpp")], check=True)
    feed = "".join(" ".join(str(x) for x in [c[0], c[1]] + c[2] + c[3] + c[4]) + "\n" for c, _ in CASES)
    out = subprocess.run([str(exe)], input=feed, capture_output=True, text=True, check=True).stdout.split("\n")
    return [[int(x) for x in line.split()] for line in out if line.strip()]


def _part_text(text):
    return text[text.index("void jit_formula_part("):]


def test_join_known_answers(tmp_path):
    """(c) the join form, the general form (GK_JIT_JOIN=0) and the monolithic function answer every hand-built table as written out above"""
    for c, _ in CASES:
        assert len(c[2]) == 3 and len(c[3]) == 3 and len(c[4]) == 12
    form = _plan_text(tmp_path, 2)
    general = _plan_text(tmp_path, 2, GK_JIT_JOIN=0)
    assert "xs_" in _part_text(form) and "vid_eq(" not in _part_text(form)
    assert "xs_" not in general and "vid_eq(" in _part_text(general)
    for name, text in (("form", form), ("general", general)):
        got = _run_cases(tmp_path, name, text)
        assert len(got) == len(CASES)
        for (c, (j, viol)), g in zip(CASES, got):
            assert g[:4] == j + [viol], "%s, staged parts: case %r gives %r" % (name, c, g)
            assert g[4:] == j + [viol], "%s, monolithic: case %r gives %r" % (name, c, g)


def test_admission_geometry_keeps_its_text(tmp_path):
    """four formula shares per half (64-review groups): the generator's output does not depend on the switch"""
    assert _plan_text(tmp_path, 4) == _plan_text(tmp_path, 4, GK_JIT_JOIN=0)
    assert "xs_" not in _plan_text(tmp_path, 4)


def test_bench_plan_text_holds_the_join_form_and_compiles(monkeypatch, tmp_path):
    """(d) configs[2] at 256-review groups: the unrolled volumeMounts x volumes nests of the formula shares are masked compares -- no
    vid_eq( is left in jit_formula_part -- and the text compiles for gfx950"""
    monkeypatch.delenv("GK_JIT_JOIN", raising=False)
    texts = J._dump_sources(monkeypatch, tmp_path, J._bench_plan(1200), env=[("GK_RPT", 256), ("GK_JIT_WAVES", 6)])
    rtc = J._hiprtc()
    for name, text in texts:
        part = _part_text(text)
        part = part[:part.index("}  // namespace gk")]
        assert part.count("^ xs_) & ") >= 12 and "vid_eq(" not in part, name
        if rtc is not None:
            ok, log, code = J.compile_gfx950(rtc, text)
            assert ok, log[-3000:]
            assert 0 <= J._scratch_bytes(code) <= 96
