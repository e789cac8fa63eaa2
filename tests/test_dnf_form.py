"""The DNF form of phase 2 and the provenance of formula values (csrc/codegen.cpp dnf_body / dnf_run / cmpv): at sweep geometry (row
groups of 128 reviews and more, two formula shares per half) a loop body that is a short disjunction of conjunctions of its element's
word 0, and a top-level run over the bits of ONE global word or of the flags, are masked compares (w & care) == want ORed together; a
value built of compare results only is tested without the opaque copy of GK_BIT (GK_RESC, `b != 0u`).  GK_JIT_DNF=0 restores the text
of before.  The existing small-table tests run at 64-review groups and never reach any of this: these set the geometry themselves."""
import os
import random
import re
import subprocess
import sys

import pytest

import test_jit_source as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gatekeeper_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")

# the text of the commit before this form (configs[2], 1 024 reviews, test_self_join_plan_text's procedure) at both sweep geometries:
# what GK_JIT_DNF=0 must reproduce byte for byte.  The hashes cover the whole text handed to hiprtc (plan.hpp, vm_core.hpp,
# kernel_body.inc and the generator's sweep-geometry output): a later change to any of those re-pins them, on a tree where
# GK_JIT_DNF=0 and the default give the texts that change intends, exactly as test_self_join_plan_text's are re-pinned.
PARENT_SHA256 = {
    128: "a3c6dbc06359d9a2a0fd3e9b98f39c25d7a9590ac750c8da6f38987efe1c00ab",
    256: "d4167d347eb896ff01c7a6fc88c9c09d68d5e880de6bbe78fcaf16f74f81e800",
}


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GK_JIT_")}
    env.update({k: str(v) for k, v in kw.items()})
    return env


def _script(name, args, rpt, **kw):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", name)] + list(args), capture_output=True, text=True,
                         env=_env(GK_HOSTEMU_KERNEL="jit", GK_EMU_GRID=8, GK_RPT=rpt, **kw))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("rpt", [128, 256])
def test_switch_restores_the_text_of_before(rpt):
    got = _script("dnf_form_util.py", ["sha", "2"], rpt, GK_JIT_DNF=0)
    assert got.split()[-1] == PARENT_SHA256[rpt]
    assert _script("dnf_form_util.py", ["sha", "2"], rpt).split()[-1] != PARENT_SHA256[rpt], "the form selects nothing on configs[2]"


@pytest.mark.parametrize("rpt", [128, 256])
def test_tables_on_the_emulator_with_the_form_and_without(rpt):
    """configs[2] (1 500 objects) and the 200-template corpus (512) at both sweep geometries, GK_JIT_DNF on and off:
    (a) the same violation / autoreject / match words (the emulator also compares every bitmap word of the emulated kernel with the
        product's own per-review bytecode interpreter and raises on a difference);
    (b) against the ORACLE (oracle/client.py, parity_util.assert_parity): the rendered results of every object and the raw violation
        and autoreject bitmaps equal the pairs the oracle's results imply -- with the emulated kernel checked against the interpreter
        in the same run, so the kernel's words are the oracle's pairs"""
    on = _script("join_form_util.py", ["tables"], rpt)
    off = _script("join_form_util.py", ["tables"], rpt, GK_JIT_DNF=0)
    assert on.count("\n") == 2 and on == off, (on, off)
    for policy, n in (("configs2", 1500), ("corpus", 512)):
        for kw in ({}, {"GK_JIT_DNF": 0}):
            assert "oracle %s" % policy in _script("dnf_form_util.py", ["oracle", "hostemu", policy, str(n)], rpt, **kw)


# ---------------------------------------------------------------------------------------------------------------- on the device
# The emulator and g++ cannot see what the DEVICE compiler does with a test that lost its opaque copy (GK_BIT is `(b) & 1u` there), and
# the other GPU tests run at 64-review groups, where the form is never taken: these run the hiprtc build at sweep geometry.
def _gpu_script(args, rpt, **kw):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dnf_form_util.py")] + list(args), capture_output=True, text=True,
                         env=_env(GK_RPT=rpt, **kw))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("rpt", [128, 256])
def test_device_tables_with_the_form_and_without_and_against_the_oracle(rpt):
    """the plan-specialised kernel on the MI355X at sweep geometry: configs[2] (1 500 objects) and the corpus (512) give the same
    violation / autoreject / match words with the form and with GK_JIT_DNF=0, and both policy sets agree with the oracle -- rendered
    results and raw bitmaps -- with the form on"""
    on = _gpu_script(["words", "gpu"], rpt)
    off = _gpu_script(["words", "gpu"], rpt, GK_JIT_DNF=0)
    assert on.count("\n") == 2 and on == off, (on, off)
    for policy, n in (("configs2", 1500), ("corpus", 512)):
        assert "oracle %s" % policy in _gpu_script(["oracle", "gpu", policy, str(n)], rpt)


@pytest.mark.gpu
@pytest.mark.parametrize("first", [12200, 12206, 12212, 12218])
def test_device_fuzz_at_sweep_geometry(first):
    """random templates, ten to a plan, through hiprtc at 256-review groups with the form on, each compared with the oracle: the guard
    for tests of formula values without the opaque copy (seeds no record has used; the campaign is in profiles/dnf_form.md)"""
    out = _gpu_script(["fuzz", "gpu", str(first), str(first + 5)], 256).split()
    assert out[-3] == "fuzz" and int(out[-2]) >= 200 and int(out[-1]) >= 200, out


# ---------------------------------------------------------------------------------------------------------------- formulas by hand
# tests/native/dnf_form_gen.cpp: accumulator words 0, 1 globals | 2, 3 counts | 4..6 mounts (scope 0) | 7..9 their value slots |
# 10..21 volumes (scope 1, the id packed at bit 8)
F_LDG, F_LDF, F_LDE, F_AND, F_OR, F_NOT, F_ANDN, F_CONST, F_MOV, F_LOOP, F_ENDLOOP, F_VEQ, F_RES, F_END, F_STE, F_STG = range(1, 17)
CAP = {0: 3, 1: 12}
WORD = {0: 4, 1: 10}


def fi(op, a=0, b=0, c=0):
    return op | (a << 8) | (b << 16) | (c << 24)


def interpret(code, flags, words):
    """the formula code bit by bit, as plan.hpp states it -> (violation word, accumulator words behind it)"""
    w = list(words)
    reg = [0] * 64
    viol = 0
    cur = {}

    def elem_id(scope, slot):
        return w[7 + cur[scope]] if scope == 0 else (w[WORD[1] + cur[1]] >> 8) & 0xFFFF

    def run(pc, end):
        nonlocal viol
        while pc < end:
            ins = code[pc]
            pc += 1
            op, a, b, c = ins & 0xFF, (ins >> 8) & 0xFF, (ins >> 16) & 0xFF, ins >> 24
            if op == F_LDG:
                bit = b | (c << 8)
                reg[a] = (w[bit >> 5] >> (bit & 31)) & 1
            elif op == F_LDF:
                reg[a] = (flags >> b) & 1
            elif op == F_LDE:
                reg[a] = (w[WORD[b] + cur[b]] >> c) & 1
            elif op == F_AND:
                reg[a] = reg[b] & reg[c]
            elif op == F_OR:
                reg[a] = reg[b] | reg[c]
            elif op == F_NOT:
                reg[a] = reg[b] ^ 1
            elif op == F_ANDN:
                reg[a] = reg[b] & (reg[c] ^ 1)
            elif op == F_CONST:
                reg[a] = b & 1
            elif op == F_MOV:
                reg[a] = reg[b]
            elif op == F_VEQ:
                x = code[pc]
                pc += 1
                ia, ib = elem_id(x & 0xFF, (x >> 8) & 0xFF), elem_id((x >> 16) & 0xFF, x >> 24)
                reg[a] = int(ia == ib and ia != 0)
            elif op == F_LOOP:
                depth, q = 0, pc
                while True:
                    qop = code[q] & 0xFF
                    if qop == F_VEQ:
                        q += 2
                        continue
                    if qop == F_LOOP:
                        depth += 1
                    if qop == F_ENDLOOP:
                        if depth == 0:
                            break
                        depth -= 1
                    q += 1
                reg[c] = 0
                ea, eb = (code[q] >> 8) & 0xFF, (code[q] >> 16) & 0xFF
                for e in range(CAP[a]):
                    cur[a] = e
                    run(pc, q)
                    reg[ea] |= reg[eb] & w[WORD[a] + e] & 1
                pc = q + 1
            elif op == F_RES:
                assert b == 0
                viol |= reg[a] << c
            elif op == F_STE:
                w[WORD[b] + cur[b]] |= reg[a] << c
            elif op == F_STG:
                bit = b | (c << 8)
                w[bit >> 5] |= reg[a] << (bit & 31)
            elif op == F_END:
                return
            else:
                raise AssertionError(op)

    run(0, len(code))
    return viol, w


def _gen_exe(tmp_path):
    gen = tmp_path / "dnf_form_gen"
    if not gen.exists():
        subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-I", CSRC, "-o", str(gen), os.path.join(NATIVE, "dnf_form_gen.cpp"),
                        os.path.join(CSRC, "codegen.cpp")], check=True)
    return gen


def _plan_text(tmp_path, parts, n_viol, blocks, **kw):
    code, segs = [], []
    for blk in blocks:
        code += blk
        segs.append(len(code))
    code.append(fi(F_END))
    feed = "%d %d %s\n%d %s\n" % (n_viol, len(code), " ".join(map(str, code)), len(segs), " ".join(map(str, segs)))
    text = subprocess.run([str(_gen_exe(tmp_path)), str(parts)], input=feed, capture_output=True, text=True, check=True, env=_env(**kw)).stdout
    return code, text


def _run_tables(tmp_path, name, text, tables):
    d = tmp_path / name
    d.mkdir()
    (d / "dnf_form_plan.inc").write_text(text)
    exe = d / "run"
    subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-I", str(d), "-I", CSRC, "-o", str(exe), os.path.join(NATIVE, "dnf_form_run.cpp")], check=True)
    feed = "".join("%d %s\n" % (f, " ".join(map(str, w))) for f, w in tables)
    out = subprocess.run([str(exe)], input=feed, capture_output=True, text=True, check=True).stdout.split("\n")
    rows = []
    for line in out:
        if line.strip():
            t = line.split()
            rows.append(((int(t[0], 16), [int(x) for x in t[1:11]]), (int(t[11], 16), [int(x) for x in t[12:22]])))
    assert len(rows) == len(tables)
    return rows


def _part_text(text):
    return text[text.index("void jit_formula_part("):]


def _table(flags=0, g0=0, g1=0, mounts=(), ids=(), volumes=()):
    mounts, ids, volumes = list(mounts), list(ids), list(volumes)
    w = [g0, g1, len(mounts), len(volumes)] + mounts + [0] * (3 - len(mounts)) + ids + [0] * (3 - len(ids)) + volumes + [0] * (12 - len(volumes))
    assert len(w) == 22
    return flags, w


def _vol(vid, bits=0):
    return 1 | bits | (vid << 8)


# the known-answer plan.  M(m) = bit1(m) & !(bit2(m) & !bit3(m)), a disjunctive body with a negated literal
#   violation 0 = g0.5 & !g0.6 & [some present mount with M]            a run that mixes a loop result into a DNF
#   g1.3 |= some present mount with (bit1 & !bit1) | (bit2 & bit4)      a contradictory term
#   violation 1 = (g0.5 & g0.6) | (!g0.7 & g0.8)                        a one-word result formula over a g word
#   violation 2 = (!flag0 & !flag1) | flag17                            ... and over the flags
#   mount bit 5 |= J(m) = some present volume v with (bit1(v) | bit2(v)) & id(v) == id(m);  violation 3 = some present mount with J
KA_BLOCKS = [
    [fi(F_LOOP, 0, 0, 1), fi(F_LDE, 2, 0, 1), fi(F_LDE, 3, 0, 2), fi(F_LDE, 4, 0, 3), fi(F_NOT, 4, 4), fi(F_AND, 3, 3, 4), fi(F_NOT, 3, 3),
     fi(F_AND, 2, 2, 3), fi(F_ENDLOOP, 1, 2),
     fi(F_LDG, 8, 5, 0), fi(F_LDG, 9, 6, 0), fi(F_NOT, 9, 9), fi(F_AND, 8, 8, 9), fi(F_AND, 8, 8, 1), fi(F_RES, 8, 0, 0)],
    [fi(F_LOOP, 0, 0, 1), fi(F_LDE, 2, 0, 1), fi(F_NOT, 3, 2), fi(F_AND, 2, 2, 3), fi(F_LDE, 3, 0, 2), fi(F_LDE, 4, 0, 4), fi(F_AND, 3, 3, 4),
     fi(F_OR, 2, 2, 3), fi(F_ENDLOOP, 1, 2), fi(F_STG, 1, 32 + 3, 0)],
    [fi(F_LDG, 8, 5, 0), fi(F_LDG, 9, 6, 0), fi(F_AND, 8, 8, 9), fi(F_LDG, 9, 7, 0), fi(F_LDG, 10, 8, 0), fi(F_ANDN, 9, 10, 9), fi(F_OR, 8, 8, 9),
     fi(F_RES, 8, 0, 1)],
    [fi(F_LDF, 8, 0), fi(F_NOT, 8, 8), fi(F_LDF, 9, 1), fi(F_ANDN, 8, 8, 9), fi(F_LDF, 9, 17), fi(F_OR, 8, 8, 9), fi(F_RES, 8, 0, 2)],
    [fi(F_LOOP, 0, 0, 1), fi(F_LOOP, 1, 0, 2), fi(F_LDE, 3, 1, 1), fi(F_LDE, 4, 1, 2), fi(F_OR, 3, 3, 4), fi(F_VEQ, 5), 1 | (0 << 8) | (0 << 16) | (0 << 24),
     fi(F_AND, 3, 3, 5), fi(F_ENDLOOP, 2, 3), fi(F_STE, 2, 0, 5), fi(F_ENDLOOP, 1, 2), fi(F_RES, 1, 0, 3)],
]
P, B1, B2, B3, B4, J5 = 1, 2, 4, 8, 16, 32   # mount word: present, bits 1..4, the derived bit 5
G5, G6, G7, G8, D3 = 1 << 5, 1 << 6, 1 << 7, 1 << 8, 1 << 3
# (table) -> (violation bits 0..3, g1 behind the formulas, mount words behind them)
KA_CASES = [
    # nothing at all: violation 2 alone (no flag 0, no flag 1)
    (_table(), (0b0100, 0, [0, 0, 0])),
    # M through "not bit2"; g0.5 without g0.6: violation 0.  g0.8 without g0.7: violation 1.  flag 0 kills violation 2
    (_table(flags=1, g0=G5 | G8, mounts=[P | B1]), (0b0011, 0, [P | B1, 0, 0])),
    # M through bit3 with bit2 set, on the third mount; the first is an ABSENT element (zero word inside the count), the second fails M
    (_table(flags=2, g0=G5, mounts=[0, P | B1 | B2, P | B1 | B2 | B3]), (0b0001, 0, [0, P | B1 | B2, P | B1 | B2 | B3])),
    # the only mount with M is absent (its presence bit is clear): no violation 0; g0.7 kills violation 1; flag 17 brings violation 2 back
    (_table(flags=3 | (1 << 17), g0=G5 | G7 | G8, mounts=[B1, P | B2]), (0b0100, 0, [B1, P | B2, 0])),
    # g0.6 kills violation 0 although M holds
    (_table(flags=1, g0=G5 | G6, mounts=[P | B1]), (0b0010, 0, [P | B1, 0, 0])),
    # the contradictory term never fires (bit1 alone), bit2 & bit4 does: the derived global bit
    (_table(flags=1, mounts=[P | B1]), (0, 0, [P | B1, 0, 0])),
    (_table(flags=1, mounts=[P | B1, P | B2 | B4]), (0, D3, [P | B1, P | B2 | B4, 0])),
    (_table(flags=1, mounts=[B2 | B4]), (0, 0, [B2 | B4, 0, 0])),
    # the join inside a disjunction: volume 1 has the id through bit2, volume 0 has it without either bit, volume 2 has bit1 and another id
    (_table(flags=1, mounts=[P, P], ids=[7, 9], volumes=[_vol(7), _vol(9, B2), _vol(8, B1)]), (0b1000, 0, [P, P | J5, 0])),
    # id 0 equals nothing; an absent volume with everything else right is no volume
    (_table(flags=1, mounts=[P, P], ids=[0, 5], volumes=[_vol(0, B1), _vol(5, B1) & ~1]), (0, 0, [P, P, 0])),
    # the twelfth volume, ids that differ in bit 15 only
    (_table(flags=1, mounts=[P], ids=[0x8003], volumes=[_vol(0x0003, B1)] * 11 + [_vol(0x8003, B1 | B2)]), (0b1000, 0, [P | J5, 0, 0])),
    # the join holds for an absent mount's slot only: its derived bit is set (as in the general form), the violation is not
    (_table(flags=1, mounts=[P, 0], ids=[4, 6], volumes=[_vol(6, B2)]), (0, 0, [P, J5, 0])),
]


def test_dnf_known_answers(tmp_path):
    """the form, the general form (GK_JIT_DNF=0) and the monolithic function answer every hand-built table as written out above"""
    _, form = _plan_text(tmp_path, 2, 4, KA_BLOCKS)
    _, general = _plan_text(tmp_path, 2, 4, KA_BLOCKS, GK_JIT_DNF=0)
    fp = _part_text(form)
    # both loop bodies, all three runs and the join body took the form; their results are tested without the opaque copy.  Violation 3 is
    # the accumulator of an unrolled loop, `b1 | (b2 & v0)` with v0 an extract: it keeps GK_RES
    body = fp[fp.index("switch (part)"):]
    assert body.count("GK_RESC(") == 3 and "GK_BIT(" not in body and body.count("GK_RES(") == 1 and "GK_RES(0, 3, b1);" in body, fp
    assert "(uint32_t)((W0_0 & 7u) == 3u) | (uint32_t)((W0_0 & 11u) == 11u)" in fp          # present & bit1 & !bit2 | present & bit1 & bit3
    assert "(uint32_t)((W0_0 & 21u) == 21u);" in fp                                         # the contradictory term is gone
    assert "(uint32_t)((g0 & 96u) == 32u) & b1" in fp                                       # the loop result enters as an opaque literal
    assert "(uint32_t)((flags & 3u) == 0u) | (uint32_t)((flags & 131072u) == 131072u)" in fp
    assert fp.count("^ xs_) & 16776963u) == 3u) | (uint32_t)(((wq_ ^ xs_) & 16776965u) == 5u)") == 36 and "vid_eq(" not in fp
    assert "GK_RESC" not in general and "GK_BIT(" in _part_text(general) and "vid_eq(" in _part_text(general)
    tables = [t for t, _ in KA_CASES]
    for name, text in (("form", form), ("general", general)):
        got = _run_tables(tmp_path, name, text, tables)
        for (t, (viol, g1, mounts)), ((sv, sw), (mv, mw)) in zip(KA_CASES, got):
            assert (sv, sw[1], sw[4:7]) == (viol, g1, mounts), "%s, staged parts: table %r gives %r" % (name, t, (sv, sw))
            assert (mv, mw[4:7]) == (viol, mounts), "%s, monolithic: table %r gives %r" % (name, t, (mv, mw))


def test_admission_geometry_keeps_its_text(tmp_path):
    """four formula shares per half (64-review groups): the generator's output does not depend on the switch"""
    _, a = _plan_text(tmp_path, 4, 4, KA_BLOCKS)
    _, b = _plan_text(tmp_path, 4, 4, KA_BLOCKS, GK_JIT_DNF=0)
    assert a == b and "GK_RESC" not in a


# ---------------------------------------------------------------------------------------------------------------- differential fuzz
def _rand_formula(rng, leaves, depth):
    r = rng.random()
    if depth == 0 or r < 0.2:
        return ("const", rng.randrange(2)) if rng.random() < 0.05 else ("lit", rng.choice(leaves))
    if r < 0.35:
        return ("not", _rand_formula(rng, leaves, depth - 1))
    return (rng.choice(["and", "and", "or", "andn"]), _rand_formula(rng, leaves, depth - 1), _rand_formula(rng, leaves, depth - 1))


def _lower(f, load, out, nxt):
    """formula -> instructions appended to `out`; returns its register (fresh registers from nxt[0])"""
    if f[0] == "reg":
        return f[1]
    r = nxt[0]
    nxt[0] += 1
    assert r < 64
    if f[0] == "lit":
        out.append(load(r, f[1]))
    elif f[0] == "const":
        out.append(fi(F_CONST, r, f[1]))
    elif f[0] == "not":
        out.append(fi(F_NOT, r, _lower(f[1], load, out, nxt)))
    else:
        x, y = _lower(f[1], load, out, nxt), _lower(f[2], load, out, nxt)
        out.append(fi({"and": F_AND, "or": F_OR, "andn": F_ANDN}[f[0]], r, x, y))
    return r


G0_BITS, FLAG_BITS, ELEM_BITS, G1_BITS = [1, 2, 3, 4, 5, 6], [0, 1, 2, 17], [1, 2, 3, 4], [8, 9, 10, 11]


def _fuzz_plan(rng):
    """random small formulas, each over ONE word: runs over g0, runs over the flags, loop bodies over the mount word whose result is
    mixed into a run over g1 or becomes a derived global bit"""
    blocks, slot, derived = [], 0, 20
    for _ in range(24):
        kind, blk, nxt = rng.randrange(4), [], [8]
        depth = rng.choice([1, 2, 2, 3, 3])
        if kind == 0:
            r = _lower(_rand_formula(rng, G0_BITS, depth), lambda r, b: fi(F_LDG, r, b, 0), blk, nxt)
        elif kind == 1:
            r = _lower(_rand_formula(rng, FLAG_BITS, depth), lambda r, b: fi(F_LDF, r, b), blk, nxt)
        else:
            blk.append(fi(F_LOOP, 0, 0, 1))
            nb = [2]
            rb = _lower(_rand_formula(rng, ELEM_BITS, depth), lambda r, b: fi(F_LDE, r, 0, b), blk, nb)
            nxt[0] = max(8, nb[0])
            blk.append(fi(F_ENDLOOP, 1, rb))
            if kind == 2:
                mix = rng.choice([("and", ("reg", 1), _rand_formula(rng, G1_BITS, 2)), ("or", _rand_formula(rng, G1_BITS, 2), ("not", ("reg", 1))),
                                  ("andn", _rand_formula(rng, G1_BITS, 1), ("reg", 1))])
                r = _lower(mix, lambda r, b: fi(F_LDG, r, 32 + b, 0), blk, nxt)
            else:
                blk.append(fi(F_STG, 1, 32 + derived, 0))
                derived += 1
                blocks.append(blk)
                continue
        blk.append(fi(F_RES, r, 0, slot))
        slot += 1
        blocks.append(blk)
    return blocks, max(slot, 1)


def _fuzz_tables(rng):
    def mount():
        return rng.choice([0, rng.randrange(32) | 1, rng.randrange(32) & ~1])

    def base():
        return [rng.getrandbits(32) & 0xFFFFF, rng.getrandbits(32) & 0xFFFFF], [mount(), mount(), mount()]
    tables = []
    for a in range(64):          # every assignment of the g0 bits
        (g0, g1), m = base()
        tables.append(_table(flags=rng.getrandbits(20), g0=(g0 & ~0x7E) | (a << 1), g1=g1, mounts=m))
    for a in range(16):          # ... of the flag bits
        (g0, g1), m = base()
        tables.append(_table(flags=(rng.getrandbits(17) & ~7) | (a & 7) | ((a >> 3) << 17), g0=g0, g1=g1, mounts=m))
    for a in range(32):          # ... of one mount word (the presence bit among them), in each position, against every assignment of the g1 bits
        for k in range(16):
            (g0, g1), m = base()
            m[(a + k) % 3] = a
            tables.append(_table(flags=rng.getrandbits(20), g0=g0, g1=(g1 & ~0xF00) | (k << 8), mounts=m))
    return tables


@pytest.mark.parametrize("seed", [4101, 4102, 4103, 4104])
def test_dnf_differential_fuzz(tmp_path, seed):
    """seeded random formulas over one word, evaluated bit by bit (the interpreter above), through the DNF analysis (the staged parts with
    the form) and through the monolithic jit_formulas: all three agree on every assignment of the word's bits"""
    rng = random.Random(seed)
    blocks, n_viol = _fuzz_plan(rng)
    code, form = _plan_text(tmp_path, 2, n_viol, blocks)
    _, general = _plan_text(tmp_path, 2, n_viol, blocks, GK_JIT_DNF=0)
    assert form != general and "GK_RESC(" in _part_text(form), "seed %d: the form selects nothing" % seed
    tables = _fuzz_tables(rng)
    for name, text in (("form", form), ("general", general)):
        got = _run_tables(tmp_path, name, text, tables)
        for (flags, w), ((sv, sw), (mv, mw)) in zip(tables, got):
            viol, after = interpret(code, flags, w)
            assert (sv, sw) == (viol, after[:10]), "seed %d, %s, staged parts: flags %#x words %r" % (seed, name, flags, w)
            assert mv == viol, "seed %d, %s, monolithic: flags %#x words %r" % (seed, name, flags, w)


# ---------------------------------------------------------------------------------------------------------------- the bench plan
def _valu(code, tmp_path, name):
    co = os.path.join(str(tmp_path), name + ".co")
    with open(co, "wb") as f:
        f.write(code)
    dis = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", co], capture_output=True, text=True).stdout
    ops = [m.group(1) for m in (re.match(r"\s+([a-z_0-9]+)\s", line) for line in dis.splitlines()) if m]
    return sum(1 for op in ops if op.startswith("v_") and not op.startswith(("v_readlane", "v_writelane", "v_readfirstlane", "v_accvgpr")))


def test_bench_plan_text_holds_the_form_and_compiles_to_fewer_vector_instructions(tmp_path):
    """configs[2] at 256-review groups and the bench tables' register budget: the result formulas over one word are masked compares handed
    to GK_RESC, no test of a formula value in the shares goes through gk_bit but GK_RES's own; the text compiles for gfx950 without
    scratch, and to fewer vector instructions than the text of GK_JIT_DNF=0"""
    texts = {}
    for name, kw in (("on", {}), ("off", {"GK_JIT_DNF": 0})):
        d = tmp_path / name
        d.mkdir()
        _script("dnf_form_util.py", ["text", str(d)], 256, GK_JIT_WAVES=6, **kw)
        (f,) = sorted(d.glob("gk_plan_*.hip"))
        texts[name] = f.read_text()
    part = _part_text(texts["on"])
    part = part[:part.index("}  // namespace gk")]
    assert part.count("GK_RESC(") >= 25 and "GK_BIT(" not in part and "GK_RESC" not in texts["off"]
    lines = {k: [len(c.split("\n")) for c in re.split(r"\n    case \d+: \{\n", _part_text(v))[1:]] for k, v in texts.items()}
    assert max(lines["on"]) < max(lines["off"]), lines   # the heavier share bounds the stage
    rtc = J._hiprtc()
    if rtc is None or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("libhiprtc.so or llvm-objdump is not installed: scratch and the vector-instruction count are not checked")
    valu = {}
    for name, text in texts.items():
        ok, log, code = J.compile_gfx950(rtc, text)
        assert ok, log[-3000:]
        assert J._scratch_bytes(code) == 0, name
        valu[name] = _valu(code, tmp_path, name)
    assert valu["on"] < valu["off"], valu
