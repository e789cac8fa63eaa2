"""The review-words variant of the plan-specialised kernel text (csrc/review_words.hpp, csrc/embed_sources.py RW_HOOKS): the words the
plan's all-global predicate classes leave per review come from the binding's array instead of those classes' chunks.  The GPU-less build
dumps the variant with GK_JIT_REVIEW_WORDS=force (jit_source.hpp) and this file puts it through hiprtc beside the plain text of the same
plan: it compiles for gfx950, spills no more than the plain text, and keeps the distance between a row request and its first wait."""
import os

import pytest

import test_jit_source as J
from gatekeeper_amd import driver as D
from gatekeeper_amd import synth


def _meta_int(code, key):
    """an unsigned integer of gk_jit_tiles' kernel metadata (msgpack note record), -1 if not found"""
    i = code.find(key)
    if i < 0:
        return -1
    at = i + len(key)
    v = code[at]
    if v < 0x80:
        return v
    if v in (0xCC, 0xCD, 0xCE):
        n = {0xCC: 1, 0xCD: 2, 0xCE: 4}[v]
        return int.from_bytes(code[at + 1:at + 1 + n], "big")
    return -1


def _table(policy, n):
    fx = synth.load_fixtures()
    templates, constraints = (synth.psp_templates(fx), synth.audit_constraints()) if policy == "configs2" else synth.corpus(fx, 200)
    drv = D.Driver(device=0, hostemu=True)
    client = D.Client(drv)
    for t in templates:
        client.AddTemplate(t)
    for k in constraints:
        client.AddConstraint(k)
    batch = synth.NativeBatch(drv.engine.lib, n, seed=synth.SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
    table = drv.engine.create_table_native(batch.reviews, n, keep_docs=False, resident=True)
    table._keep = (batch, client)
    return table


def _pair(monkeypatch, tmp_path, policy, n, env):
    """(plain text, variant text) of ONE plan and geometry: two evaluations of one table of one engine -- two engines give their key paths
    ids in the order their ingest threads met them, and the register allocation of the two texts would differ by more than the hooks"""
    monkeypatch.setenv("GK_HOSTEMU_KERNEL", "jit")
    monkeypatch.setenv("GK_EMU_GRID", "8")
    monkeypatch.delenv("GK_JIT_REVIEW_WORDS", raising=False)
    for k, v in env:
        monkeypatch.setenv(k, str(v))
    texts = []
    table = _table(policy, n)
    try:
        for sub, force in (("plain", False), ("rw", True)):
            (tmp_path / sub).mkdir()
            monkeypatch.setenv("GK_EMU_HIP_SOURCE_DIR", str(tmp_path / sub))
            if force:
                monkeypatch.setenv("GK_JIT_REVIEW_WORDS", "force")
            table.launch()
            table.eval(download=True, collect_only=True)
            got = {open(os.path.join(str(tmp_path / sub), f)).read() for f in os.listdir(str(tmp_path / sub)) if f.startswith("gk_plan_")}
            assert len(got) == 1, "expected one plan-specialised text, got %d" % len(got)
            texts.append(got.pop())
    finally:
        monkeypatch.delenv("GK_JIT_REVIEW_WORDS", raising=False)
        monkeypatch.delenv("GK_EMU_HIP_SOURCE_DIR", raising=False)
        table.free()
    return texts[0], texts[1]


def _check_pair(tmp_path, plain, rw):
    rtc = J._hiprtc()
    assert "rwords" not in plain and "GK_RW_K" not in plain
    assert "#define GK_RW_K " in rw and "const uint32_t* __restrict__ rwords, uint32_t rw_stride" in rw
    assert rw.count("auto rw_of = ") == 1 and rw.count("rw_of(") == 1 and rw.count("__hip_atomic_fetch_or(&lds[GK_RW_WORD(k) * RPP + rl2]") == 1
    if rtc is None:
        pytest.skip("libhiprtc.so is not installed")
    ok0, log0, code0 = J.compile_gfx950(rtc, plain)
    ok1, log1, code1 = J.compile_gfx950(rtc, rw)
    assert ok0, log0[-3000:]
    assert ok1, "the review-words text does not compile for gfx950:\n%s" % log1[-3000:]
    s0, s1 = J._scratch_bytes(code0), J._scratch_bytes(code1)
    v0, v1 = _meta_int(code0, b".vgpr_spill_count"), _meta_int(code1, b".vgpr_spill_count")
    print("scratch bytes plain %d variant %d; vector spills plain %d variant %d" % (s0, s1, v0, v1))
    assert s0 >= 0 and v0 >= 0
    assert 0 <= s1 <= s0, "the variant uses more scratch (%d bytes per lane) than the plain text (%d)" % (s1, s0)
    assert 0 <= v1 <= v0, "the variant spills more vector registers (%d) than the plain text (%d)" % (v1, v0)
    gaps = J._row_load_wait_gaps(code1, tmp_path)
    if gaps is not None:
        print("row-load wait gaps of the variant: %s" % sorted(gaps)[:6])
        assert gaps and min(gaps) >= 16, "a row load is waited for %d instructions after its request (gaps %s)" % (min(gaps), gaps)


@pytest.mark.parametrize("waves", [6, 8])
def test_bench_plan_variant_compiles_without_more_spills(monkeypatch, tmp_path, waves):
    """configs[2] in the bench tables' geometry (256-review groups) at both register budgets in use: 80 and 64 VGPRs"""
    plain, rw = _pair(monkeypatch, tmp_path, "configs2", 1200, [("GK_RPT", 256), ("GK_JIT_WAVES", waves)])
    _check_pair(tmp_path, plain, rw)


@pytest.mark.parametrize("rpt", [128, 256])
def test_corpus_variant_compiles_without_more_spills(monkeypatch, tmp_path, rpt):
    """the 200-template corpus as one plan, at the two sweep geometries: the variant is only ever asked for with row groups of 128 reviews
    and more (review_words.hpp review_words_wanted; 128 is what the corpus tables get on the device).  A 512-object table's own geometry,
    64-review groups with four formula shares per half, is one the product never builds the variant for; there the hooks cost one vector
    spill under one of the two hiprtc builds this suite can meet -- the ROCm installation's: plain 32 B / 9 spills, variant 12 / 2; the one
    bundled with torch, which a process that imported torch first resolves `libhiprtc.so` to: plain 12 / 2, variant 16 / 3.  At 128 and
    256 both builds give 0 / 0 for both texts."""
    plain, rw = _pair(monkeypatch, tmp_path, "corpus", 512, [("GK_RPT", rpt)])
    assert "#define GK_RPT_K %d\n" % rpt in rw
    _check_pair(tmp_path, plain, rw)


def test_default_text_is_the_text_with_the_switch_off(monkeypatch, tmp_path):
    """the text nobody asked the variant of -- what the product assembles with the switch off, below the size threshold, for a plan without
    all-global classes and at admission geometry -- is the plain one whatever GK_REVIEW_WORDS says, with kernel_body.inc in it as it is (the
    pins of tests/test_plan_text_pins.py hold it byte for byte).  That the PRODUCT asks for this text when the switch is off is checked on the
    device: tests/test_review_words.py::test_switch_off_is_the_text_nobody_asked_the_variant_of."""
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    monkeypatch.delenv("GK_JIT_REVIEW_WORDS", raising=False)
    monkeypatch.delenv("GK_REVIEW_WORDS", raising=False)
    a = J._dump_sources(monkeypatch, tmp_path / "a", J._bench_plan(300), env=[("GK_RPT", 256)])
    b = J._dump_sources(monkeypatch, tmp_path / "b", J._bench_plan(300), env=[("GK_RPT", 256), ("GK_REVIEW_WORDS", 0)])
    assert [t for _, t in a] == [t for _, t in b]
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gatekeeper_amd", "csrc")
    body = "".join(line for line in open(os.path.join(csrc, "kernel_body.inc"), encoding="utf-8") if not line.startswith(("#include", "#pragma once")))
    assert all(body in t and "rwords" not in t for _, t in a)
