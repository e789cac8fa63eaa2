"""The plan-specialised text of configs[2]'s policy with the ratio constraints of tests/test_derived_values.py beside it, through hiprtc
for gfx950 -- no device needed.  A comparison of two derived values is the integer compare of two value ids the plans already make for
two plain leaves, so the text must compile at both geometries, stay within the registers its launch bounds leave a wave, and use no more
scratch than the same build reports for configs[2] alone."""
import re

import pytest

import test_derived_values as T
import test_jit_source as J
import test_self_join_plan_text as PT
from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from test_value_order import _meta_int


def _texts(monkeypatch, tmp_path, rpt, with_ratio, n=1024):
    def run():
        drv = D.Driver(device=0, hostemu=True)
        client = D.Client(drv)
        templates, constraints = PT._policy(2, synth.load_fixtures())
        if with_ratio:
            templates, constraints = templates + T.LIBRARY["ratio"][0], constraints + T.LIBRARY["ratio"][1]
        for t in templates:
            client.AddTemplate(t)
        for k in constraints:
            client.AddConstraint(k)
        batch = synth.NativeBatch(drv.engine.lib, n, seed=synth.SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
        table = drv.engine.create_table_native(batch.reviews, n, keep_docs=False, resident=True)
        table.launch()
        table.eval(download=True, collect_only=True)
        table.free()
    return J._dump_sources(monkeypatch, tmp_path, run, env=[("GK_RPT", rpt)])


def _figures(rtc, texts):
    """[(name, scratch bytes per lane, VGPRs, VGPR budget)] of the texts' code objects; every text must compile"""
    out = []
    for name, text in texts:
        ok, log, code = J.compile_gfx950(rtc, text)
        assert ok, "%s does not compile for gfx950:\n%s" % (name, log[-3000:])
        _, waves = (int(x) for x in re.search(r"__launch_bounds__\((\d+), (\d+)\)", text).groups())
        out.append((name, _meta_int(code, b".private_segment_fixed_size"), _meta_int(code, b".vgpr_count"), 512 // waves // 8 * 8))
    return out


@pytest.mark.parametrize("rpt", [64, 256])
def test_configs2_with_the_ratio_constraints_compiles_for_gfx950(monkeypatch, tmp_path, rpt):
    rtc = J._hiprtc()
    if rtc is None:
        pytest.skip("libhiprtc.so is not installed")
    (tmp_path / "base").mkdir(), (tmp_path / "ratio").mkdir()
    base = _figures(rtc, _texts(monkeypatch, tmp_path / "base", rpt, False))
    texts = _texts(monkeypatch, tmp_path / "ratio", rpt, True)
    assert any(re.search(r"xa_ (<|<=|>|>=) xb_", text) for _, text in texts)   # (the ordering compare of two value ids is in the text)
    ratio = _figures(rtc, texts)
    print("rpt %d: configs[2] alone (text, scratch bytes, VGPRs, budget) %r" % (rpt, base))
    print("rpt %d: configs[2] + ratio constraints %r" % (rpt, ratio))
    for name, scratch, vgprs, budget in ratio:
        assert 0 < vgprs <= budget, "%s: %d VGPRs, budget %d" % (name, vgprs, budget)
        assert 0 <= scratch <= max(s for _, s, _, _ in base), "%s: %d bytes of scratch per lane, configs[2] alone has %r" % (name, scratch, base)
