"""Self-joins (loop cursors, F_KCMP) change nothing for plans without one: the text handed to hiprtc for the benchmark's
policy sets -- configs[1] (30 PSP constraints), configs[2] (the 50-constraint audit set) and configs[4] (the 200-template
corpus) -- is byte for byte what the engine produced before loop cursors existed.  The hashes were taken on that tree with this
file's own procedure (the GPU-less test build writes the plan-specialised source of every launch to GK_EMU_HIP_SOURCE_DIR)."""
import glob
import hashlib
import os

import pytest

from gatekeeper_amd import driver as D
from gatekeeper_amd import synth

BASE_SHA256 = {
    1: "31d764941f8ba3aeb0b58e446c2e0d494d27718e1cd2d38b7744a78fc41bbb4c",
    2: "01cf31db45b7c6a8d447b9860e0a907466f0312bc3243789ce5e4bcb5e03fd6c",
    4: "70b02f3f4dc7ecc46b85d8346e66271fa4d185342e8bf0a8786b45876d016ab0",
}


def _policy(config, fx):
    if config == 1:
        return synth.psp_templates(fx), synth.psp_constraints()
    if config == 2:
        return synth.psp_templates(fx), synth.audit_constraints()
    return synth.corpus(fx, 200)


def plan_text_sha256(config, out_dir, n=1024):
    """SHA-256 over the distinct plan-specialised sources (sorted) of one resident sweep of `n` synthetic reviews"""
    os.environ["GK_HOSTEMU_KERNEL"] = "jit"
    os.environ["GK_EMU_HIP_SOURCE_DIR"] = str(out_dir)
    os.environ["GK_EMU_GRID"] = "8"
    try:
        fx = synth.load_fixtures()
        templates, constraints = _policy(config, fx)
        drv = D.Driver(device=0, hostemu=True)
        client = D.Client(drv)
        for t in templates:
            client.AddTemplate(t)
        for k in constraints:
            client.AddConstraint(k)
        batch = synth.NativeBatch(drv.engine.lib, n, seed=synth.SEED, mixed=(config != 1), start=0, namespaces=synth.gen_namespaces())
        table = drv.engine.create_table_native(batch.reviews, n, keep_docs=False, resident=True)
        table.launch()
        table.eval(download=True, collect_only=True)
        table.free()
    finally:
        for k in ("GK_HOSTEMU_KERNEL", "GK_EMU_HIP_SOURCE_DIR", "GK_EMU_GRID"):
            os.environ.pop(k, None)
    texts = sorted({open(f).read() for f in glob.glob(os.path.join(str(out_dir), "gk_plan_*.hip"))})
    assert texts, "the emulated sweep produced no plan-specialised source"
    h = hashlib.sha256()
    for t in texts:
        h.update(hashlib.sha256(t.encode()).digest())
    return h.hexdigest()


@pytest.mark.parametrize("config", [1, 2, 4])
def test_headline_plan_text_unchanged(config, tmp_path):
    assert plan_text_sha256(config, tmp_path) == BASE_SHA256[config]


if __name__ == "__main__":   # prints the hashes of the tree it runs in
    import tempfile
    for c in (1, 2, 4):
        with tempfile.TemporaryDirectory() as d:
            print(c, plan_text_sha256(c, d))
