"""The review-words analysis (csrc/review_words.hpp) and the list filter on REAL plans and a real table's slot index, without a GPU:
gk_table_review_words computes, on the host, what kernels.hip binds -- the classes of jit_path_classes, analyse_review_words, the bound
paths split into kept and hoisted, build_chunk_lists over the table's slot index with all paths and with the kept ones.
Policies: configs[2] (50 constraints of the PSP family), the 200-template corpus, and required labels alone (review-level tests only:
every class is hoisted, so every row group holds rows of hoisted paths only)."""
import pytest

from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from review_words_util import policy


def report(monkeypatch, name, n, rpt):
    monkeypatch.setenv("GK_RPT", str(rpt))
    drv = D.Driver(device=0, hostemu=True)
    lib = drv.engine.lib
    c = D.Client(drv)
    templates, constraints = policy(name)
    for t in templates:
        c.AddTemplate(t)
    for k in constraints:
        c.AddConstraint(k)
    assert lib.gk_debug_set(b"keep_slot_index", 1) == 0
    try:
        batch = synth.NativeBatch(lib, n, seed=synth.SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
        table = drv.engine.create_table_native(batch.reviews, n, keep_docs=False, resident=True)
    finally:
        lib.gk_debug_set(b"keep_slot_index", 0)
    try:
        r = drv.engine.table_review_words(table)
    finally:
        table.free()
    assert r["rpt"] == rpt and r["groups"] == (n + rpt - 1) // rpt
    return r


@pytest.mark.parametrize("name,n,rpt", [("configs2", 600, 256), ("configs2", 300, 128), ("corpus", 512, 128)])
def test_hoisted_set_and_shorter_lists(monkeypatch, name, n, rpt):
    r = report(monkeypatch, name, n, rpt)
    assert 0 < r["hoisted_classes"] < r["classes"]
    assert 0 < r["k"] <= r["n_gwords"] and len(r["words"]) == r["k"]
    assert r["words"] == sorted(set(r["words"])) and all(0 <= w < r["n_gwords"] for w in r["words"])
    assert r["kept_paths"] + r["hoisted_paths"] == r["bound_paths"] and r["hoisted_paths"] > 0 and r["kept_paths"] > 0
    assert 0 < r["chunks_kept"] < r["chunks_full"] and r["capg_kept"] <= r["capg_full"]
    assert r["overflow_groups_full"] == 0 and r["overflow_groups_kept"] == 0
    assert r["groups_only_hoisted_with_empty_list"] == r["groups_only_hoisted"]
    if name == "configs2":
        assert r["words"] == [0, 1, 2]   # (the issue's figure for configs[2])


def test_groups_with_hoisted_paths_only_get_an_empty_list(monkeypatch):
    r = report(monkeypatch, "labels", 600, 256)
    assert r["hoisted_classes"] == r["classes"] > 0 and 0 < r["k"] <= r["n_gwords"]
    assert r["kept_paths"] == 0 and r["hoisted_paths"] == r["bound_paths"] > 0
    assert r["chunks_full"] > 0 and r["chunks_kept"] == 0 and r["capg_kept"] == 1
    assert r["groups_only_hoisted"] == r["groups"] == 3
    assert r["groups_only_hoisted_with_empty_list"] == 3 and r["overflow_groups_kept"] == 0


def test_table_without_its_slot_index_is_refused(monkeypatch):
    drv = D.Driver(device=0, hostemu=True)
    c = D.Client(drv)
    templates, constraints = policy("labels")
    c.AddTemplate(templates[0])
    c.AddConstraint(constraints[0])
    batch = synth.NativeBatch(drv.engine.lib, 70, seed=synth.SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
    table = drv.engine.create_table_native(batch.reviews, 70, keep_docs=False, resident=True)
    try:
        with pytest.raises(D.EngineError):
            drv.engine.table_review_words(table)
    finally:
        table.free()
