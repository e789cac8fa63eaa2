"""The number of plan groups is invisible to the caller.  A policy set that does not fit one plan is evaluated as several plan groups over
the same table and their bitmap rows are appended; every entry point that walks the groups must then answer what
it answers when the whole set is ONE plan.

Policies: the PSP templates with the audit constraint set (50 constraints), once as one plan and once under plan_group_max(20): three
groups of 20 / 20 / 10 -- the last one smaller than the others, the shape at which a wrong first row or a walk cut off by one shows.
Objects: 300 synthetic ones, five bitmap words, the last partly filled.  The answers of the two engines are compared by (kind, name):
constraint ids differ from engine to engine.  The three-group engine is compared twice: as loaded, and after a constraint of the middle
group was removed and added back (with an evaluation in between) -- the table's per-group state outlives two plan generations."""
import functools

import pytest

from gatekeeper_amd import _lib as L
from gatekeeper_amd import synth
from parity_util import BACKENDS, make_client, plan_group_max
from test_resident_violations import stream as violations_stream   # (the neighbours' helpers, as they are)
from test_step_overhead import _by_name as by_name

TWO = [b for b in BACKENDS if b.id in ("hostemu", "gpu")]
N, SEED, K, PAGE, GROUP_MAX = 300, 23, 3, 64, 20


def _client(backend):
    c = make_client(backend)
    for t in synth.psp_templates(synth.load_fixtures()):
        c.AddTemplate(t)
    for k in synth.audit_constraints():
        c.AddConstraint(k)
    assert len(c.constraints) == 50
    return c


def _names(c):
    return {c.driver.constraint_id(k): key for key, k in c.constraints.items()}


def _table(c):
    batch = synth.NativeBatch(c.driver.engine.lib, N, seed=SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
    table = c.driver.engine.create_table_native(batch.reviews, N, keep_docs=False, resident=True, keep_text=True)
    table._batch = batch   # (the table reads the batch's text)
    return table


def _table_answers(c, table):
    """what gk_table_eval, gk_table_topk and gk_table_totals say about `table`, by (kind, name) -> (answers, n_plan_groups)"""
    name = _names(c)
    ev = table.eval(want_match=True, want_list=True)
    assert ev.n_reviews == N and ev.n_tiles == 5 and ev.n_constraints == len(name) and ev.match is not None
    row_name = [name[int(cid)] for cid in ev.constraint_ids]
    assert ev.list_total == len(ev.list)
    ans = {"viol": by_name(c, ev, "viol"), "err": by_name(c, ev, "err"), "match": by_name(c, ev, "match"), "too_big": ev.too_big.tobytes(),
           "counts": {row_name[i]: int(n) for i, n in enumerate(ev.counts)},
           "list": sorted((row_name[int(row)], int(review)) for row, review in ev.list),
           "topk": {name[cid]: (sorted(reviews), overflow) for cid, (reviews, overflow) in table.topk(K).items()},
           "totals": {name[cid]: v for cid, v in table.totals().items()}}
    assert len(set(ans["list"])) == len(ans["list"]) and len(ans["topk"]) == len(ans["totals"]) == len(name)
    return ans, ev.n_plan_groups


def _put_objects(c):
    for o in list(synth.gen_namespaces().values()) + synth.gen_objects(N, seed=SEED, mixed=True):
        c.AddData(o)


def _resident_answers(c, backend, n_groups):
    """what the resident entry points say about the set, by (kind, name); the verification is asserted here: its answer is not a comparison
    between engines but "no differences, every group that has a specialised build was compared" """
    name = _names(c)
    d = c.driver
    sweep, audit = d.ResidentSweep(), d.ResidentAudit(K)
    assert sweep["n_chunks"] == audit["n_chunks"] == 1 and sorted(sweep["pairs"]) == sorted(audit["pairs"]) == sorted(name)
    pages = violations_stream(c, PAGE, 0)
    assert all(p["ids"] == pages[0]["ids"] and p["total"] == pages[0]["total"] for p in pages) and sorted(pages[0]["ids"]) == sorted(name)
    ans = {"n_objects": sweep["n_objects"], "beyond": (sweep["beyond_limits"], audit["beyond_limits"], pages[0]["beyond"]),
           "sweep_pairs": {name[cid]: n for cid, n in sweep["pairs"].items()},
           "audit_pairs": {name[cid]: n for cid, n in audit["pairs"].items()},
           "audit_err_pairs": {name[cid]: n for cid, n in audit["err_pairs"].items()},
           "audit_lists": {name[cid]: (sorted(paths), overflow) for cid, (paths, overflow) in audit["lists"].items()},
           "stream_total": pages[0]["total"], "stream_pages": [len(p["entries"]) for p in pages],
           "stream": [(path, sorted(name[i] for i in viol), sorted(name[i] for i in err)) for p in pages for path, viol, err, _ in p["entries"]]}
    v = d.VerifyResident()
    assert v.diff_total == 0 and v.diff_too_big == 0 and v.entries_total == 0 and v.quarantined_groups == 0
    assert v.n_plan_groups == n_groups and v.specialised_groups == (n_groups if backend == "gpu" else 0)   # (plain hostemu has no specialised side)
    assert sorted(v.constraint_ids) == sorted(name)
    return ans


@functools.lru_cache(maxsize=None)
def _one_plan_table(backend):
    c = _client(backend)
    table = _table(c)
    try:
        ans, groups = _table_answers(c, table)
    finally:
        table.free()
    assert groups == 1
    assert sum(ans["counts"].values()) > 100 and len(ans["list"]) == sum(ans["counts"].values())   # or the comparison shows nothing
    assert any(r for r, _ in ans["topk"].values()) and any(results > pairs for results, pairs in ans["totals"].values())
    return ans


@functools.lru_cache(maxsize=None)
def _one_plan_resident(backend):
    c = _client(backend)
    _put_objects(c)
    ans = _resident_answers(c, backend, 1)
    assert ans["stream_total"] > 2 * PAGE and len(ans["stream_pages"]) > 2 and sum(ans["sweep_pairs"].values()) > 100
    assert sum(ans["audit_err_pairs"].values()) > 0 and any(paths for paths, _ in ans["audit_lists"].values())
    return ans


def _middle_group_constraint(c, ev_ids):
    """a constraint whose bitmap row lies in the middle group"""
    by_id = {c.driver.constraint_id(k): k for k in c.constraints.values()}
    return by_id[int(ev_ids[GROUP_MAX + 7])]


@pytest.mark.parametrize("backend", TWO)
def test_table_entry_points_answer_alike_for_one_plan_and_three_groups(backend):
    want = _one_plan_table(backend)
    with plan_group_max(L.load(hostemu=backend.startswith("hostemu")), GROUP_MAX):
        c = _client(backend)
        table = _table(c)
        try:
            got, groups = _table_answers(c, table)
            assert groups == 3
            assert got == want
            moved = _middle_group_constraint(c, table.eval().constraint_ids)
            c.RemoveConstraint(moved)
            ev = table.eval()
            assert ev.n_constraints == 49 and ev.n_plan_groups == 3
            c.AddConstraint(moved)
            got, groups = _table_answers(c, table)
            assert groups == 3
            assert got == want
        finally:
            table.free()


@pytest.mark.parametrize("backend", TWO)
def test_resident_entry_points_answer_alike_for_one_plan_and_three_groups(backend):
    want = _one_plan_resident(backend)
    with plan_group_max(L.load(hostemu=backend.startswith("hostemu")), GROUP_MAX):
        c = _client(backend)
        _put_objects(c)
        assert _resident_answers(c, backend, 3) == want
        ids = violations_stream(c, PAGE, 0)[0]["ids"]
        moved = _middle_group_constraint(c, ids)
        c.RemoveConstraint(moved)
        sweep = c.driver.ResidentSweep()
        assert len(sweep["pairs"]) == 49 and sweep["n_chunks"] == 1
        c.AddConstraint(moved)
        assert _resident_answers(c, backend, 3) == want
