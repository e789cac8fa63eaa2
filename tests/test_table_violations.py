"""Row a11, the list-based audit: gk_table_violations streams every review of a table that has at least one result in the table's most
recent evaluation, with its violation and autoreject masks, in pages -- the device compacts both bitmaps of all plan groups
(gk_tviol_index + gk_tviol_emit; tests/native/hostemu_tviol.cpp on the CPU build), the host merges the pairs its own evaluation of
over-limit reviews added.

Expected answers: plain numpy over the bitmaps a separate downloading Table.eval() returns -- column r of every row of ev.viol / ev.err
(reference()), nothing of the new kernels; where the construction says what must violate, that as well.  The audit leg compares
Client.AuditStream with Client.ReviewBatch(process="audit") and with the oracle client's serial review loop.  The pure cursor / index /
merge logic and the stand-in's loops are covered on their own by tests/test_table_stream_native.py."""
import contextlib

import numpy as np
import pytest

from gatekeeper_amd import _lib as L
from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from oracle import client as OC
from oracle import excluder as OX
from parity_util import BACKENDS, load_both, make_client, plan_group_max, to_oracle_review

TABLE_BACKENDS = [b for b in BACKENDS if b.id in ("hostemu", "gpu")]
C = L.C
PAGES = (64, 100, 1000000)
MOVED = "start again with cursor 0"

DENY_LABEL = '''package k8sdenylabel
violation[{"msg": msg}] {
  want := input.parameters.label
  input.review.object.metadata.labels[want]
  msg := sprintf("label %v is forbidden", [want])
}
'''


def tmpl(kind, rego):
    return {"apiVersion": "templates.gatekeeper.sh/v1", "kind": "ConstraintTemplate", "metadata": {"name": kind.lower()},
            "spec": {"crd": {"spec": {"names": {"kind": kind}}}, "targets": [{"target": D.TARGET_NAME, "rego": rego}]}}


def deny(name, match=None):
    """violated by every object that carries the label `name`"""
    spec = {"parameters": {"label": name}}
    if match:
        spec["match"] = match
    return {"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": "K8sDenyLabel", "metadata": {"name": name}, "spec": spec}


def cm(i, labels, namespace="default"):
    return {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": "obj-%04d" % i, "namespace": namespace, "labels": {x: "y" for x in labels}}}


def rin(obj, ns=None, source=""):
    return D.to_review_in(D.AugmentedUnstructured(D.Unstructured(obj), ns, source))


def violated_rows(i, n, nc):
    """the constraints review i of an n-review table violates.  Bitmap word 0: every review has an entry, each its own set (review 63:
    all constraints); word 1: no review has one; the five last words of a table of more than 1000 reviews: none either; elsewhere every
    third review."""
    w = i // 64
    if w == 1 or (n > 1000 and w >= (n + 63) // 64 - 5):
        return []
    if w == 0:
        return list(range(nc)) if i == 63 else sorted({i % nc} | {j for j in range(nc) if (i * 7 + j * 3) % 11 == 0})
    return [j for j in range(nc) if (i * 5 + j) % 13 == 0] if i % 3 == 0 else []


def reference(ev, skip=()):
    """{review: (violated bitmap rows, autoreject bitmap rows)} of the reviews with a bit in some row of the downloaded bitmaps"""
    n = ev.n_reviews

    def cols(bm):
        if bm is None or bm.size == 0:
            return np.zeros((ev.n_constraints, n), bool)
        return np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)

    v, e = cols(ev.viol), cols(ev.err)
    return {int(r): ([int(x) for x in np.nonzero(v[:, r])[0]], [int(x) for x in np.nonzero(e[:, r])[0]])
            for r in np.nonzero((v | e).any(axis=0))[0] if int(r) not in skip}


def raw(table, cursor, max_entries, flags=0):
    """one raw gk_table_violations -> (status, error text, next cursor)"""
    eng = table.engine
    out = C.POINTER(L.gk_table_violations_out)()
    rc = eng.lib.gk_table_violations(eng.handle, table.handle, cursor, max_entries, flags, C.byref(out))
    if rc != L.GK_OK:
        try:
            eng._check(rc)
        except D.EngineError as e:
            return rc, str(e), None
    nxt = int(out.contents.next_cursor)
    eng.lib.gk_table_violations_free(out)
    return rc, "", nxt


def rows_of(mask_row):
    return [w * 64 + b for w, m in enumerate(mask_row) for b in range(64) if (int(m) >> b) & 1]


def entries_of(pages):
    return {int(r): (rows_of(p["viol"][i]), rows_of(p["err"][i])) for p in pages for i, r in enumerate(p["reviews"])}


def check_pages(table, ev, want, beyond=0, sizes=PAGES):
    """the stream of every page size: exactly `want`, in ascending order, whole words per page, the totals on every page"""
    for size in sizes:
        pages = list(table.violation_pages(size))
        reviews = [int(r) for p in pages for r in p["reviews"]]
        assert reviews == sorted(want), (size, sorted(set(reviews) ^ set(want))[:10])
        assert all(a < b for a, b in zip(reviews, reviews[1:]))
        assert entries_of(pages) == want, size
        for k, p in enumerate(pages):
            assert p["total_entries"] == len(want) and p["beyond_limits"] == beyond and p["n_reviews"] == ev.n_reviews
            assert p["ids"] == [int(x) for x in ev.constraint_ids] and p["mask_words"] == (len(p["ids"]) + 63) // 64
            assert len(p["reviews"]) <= max(size, 64) and (len(p["reviews"]) or len(pages) == 1)   # no empty page inside a stream
            assert (p["next_cursor"] != 0) == (k + 1 < len(pages))
            assert len({int(r) // 64 for r in p["reviews"]} & {int(r) // 64 for q in pages[:k] for r in q["reviews"]}) == 0   # whole words
        if size == 64 and len(want) > 64:
            assert len(pages) > 1
    assert [e[:3] for e in table.violations(sizes[0])] == [(r,) + want[r] for r in sorted(want)]   # the Python generator


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("nc", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_shapes_where_the_kernels_can_go_wrong(backend, nc):
    """mask_words 1, 2 and 3; 1 .. 4 133 reviews (65 bitmap words: 17 blocks of four waves, the last wave and the last word partial);
    a word with 64 entries, a word with none, a run of empty words at the end.  After eval(download=False): the same stream."""
    names = ["l%03d" % j for j in range(nc)]
    c = make_client(backend)
    c.AddTemplate(tmpl("K8sDenyLabel", DENY_LABEL))
    for x in names:
        c.AddConstraint(deny(x))
    eng = c.driver.engine
    row_of = None
    for n in (1, 63, 64, 65, 200, 4133):
        table = eng.create_table([rin(cm(i, [names[j] for j in violated_rows(i, n, nc)])) for i in range(n)])
        try:
            ev = table.eval()
            assert ev.n_plan_groups == 1 and ev.n_constraints == nc and not ev.too_big_reviews()   # (130 distinct formulas: one plan)
            if row_of is None:
                by_id = {c.driver.constraint_id(deny(x)): j for j, x in enumerate(names)}
                row_of = [by_id[int(cid)] for cid in ev.constraint_ids]   # bitmap row -> index into names
            want = reference(ev)
            built = {i: (sorted(row_of.index(j) for j in violated_rows(i, n, nc)), []) for i in range(n) if violated_rows(i, n, nc)}
            assert want == built                                          # the reference says what the construction says
            if n >= 64:
                assert all(i in want for i in range(64)) and len(want[63][0]) == nc
            if n >= 200:
                assert not any(64 <= i < 128 for i in want) and max(want) // 64 >= 2
            if n == 4133:
                assert max(want) // 64 == 59                              # five words without entries behind the last entry
            check_pages(table, ev, want)
            table.eval(download=False)
            assert entries_of(table.violation_pages(100)) == want
            table.eval(download=False, host_eval=False)
            assert entries_of(table.violation_pages(1000000)) == want
        finally:
            table.free()


# ------------------------------------------------------------------------------------------------ 2. plan groups
def group_stream(backend, nc, group_max, n=200):
    """-> ({review: (violated names, autoreject names)}, plan groups) of the n-review table under nc deny-label constraints"""
    names = ["l%03d" % j for j in range(nc)]
    lib = L.load(hostemu=backend.startswith("hostemu"))
    with (plan_group_max(lib, group_max) if group_max else contextlib.nullcontext()):
        c = make_client(backend)
        c.AddTemplate(tmpl("K8sDenyLabel", DENY_LABEL))
        for x in names:
            c.AddConstraint(deny(x))
        name_of = {c.driver.constraint_id(deny(x)): x for x in names}
        table = c.driver.engine.create_table([rin(cm(i, [names[j] for j in violated_rows(i, n, nc)])) for i in range(n)])
        try:
            ev = table.eval()
            want = reference(ev)
            check_pages(table, ev, want)
            ids = [int(x) for x in ev.constraint_ids]
            return {r: ([name_of[ids[j]] for j in v], [name_of[ids[j]] for j in e]) for r, (v, e) in want.items()}, ev.n_plan_groups
        finally:
            table.free()


@pytest.mark.parametrize("nc,group_max,groups", [(130, 50, 3), (50, 20, 3), (50, 5, 10)], ids=["130-by-50", "50-by-20", "50-by-5"])
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_plan_groups_give_the_stream_of_one_plan(backend, nc, group_max, groups):
    """row0 = 0, 50, 100: the middle group's rows straddle bit 64 of the mask; row0 = 0, 20, 40; ten groups: more than the by-value
    descriptor holds, the groups go through device memory.  Every one of them streams what ONE plan streams."""
    one, g1 = group_stream(backend, nc, None)
    many, gn = group_stream(backend, nc, group_max)
    assert g1 == 1 and gn == groups
    assert many == one and len(one) > 64
    assert one == {i: (["l%03d" % j for j in violated_rows(i, 200, nc)], []) for i in range(200) if violated_rows(i, 200, nc)}


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_more_mask_words_than_the_kernel_keeps_in_registers(backend):
    """260 constraints: five mask words -- the emit kernel keeps up to four in registers and beyond that ORs into the entry's own words
    of the output -- and more formulas than one plan holds, so at least two plan groups without any knob"""
    got, groups = group_stream(backend, 260, None)
    assert groups >= 2
    assert got == {i: (["l%03d" % j for j in violated_rows(i, 200, 260)], []) for i in range(200) if violated_rows(i, 200, 260)}
    assert any(v[-1] == "l259" for v, _ in got.values()) and len(got[63][0]) == 260


# ------------------------------------------------------------------------------------------------ 3. the kinds of review
NS_A = {"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": "default", "labels": {"team": "a"}}}
NS_HIDDEN = {"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": "hidden", "labels": {"team": "a"}}}


def delete_without_old_object():
    """a review HandleReview answers with an error (target.go: oldObject cannot be nil for DELETE operations)"""
    return D.AugmentedReview(D.AdmissionRequest({"uid": "u-1", "operation": "DELETE", "kind": {"group": "", "version": "v1", "kind": "ConfigMap"},
                                                 "name": "gone", "namespace": "default"}), None, "Original")


def kinds_client(backend):
    c = make_client(backend)
    c.AddTemplate(tmpl("K8sDenyLabel", DENY_LABEL))
    for k in (deny("l0"), deny("l1"), deny("l2", {"namespaceSelector": {"matchLabels": {"team": "a"}}})):
        c.AddConstraint(k)
    c.SetExcluder([{"excludedNamespaces": ["hidden"], "processes": ["audit"]}])
    return c


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_autoreject_only_excluded_and_rejected_reviews(backend):
    c = kinds_client(backend)
    rins = [rin(cm(0, ["l0"]), NS_A),                   # one violation
            rin(cm(1, [])),                             # complies; its Namespace is not cached: the namespaceSelector constraint autorejects
            rin(cm(2, ["l0"], "hidden"), NS_HIDDEN),    # the Config hides its namespace from the audit process
            D.to_review_in(delete_without_old_object()),   # HandleReview rejects it
            rin(cm(4, ["l0", "l1", "l2"]), NS_A),       # all three
            rin(cm(5, []), NS_A)]                       # nothing
    table = c.driver.engine.create_table(rins, process="audit")
    try:
        assert table.statuses[2] == L.GK_REVIEW_EXCLUDED and table.statuses[3] not in (L.GK_OK, L.GK_REVIEW_EXCLUDED)
        ev = table.eval()
        want = reference(ev)
        ids = [int(x) for x in ev.constraint_ids]
        row = {x: ids.index(c.driver.constraint_id(deny(x))) for x in ("l0", "l1", "l2")}
        assert want == {0: ([row["l0"]], []), 1: ([], [row["l2"]]), 4: (sorted(row.values()), [])}
        check_pages(table, ev, want)
        # rendered: per entry the rows of its set bits in row order -- an err bit gk_render_error's, a viol bit gk_render's
        got = list(table.violations(64, render=True))
        assert [e[:3] for e in got] == [(r,) + want[r] for r in sorted(want)]
        for r, viol, err, rows in got:
            exp = []
            for j in range(len(ids)):
                if j in err:
                    exp += [dict(x, constraint=ids[j]) for x in table.render_error(ids[j], r)]
                if j in viol:
                    exp += [dict(x, constraint=ids[j]) for x in table.render(ids[j], r)]
            assert rows == exp and rows, r
        assert got[1][3][0]["autoreject"] is True and got[0][3][0]["msg"] == "label l0 is forbidden"
    finally:
        table.free()


def psp_client(backend):
    fx = synth.load_fixtures()
    c, oc = load_both(backend, synth.psp_templates(fx), synth.audit_constraints())
    return c, oc


def huge_pod(name):
    """256 containers where predicates iterate elements: beyond the device's limits, answered by the host evaluator"""
    return {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": name, "namespace": "prod-1", "labels": {}},
            "spec": {"containers": [{"name": "c%d" % i, "image": "x", "securityContext": {"privileged": i == 255}} for i in range(256)]}}


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_a_host_evaluated_review_and_one_left_beyond_the_limits(backend):
    c, _ = psp_client(backend)
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(70, seed=5, mixed=True)
    objs[66] = huge_pod("huge-66")
    table = c.driver.engine.create_table([rin(o, synth.namespace_for(o, nss), "Original") for o in objs])
    try:
        ev = table.eval()
        assert ev.host_evaluated == [66] and not ev.too_big_reviews()
        want = reference(ev)
        assert want[66][0] and len(want) > 10                             # its entry comes from the host's pairs
        check_pages(table, ev, want, beyond=0)
        dev = table.eval(host_eval=False)                                 # the device's answer alone: no entry, one review beyond the limits
        assert dev.too_big_reviews() == [66]
        rest = {r: x for r, x in want.items() if r != 66}
        assert reference(dev, skip=(66,)) == rest
        check_pages(table, dev, rest, beyond=1, sizes=(64, 1000000))
        ev = table.eval()                                                 # host-completed again ...
        check_pages(table, ev, want, beyond=0, sizes=(64,))
        table.eval(download=False)                                        # ... and an evaluation that did not complete on the host inherits nothing
        check_pages(table, ev, rest, beyond=1, sizes=(64, 1000000))
    finally:
        table.free()


# ------------------------------------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_what_the_call_refuses(backend):
    c = kinds_client(backend)
    eng = c.driver.engine
    rins = [rin(cm(i, ["l0"]), NS_A) for i in range(130)]
    table, bare = eng.create_table(rins), None
    try:
        rc, err, _ = raw(table, 0, 64)
        assert rc == L.GK_ERR_INVALID and "evaluate the table first" in err                          # never evaluated
        rc, err, _ = raw(table, 0xDEADBEEF, 64)
        assert rc == L.GK_ERR_INVALID
        table.launch()
        rc, err, _ = raw(table, 0, 64)
        assert rc == L.GK_ERR_INVALID and "still to be collected" in err                             # pending launches
        ev = table.eval(collect_only=True)
        want = reference(ev)
        assert sorted(want) == list(range(130))

        def page_one():
            rc, err, nxt = raw(table, 0, 64)
            assert rc == L.GK_OK and nxt, err
            assert raw(table, nxt, 64)[0] == L.GK_OK and raw(table, nxt, 64)[0] == L.GK_OK           # while nothing moves the cursor works, again and again
            return nxt

        def refused(cursor):
            rc, err, _ = raw(table, cursor, 64)
            assert rc == L.GK_ERR_INVALID and MOVED in err, (rc, err)

        saved = page_one()
        refused(0xDEADBEEF), refused(saved ^ 1 << 63), refused(saved ^ 1 << 40), refused(saved + 1000)   # garbage; another generation; a word that is not there
        table.eval()                                                                                 # a second evaluation
        refused(saved)
        saved = page_one()
        table.launch()                                                                               # launches alone move it as well
        table.eval(collect_only=True)
        refused(saved)
        saved = page_one()
        c.AddConstraint(deny("l9"))                                                                  # the policies change
        refused(saved)
        rc, err, _ = raw(table, 0, 64)
        assert rc == L.GK_ERR_INVALID and ("evaluate it again" in err or "create it again" in err)   # (a new label value: the table itself is stale)
        again = eng.create_table(rins)
        try:
            ev = again.eval()
            assert ev.n_constraints == 4
            check_pages(again, ev, reference(ev), sizes=(64,))
            c.RemoveConstraint(deny("l9"))                                                           # a policy change that leaves the table's rows valid
            rc, err, _ = raw(again, 0, 64)
            assert rc == L.GK_ERR_INVALID and "evaluate it again" in err
            assert again.eval().n_constraints == 3 and raw(again, 0, 64)[0] == L.GK_OK
        finally:
            again.free()
        # rendering needs the documents
        bare = eng.create_table(rins[:3], keep_docs=False)
        bare.eval()
        assert raw(bare, 0, 64)[0] == L.GK_OK
        rc, err, _ = raw(bare, 0, 64, L.GK_VIOLATIONS_RENDER)
        assert rc == L.GK_ERR_INVALID and "GK_TABLE_KEEP_DOCS" in err
    finally:
        table.free()
        if bare:
            bare.free()


# ------------------------------------------------------------------------------------------------ 5. the audit's stream
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_audit_stream_is_review_batch_and_the_oracles_loop(backend):
    c, oc = psp_client(backend)
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(200, seed=5, mixed=True)
    objs[7] = huge_pod("huge-7")
    hide = objs[30]["metadata"].get("namespace") or objs[31]["metadata"]["namespace"]
    excl = [{"excludedNamespaces": [hide], "processes": ["audit"]}]
    c.SetExcluder(excl)
    ox = OX.Excluder(excl)
    rv = [D.AugmentedUnstructured(D.Unstructured(o), synth.namespace_for(o, nss), "Original") for o in objs]
    rv[20] = delete_without_old_object()                                  # HandleReview rejects it
    got = list(c.AuditStream(rv, page=64))
    assert [i for i, _ in got] == sorted(i for i, _ in got) and len(got) > 64
    got = dict(got)
    batch = c.ReviewBatch(rv, D.AUDIT_EP, process="audit")
    exp = {i: b for i, b in enumerate(batch) if isinstance(b, D.ReviewFailure) or b}
    assert sorted(got) == sorted(exp)
    for i in exp:
        if isinstance(exp[i], D.ReviewFailure):
            assert isinstance(got[i], D.ReviewFailure) and str(got[i]) == str(exp[i]) and got[i].index == i
        else:
            assert [r.key() for r in got[i]] == [r.key() for r in exp[i]], i
    assert isinstance(got[20], D.ReviewFailure) and not isinstance(got[7], D.ReviewFailure) and got[7]   # rejected; host-evaluated
    # the oracle client's serial loop (manager.go:667-776)
    n_results = 0
    for i, o in enumerate(objs):
        if i != 20 and ox.is_namespace_excluded("audit", o):
            assert i not in got, i
            continue
        try:
            res = oc.review(to_oracle_review(rv[i]), OC.AUDIT_EP)
        except Exception:
            assert i == 20 and isinstance(got.get(i), D.ReviewFailure), i
            continue
        want = sorted((r.constraint["metadata"]["name"], r.msg, r.enforcement_action) for r in res)
        assert sorted((r.constraint["metadata"]["name"], r.msg, r.enforcement_action) for r in got.get(i, [])) == want, i
        n_results += len(want)
    assert n_results > 100 and any(hide == (o["metadata"].get("namespace")) for o in objs)
    # the messages an audit run publishes: one per result, AuditViolationMessages' dicts
    ok = [x for i, x in enumerate(rv) if i != 20]
    msgs = list(c.AuditMessages(ok, "2026-01-01T00:00:00Z", page=100))
    assert len(msgs) == n_results and all(m["eventType"] == "violation_audited" and m["id"] == "2026-01-01T00:00:00Z" for m in msgs)
    first = min(i for i in got if i != 20)
    m0 = msgs[0]                                                          # (the first object's messages come first, in bitmap-row order)
    assert (m0["name"], m0["message"], m0["enforcementAction"], m0["resourceName"]) in \
        {(r.constraint["metadata"]["name"], D.truncate_string(r.msg, 256), r.enforcement_action, objs[first]["metadata"]["name"]) for r in got[first]}
    with pytest.raises(D.ReviewFailure):
        list(c.AuditMessages(rv, "t"))
