"""Rows a11 + f2: the per-result half of an audit run over the RESIDENT set (pkg/audit/manager.go:927-939: logViolation, Publish,
emitEvent for every single result) -- gk_resident_violations streams every shown object that has at least one result, with the constraints
it has them for, in pages: the device compacts the sweep's bitmaps (gk_viol_any + gk_viol_emit), the host merges autoreject pairs and
host-evaluated pairs.

Expected answers: the oracle client's serial loop over the cached objects (serial_loop, restated from tests/test_resident_audit.py); the
product's own AuditFromCache is a second leg.  The pure page / cursor / merge logic and the CPU stand-in's loops are covered on their own by
tests/test_viol_stream_native.py."""
import json

import pytest

from gatekeeper_amd import _lib as L
from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from oracle import client as OC
from oracle import excluder as OX
from oracle import target as OT
from parity_util import BACKENDS, load_both, plan_group_max

RESIDENT_BACKENDS = [b for b in BACKENDS if b.id in ("hostemu", "gpu")]
C = L.C
MATCH_ERR = "unable to match constraints: "
MOVED = "the resident set or the policies changed since the stream began: start again with cursor 0"
PAGES = (64, 100, 1000000)


def ckey(c):
    return (c.get("kind", ""), c.get("apiVersion", ""), (c.get("metadata") or {}).get("name", ""))


def serial_loop(oc, cached, hidden=None, memo=None, sig=None):
    """auditFromCache (manager.go:591-642): nsMap from the cached Namespaces, one Review per cached object that the audit process shows,
    with AugmentedUnstructured{obj, ns}.  -> [(Result, obj)].  memo / sig: one Review per distinct signature while the policies stand."""
    ns_map = {o["metadata"]["name"]: o for o in cached.values() if o.get("kind") == "Namespace" and o.get("apiVersion") == "v1"}
    results = []
    for o in cached.values():
        if hidden is not None and hidden(o):
            continue
        ns = ns_map.get((o.get("metadata") or {}).get("namespace") or "")
        if memo is None:
            res = oc.review(OT.AugmentedUnstructured(OT.Unstructured(o), ns, ""), OC.AUDIT_EP, ns)
        else:
            s = sig(o, ns)
            if s not in memo:
                memo[s] = oc.review(OT.AugmentedUnstructured(OT.Unstructured(o), ns, ""), OC.AUDIT_EP, ns)
            res = memo[s]
        results += [(r, o) for r in res]
    return results


def text_sig(o, ns):
    return json.dumps(o, sort_keys=True), json.dumps(ns, sort_keys=True)


def label_sig(o, ns=None):
    return tuple(sorted(o["metadata"].get("labels") or ()))


# the oracle's answers for the PSP / audit_constraints policy set, shared by every test and backend that loads exactly that set
PSP_MEMO = {}


def shuffled(xs, seed):
    rng, xs = synth.SplitMix64(seed), list(xs)
    for i in range(len(xs) - 1, 0, -1):
        j = rng.below(i + 1)
        xs[i], xs[j] = xs[j], xs[i]
    return xs


def expected_sets(results):
    """{path: (violated constraint keys, autoreject constraint keys)} of the oracle's results"""
    out = {}
    for r, o in results:
        v, e = out.setdefault(tuple(D.process_data(o)), (set(), set()))
        (e if r.msg.startswith(MATCH_ERR) else v).add(ckey(r.constraint))
    return out


def call(c, cursor, max_objects, flags=L.GK_VIOLATIONS_RENDER):
    """one raw gk_resident_violations -> (status, error text, page dict or None)"""
    eng = c.driver.engine
    out = C.POINTER(L.gk_violations_out)()
    rc = eng.lib.gk_resident_violations(eng.handle, cursor, max_objects, flags, C.byref(out))
    if rc != L.GK_OK:
        try:
            eng._check(rc)
        except D.EngineError as e:
            return rc, str(e), None
    o = out.contents
    ids, mw = [int(o.constraint_ids[i]) for i in range(o.n_constraints)], int(o.mask_words)
    assert mw == (len(ids) + 63) // 64

    def bits(arr, i):
        m = 0
        for w in range(mw):
            m |= int(arr[i * mw + w]) << (64 * w)
        assert m >> len(ids) == 0
        return [ids[r] for r in range(len(ids)) if (m >> r) & 1]

    page = {"total": int(o.total_objects), "next": int(o.next_cursor), "beyond": int(o.beyond_limits), "n_objects": int(o.n_objects), "n_chunks": int(o.n_chunks), "ids": ids,
            "entries": [(tuple(json.loads(o.paths[i].decode())), bits(o.viol, i), bits(o.err, i), o.results_json[i] if flags & L.GK_VIOLATIONS_RENDER else None)
                        for i in range(o.n_entries)]}
    assert (flags & L.GK_VIOLATIONS_RENDER) or not o.results_json
    eng.lib.gk_violations_free(out)
    return rc, "", page


def stream(c, max_objects, flags=L.GK_VIOLATIONS_RENDER):
    """the whole stream from cursor 0 -> [page dict]"""
    pages, cursor = [], 0
    while True:
        rc, err, page = call(c, cursor, max_objects, flags)
        assert rc == L.GK_OK, err
        pages.append(page)
        cursor = page["next"]
        if not cursor:
            return pages
        assert len(pages) < 100000


def review_bytes(c, path):
    """gk_resident_review's answer as the bytes it returns"""
    eng = c.driver.engine
    arr = (C.c_char_p * len(path))(*[p.encode() for p in path])
    out = C.c_void_p()
    eng._check(eng.lib.gk_resident_review(eng.handle, arr, len(path), C.byref(out)))
    text = C.string_at(out)
    eng.lib.gk_free(out)
    return text


def check_stream(c, want, page_sizes=PAGES, beyond=0, absent=()):
    """test 1's checks from cursor 0, for every page size; `want` = the oracle's [(Result, obj)]; `absent`: cached paths that are beyond the
    engine's limits (their review fails instead of answering []).  -> the entries of the last stream"""
    exp = expected_sets(want)
    key_of = {c.driver.constraint_id(k): ckey(k) for k in c.constraints.values()}
    audit = c.driver.ResidentAudit(0)
    entries = None
    for size in page_sizes:
        pages = stream(c, size)
        entries = [e for p in pages for e in p["entries"]]
        paths = [e[0] for e in entries]
        assert len(set(paths)) == len(paths)                                     # each object once
        assert set(paths) == set(exp), (size, set(paths) ^ set(exp))             # exactly the objects the oracle has results for
        for path, viol, err, _ in entries:
            assert ({key_of[i] for i in viol}, {key_of[i] for i in err}) == exp[path], (size, path)
        for p in pages:
            assert p["total"] == len(entries) and p["beyond"] == beyond and p["n_objects"] == len(c.cached) and p["ids"] == pages[0]["ids"]
            assert len(p["entries"]) <= max(size, 64) and (p["entries"] or len(pages) == 1)   # no empty page inside a stream
        # column sums over all pages = gk_resident_audit's pair totals
        assert sorted(pages[0]["ids"]) == sorted(audit["pairs"])
        assert {i: sum(1 for e in entries if i in e[1]) for i in pages[0]["ids"]} == audit["pairs"]
        assert {i: sum(1 for e in entries if i in e[2]) for i in pages[0]["ids"]} == audit["err_pairs"]
        assert pages[0]["n_chunks"] == audit["n_chunks"]
    for path, _, _, text in entries:                                             # rendered: byte for byte gk_resident_review's answer
        assert text == review_bytes(c, path), path
    named = {e[0] for e in entries}
    for path in c.cached:
        if path not in named and path not in absent:
            assert c.driver.ResidentReview(list(path)) == [], path
    # without rendering: the same entries
    assert [e[:3] for p in stream(c, page_sizes[0], 0) for e in p["entries"]] == [e[:3] for p in stream(c, page_sizes[0]) for e in p["entries"]]
    # the Python generators
    assert [(p, v, e) for p, v, e, _ in c.driver.ResidentViolations(page_sizes[0], render=False)] == [e[:3] for p in stream(c, page_sizes[0]) for e in p["entries"]]
    got = dict(c.AuditStreamFromCache(page=page_sizes[0]))
    full = c.AuditFromCache()[0]
    assert {p: [r.key() for r in rs] for p, rs in got.items()} == {p: [r.key() for r in rs] for p, rs in full.items() if not isinstance(rs, D.ReviewFailure) and rs}
    assert {p: sorted((ckey(r.constraint), r.msg) for r in rs) for p, rs in got.items()} == \
        {p: sorted((ckey(r.constraint), r.msg) for r, o in want if tuple(D.process_data(o)) == p) for p in exp}
    return entries


def psp_set(c, oc):
    """test 1's set: the namespaces plus 700 mixed objects, put in shuffled order (slot order != key order)"""
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(700, seed=23, mixed=True)
    for o in shuffled(list(nss.values()) + objs, 7):
        c.AddData(o), oc.add_data(o)
    return nss, objs


# ------------------------------------------------------------------------------------------------ 1. parity, exactly once
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_stream_names_every_violating_object_once(backend, fixtures):
    c, oc = load_both(backend, synth.psp_templates(fixtures), synth.audit_constraints())
    psp_set(c, oc)
    want = serial_loop(oc, c.cached, memo=PSP_MEMO, sig=text_sig)
    entries = check_stream(c, want)
    assert len(entries) > 128 and len(stream(c, 64)) > 2
    exp = expected_sets(want)
    # (reviews without a Source: the constraints that match on `source` answer with a match error per Pod -- autoreject results)
    assert sum(1 for r, _ in want if r.msg.startswith(MATCH_ERR)) > 50
    assert sum(1 for v, e in exp.values() if e and not v) > 0 and sum(1 for v, e in exp.values() if e and v) > 0   # err-only objects, and both kinds
    assert len(exp) < len(c.cached)                                              # ... and objects without any result


# ------------------------------------------------------------------------------------------------ 2. shapes
NEED_LABEL = '''package k8sneedlabel
violation[{"msg": msg}] {
  want := input.parameters.label
  not input.review.object.metadata.labels[want]
  msg := sprintf("label %v is missing", [want])
}
'''


def tmpl(kind, rego):
    return {"apiVersion": "templates.gatekeeper.sh/v1", "kind": "ConstraintTemplate", "metadata": {"name": kind.lower()},
            "spec": {"crd": {"spec": {"names": {"kind": kind}}}, "targets": [{"target": D.TARGET_NAME, "rego": rego}]}}


def need_label(name):
    """violated by every object that does not carry the label `name`"""
    return {"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": "K8sNeedLabel", "metadata": {"name": name}, "spec": {"parameters": {"label": name}}}


def labelled(name, namespace, violates, all_names):
    return {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": name, "namespace": namespace, "labels": {x: "y" for x in all_names if x not in violates}}}


@pytest.mark.parametrize("group_max", [None, 24], ids=["one-plan", "groups-of-24"])
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_shapes_where_the_kernels_can_go_wrong(backend, group_max):
    """130 objects in one chunk = three bitmap words, the last with two slots.  Word 0: all 64 slots violate, each its own set of
    constraints (slot i: constraint i, plus a spread of others; slot 63 all 70).  Word 1: a namespace whose 64 objects all comply -- a
    word without entries between words with entries.  Word 2: slot 128 violates constraint 69 alone (mask word 1 only), slot 129 complies.
    70 constraints of one template: two row blocks in the transpose, a row count that is no multiple of 64; with groups of 24: three views
    at row offsets 0, 24, 48, the last of 22 rows."""
    names = ["l%02d" % j for j in range(70)]
    import contextlib
    with (plan_group_max(L.load(hostemu=backend.startswith("hostemu")), group_max) if group_max else contextlib.nullcontext()):
        c, oc = load_both(backend, [tmpl("K8sNeedLabel", NEED_LABEL)], [need_label(x) for x in names])
        violates = {}
        for i in range(64):
            violates[i] = set(names) if i == 63 else {names[i]} | {names[j] for j in range(70) if (i * 7 + j * 3) % 11 == 0}
        violates[128] = {names[69]}
        for i in range(130):
            o = labelled("obj-%03d" % i, "busy" if i < 64 else "clean" if i < 128 else "tail", violates.get(i, set()), names)
            c.AddData(o), oc.add_data(o)
        want = serial_loop(oc, c.cached, memo={}, sig=label_sig)
        entries = check_stream(c, want)
        if group_max:
            table = c.driver.engine.create_table([D.to_review_in(D.AugmentedUnstructured(D.Unstructured(c.cached[entries[0][0]]), None, ""))])
            try:
                assert table.eval().n_plan_groups == 3
            finally:
                table.free()
    # slot order, and the masks the construction says (the oracle said the same in check_stream)
    assert [e[0][-1] for e in entries] == ["obj-%03d" % i for i in sorted(violates)]
    name_of = {c.driver.constraint_id(k): k["metadata"]["name"] for k in c.constraints.values()}
    assert [{name_of[i] for i in e[1]} for e in entries] == [violates[i] for i in sorted(violates)]
    pages = stream(c, 64)
    assert [len(p["entries"]) for p in pages] == [64, 1]                         # the empty word is skipped, a page takes whole words


# ------------------------------------------------------------------------------------------------ 3. masks and chunks
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_masks_chunks_and_a_removed_constraint(backend, fixtures):
    c, oc = load_both(backend, synth.psp_templates(fixtures), synth.audit_constraints())
    nss, objs = psp_set(c, oc)
    pods = [o for o in objs if o["kind"] == "Pod"]
    # the Config hides one namespace (one that has violating pods) from the audit process
    want = serial_loop(oc, c.cached, memo=PSP_MEMO, sig=text_sig)
    per_ns = {}
    for r, o in want:
        per_ns[o["metadata"].get("namespace")] = per_ns.get(o["metadata"].get("namespace"), 0) + 1
    hide = max((ns for ns in per_ns if ns), key=lambda ns: (per_ns[ns], ns))
    entries = [{"excludedNamespaces": [hide], "processes": ["audit"]}]
    c.SetExcluder(entries)
    ox = OX.Excluder(entries)
    hidden = lambda o: ox.is_namespace_excluded("audit", o)   # noqa: E731
    want_hidden = serial_loop(oc, c.cached, hidden=hidden, memo=PSP_MEMO, sig=text_sig)
    assert 0 < len(want_hidden) < len(want)
    got = check_stream(c, want_hidden, (64, 1000000))
    assert not any(p[1] == hide for p, _, _, _ in got if p[0] == "namespace")
    # seven pods change, two disappear, three appear: a second chunk, dead slots in the first
    rng = synth.SplitMix64(5)
    for k in range(7):
        o = json.loads(json.dumps(pods[rng.below(len(pods))]))
        o["spec"]["hostNetwork"] = True
        o["spec"]["containers"][0].setdefault("securityContext", {})["privileged"] = k % 2 == 0
        c.AddData(o), oc.add_data(o)
    for o in (pods[3], pods[11]):
        c.RemoveData(o), oc.remove_data(o)
    for o in synth.gen_objects(3, seed=99, start=5000):
        c.AddData(o), oc.add_data(o)
    want2 = serial_loop(oc, c.cached, hidden=hidden, memo=PSP_MEMO, sig=text_sig)
    check_stream(c, want2, (64, 1000000))
    assert c.driver.ResidentSweep()["n_chunks"] == 2 and expected_sets(want2) != expected_sets(want_hidden)
    # a constraint goes: the row count changes
    k_ = synth.audit_constraints()[0]
    c.RemoveConstraint(k_), oc.remove_constraint(k_)
    want3 = serial_loop(oc, c.cached, hidden=hidden)
    check_stream(c, want3, (64, 1000000))
    assert len(stream(c, 64)[0]["ids"]) == len(synth.audit_constraints()) - 1


# ------------------------------------------------------------------------------------------------ 4. a stale cursor
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_a_stale_cursor_is_refused(backend, fixtures):
    c, oc = load_both(backend, synth.psp_templates(fixtures), synth.audit_constraints())
    nss, objs = psp_set(c, oc)
    pods = [o for o in objs if o["kind"] == "Pod"]

    def page_one():
        rc, err, page = call(c, 0, 64)
        assert rc == L.GK_OK and page["next"] and 0 < len(page["entries"]) <= 64, err
        rc2, err2, page2 = call(c, page["next"], 64)                             # (while nothing moves the cursor works, again and again)
        assert rc2 == L.GK_OK and page2["entries"] and call(c, page["next"], 64)[2]["entries"] == page2["entries"], err2
        return page["next"]

    def refused(cursor):
        rc, err, page = call(c, cursor, 64)
        assert rc == L.GK_ERR_INVALID and MOVED in err and page is None, (rc, err)

    rc, err, _ = call(c, 0xDEADBEEF, 64)                                         # before any stream began
    assert rc == L.GK_ERR_INVALID and MOVED in err
    saved = page_one()
    refused(0xDEADBEEF)
    refused(saved ^ 1 << 63), refused(saved | 0xFFFFFFF), refused(saved + (1 << 28) * 200)   # another generation, a word / a chunk that is not there

    def changed_pod(k):
        o = json.loads(json.dumps(pods[k]))
        o["spec"]["hostNetwork"] = not o["spec"].get("hostNetwork", False)
        return o

    o = changed_pod(5)
    c.AddData(o), oc.add_data(o)                                                 # a put that leaves the set unswept
    refused(saved)
    c.driver.ResidentSweep()                                                     # ... and swept by somebody else: the stream's answer has moved all the same
    refused(saved)
    check_stream(c, serial_loop(oc, c.cached, memo=PSP_MEMO, sig=text_sig), (64,))   # cursor 0 is right again
    saved = page_one()
    c.RemoveData(pods[8]), oc.remove_data(pods[8])
    refused(saved)
    saved = page_one()
    k_ = synth.audit_constraints()[0]
    c.RemoveConstraint(k_), oc.remove_constraint(k_)
    refused(saved)
    c.driver.ResidentSweep()
    refused(saved)
    saved = page_one()
    entries = [{"excludedNamespaces": [pods[0]["metadata"]["namespace"]], "processes": ["audit"]}]
    c.SetExcluder(entries)
    refused(saved)
    c.driver.ResidentSweep()
    refused(saved)
    ox = OX.Excluder(entries)
    check_stream(c, serial_loop(oc, c.cached, hidden=lambda o: ox.is_namespace_excluded("audit", o)), (64,))


# ------------------------------------------------------------------------------------------------ 5. host-evaluated objects
PRIVILEGED = '''package noprivileged
violation[{"msg": msg}] {
  k := input.review.object.spec.containers[_]
  k.securityContext.privileged == true
  msg := sprintf("container %v is privileged", [k.name])
}
'''
OWNED = 'package ownedbyrs\nviolation[{"msg": "owned"}] {\n  o := input.review.object.metadata.ownerReferences[_]\n  o.kind == "ReplicaSet"\n  o.controller == true\n}\n'


@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_host_evaluated_objects_are_entries_and_refused_ones_are_counted(backend):
    cons = [{"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": "NoPrivileged", "metadata": {"name": "np"}, "spec": {}},
            {"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": "OwnedByRS", "metadata": {"name": "o"}, "spec": {}}, need_label("team")]
    c, oc = load_both(backend, [tmpl("NoPrivileged", PRIVILEGED), tmpl("OwnedByRS", OWNED), tmpl("K8sNeedLabel", NEED_LABEL)], cons)

    def pod(name, n, privileged=(), labels=None, owners=0):
        md = {"name": name, "namespace": "default", "labels": labels if labels is not None else {"team": "x"}}
        if owners:
            md["ownerReferences"] = [{"kind": "ReplicaSet", "name": "r%d" % i, "controller": i == owners - 1} for i in range(owners)]
        return {"apiVersion": "v1", "kind": "Pod", "metadata": md,
                "spec": {"containers": [dict({"name": "c%d" % i, "image": "x"}, **({"securityContext": {"privileged": True}} if i in privileged else {})) for i in range(n)]}}

    objs = [pod("small-%02d" % i, 2, privileged=(1,) if i % 3 == 0 else (), labels={} if i % 4 == 0 else None) for i in range(70)]
    objs.insert(40, pod("huge-priv", 300, privileged=(299,)))                    # beyond the device's 255 elements: completed by the host evaluator
    objs.insert(41, pod("huge-clean", 300))                                      # ... completed as well, nothing found
    objs.insert(42, pod("huge-label", 300, labels={}))                           # ... found by a constraint that iterates nothing
    objs.insert(43, pod("owned", 1, owners=301))                                 # stays beyond the limits: fails closed
    for o in objs:
        c.AddData(o), oc.add_data(o)
    want = serial_loop(oc, c.cached)
    owned = tuple(D.process_data(objs[43]))
    assert any(tuple(D.process_data(o)) == owned for _, o in want)               # the oracle has a result for it; the engine refuses it
    with pytest.raises(D.LimitError):
        c.driver.ResidentSweep(), c.driver.ResidentReview(list(owned))
    entries = check_stream(c, [(r, o) for r, o in want if tuple(D.process_data(o)) != owned], beyond=1, absent={owned})
    by_name = {e[0][-1]: e for e in entries}
    name_of = {c.driver.constraint_id(k): k["metadata"]["name"] for k in c.constraints.values()}
    assert {name_of[i] for i in by_name["huge-priv"][1]} == {"np"} and {name_of[i] for i in by_name["huge-label"][1]} == {"team"}
    assert "huge-clean" not in by_name and "owned" not in by_name
    assert [e[0][-1] for e in entries] == [o["metadata"]["name"] for o in objs if o["metadata"]["name"] in by_name]   # slot order, host-only slots in their place


# ------------------------------------------------------------------------------------------------ 6. violationMsg
def export_msg(r, o, timestamp, msg_size=256):
    """violationMsg (manager.go:1188-1212) as JSON would carry it (ExportMsg's tags, omitempty: pkg/export/util/util.go:72-90), from
    an oracle Result and the object"""
    k = r.constraint
    ann = dict((k.get("metadata") or {}).get("annotations") or {})
    ann.pop("kubectl.kubernetes.io/last-applied-configuration", None)
    cg, _, cv = k["apiVersion"].rpartition("/")
    g, _, v = o["apiVersion"].rpartition("/")
    md = o.get("metadata") or {}
    m = {"id": timestamp, "eventType": "violation_audited", "group": cg, "version": cv, "kind": k["kind"], "name": k["metadata"]["name"],
         "namespace": k["metadata"].get("namespace", ""), "message": D.truncate_string(r.msg, msg_size), "enforcementAction": r.enforcement_action,
         "enforcementActions": list(r.scoped_enforcement_actions or []), "constraintAnnotations": ann, "resourceGroup": g, "resourceAPIVersion": v,
         "resourceKind": o["kind"], "resourceNamespace": md.get("namespace", ""), "resourceName": md.get("name", ""), "resourceLabels": dict(md.get("labels") or {})}
    m = {a: b for a, b in m.items() if b not in ("", {}, [])}
    if not r.msg.startswith(MATCH_ERR):
        m["details"] = (r.metadata or {}).get("details", {})
    return m


@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_violation_messages(backend, fixtures):
    cons = synth.audit_constraints()
    cons[1] = json.loads(json.dumps(cons[1]))
    cons[1]["metadata"]["annotations"] = {"owner": "platform", "kubectl.kubernetes.io/last-applied-configuration": "{\"a\": 1}"}
    cons.append(need_label("must-have"))                                         # (violated by every object, cluster-scoped and label-less ones included)
    c, oc = load_both(backend, synth.psp_templates(fixtures) + [tmpl("K8sNeedLabel", NEED_LABEL)], cons)
    psp_set(c, oc)
    bare = {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": "bare", "namespace": "default"}}
    c.AddData(bare), oc.add_data(bare)
    want = serial_loop(oc, c.cached)
    stamp = "2026-01-01T00:00:00Z"
    exp = [export_msg(r, o, stamp, 40) for r, o in want]
    got = list(c.AuditViolationMessages(stamp, page=100, msg_size=40))
    canon = lambda ms: sorted(json.dumps(m, sort_keys=True) for m in ms)   # noqa: E731
    assert canon(got) == canon(exp)
    assert any("constraintAnnotations" in m for m in got) and not any("last-applied" in json.dumps(m.get("constraintAnnotations", {})) for m in got)
    assert any(m.get("constraintAnnotations") == {"owner": "platform"} for m in got)
    assert any("resourceLabels" not in m and m["resourceName"] == "bare" for m in got)       # an object without labels
    assert any("resourceNamespace" not in m and m["resourceKind"] == "Namespace" for m in got)   # a cluster-scoped object
    assert any("details" not in m for m in got) and any("details" in m for m in got) and any(m["message"].endswith("...") for m in got)
    assert all(m["eventType"] == "violation_audited" and m["id"] == stamp for m in got)


# ------------------------------------------------------------------------------------------------ edge calls
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_edge_calls(backend):
    c, oc = load_both(backend, [tmpl("K8sNeedLabel", NEED_LABEL)], [need_label("team")])
    eng = c.driver.engine
    eng.lib.gk_violations_free(None)
    out = C.POINTER(L.gk_violations_out)()
    assert eng.lib.gk_resident_violations(None, 0, 64, 0, C.byref(out)) == L.GK_ERR_INVALID and eng.lib.gk_resident_violations(eng.handle, 0, 64, 0, None) == L.GK_ERR_INVALID
    rc, err, page = call(c, 0, 64)                                               # an empty resident set: one empty, last page
    assert rc == L.GK_OK and page["entries"] == [] and page["next"] == 0 and page["total"] == 0 and page["n_chunks"] == 0
    assert list(c.AuditStreamFromCache()) == [] and list(c.AuditViolationMessages("t")) == []
    for i in range(70):                                                          # nobody violates: still one empty page; max_objects 0 counts as 64
        o = labelled("obj-%02d" % i, "default", set(), ["team"])
        c.AddData(o), oc.add_data(o)
    rc, err, page = call(c, 0, 0)
    assert rc == L.GK_OK and page["entries"] == [] and page["next"] == 0 and page["total"] == 0 and page["n_chunks"] == 1
    o = labelled("obj-69", "default", {"team"}, ["team"])                        # the last slot of the partial word
    c.AddData(o), oc.add_data(o)
    pages = stream(c, 1)
    assert [[e[0][-1] for e in p["entries"]] for p in pages] == [["obj-69"]] and pages[0]["n_chunks"] == 2
    check_stream(c, serial_loop(oc, c.cached), (1, 64))
