"""Rows a11 + f2: what an audit run writes into every constraint's status -- totalViolations and the `--constraint-violations-limit`
smallest violations in LimitQueue order (pkg/audit/manager.go:112-203, 885-941) -- for the RESIDENT set (auditFromCache's objects),
from one gk_resident_audit: the device counts the shown violators per constraint and chunk and picks the candidates in object-key order
(gk_audit_permute + gk_audit_select), the host merges the chunks, only the candidates are rendered.

Expected answers: the oracle client's serial loop over the cached objects (as tests/test_resident.py), every result fed to
oracle.audit.add_audit_responses / LimitQueue, compared as tests/test_parity.py::test_audit_aggregation compares AuditAggregate.

Equal object keys cannot be produced here (a live resident object's key is its inventory path): the tie rule and the overflow flag are
covered by tests/test_audit_merge.py on the CPU."""
import json

import pytest

from gatekeeper_amd import _lib as L
from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from oracle import audit as OA
from oracle import client as OC
from oracle import excluder as OX
from oracle import target as OT
from parity_util import BACKENDS, load_both, plan_group_max

RESIDENT_BACKENDS = [b for b in BACKENDS if b.id in ("hostemu", "gpu")]
STAMP = "2026-01-01T00:00:00Z"


def ckey(c):
    return (c.get("kind", ""), c.get("apiVersion", ""), (c.get("metadata") or {}).get("name", ""))


def serial_loop(oc, cached, hidden=None, memo=None, sig=None):
    """auditFromCache (manager.go:591-642): nsMap from the cached Namespaces, one Review per cached object that the audit process shows,
    with AugmentedUnstructured{obj, ns}.  -> [(Result, obj)], {constraint key: violating objects}.
    memo / sig: the oracle's answer is a function of the object, its Namespace and the policies.  With sig = text_sig a Review is run once
    per distinct (object, Namespace) text while the policies stay as they are; where a test's template reads nothing but the labels
    (label_sig), one Review per distinct label set is run and its results stand for every object that carries the same labels."""
    ns_map = {o["metadata"]["name"]: o for o in cached.values() if o.get("kind") == "Namespace" and o.get("apiVersion") == "v1"}
    results, pairs = [], {}
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
        for k in {ckey(r.constraint) for r in res}:
            pairs[k] = pairs.get(k, 0) + 1
    return results, pairs


def text_sig(o, ns):
    return json.dumps(o, sort_keys=True), json.dumps(ns, sort_keys=True)


def check(c, want, limits):
    """Client.AuditReportFromCache(limit) == the oracle's lists, totals and status for every limit; -> the last report"""
    results, pairs = want
    for limit in limits:
        got = c.AuditReportFromCache(limit=limit)
        lists, totals, per_action = {}, {}, {}
        OA.add_audit_responses(lists, totals, per_action, results, limit=limit)
        assert {k: v["total_pairs"] for k, v in got.items() if v["total_pairs"]} == pairs
        assert {k: v["total"] for k, v in got.items() if v["total"]} == totals
        assert got.totals_per_action == per_action and not got.errors
        assert set(got) == {ckey(k) for k in c.constraints.values()}
        for k, v in got.items():
            q = lists.get(k) or OA.LimitQueue(limit)
            assert v["violations"] == q.sorted(), (k, limit)
            st = got.constraint_status(k, STAMP, violations_limit=limit)
            assert st == OA.constraint_status(q, totals.get(k, 0), STAMP, violations_limit=limit), (k, limit)
        # only candidates were rendered: at most limit objects per constraint (no key ties here)
        assert got.n_rendered <= limit * len(got)
    return got


def pairs_agree(c, k=20):
    """gk_resident_audit's pair totals are gk_resident_sweep's for the same state"""
    a, s = c.driver.ResidentAudit(k), c.driver.ResidentSweep()
    assert a["pairs"] == s["pairs"] and a["n_objects"] == s["n_objects"] and a["n_chunks"] == s["n_chunks"] and a["beyond_limits"] == s["beyond_limits"]
    assert c.driver.ResidentAudit(k, result_totals=True)["results"] == c.driver.ResidentSweep(result_totals=True)["results"]
    return a


def shuffled(xs, seed):
    rng, xs = synth.SplitMix64(seed), list(xs)
    for i in range(len(xs) - 1, 0, -1):
        j = rng.below(i + 1)
        xs[i], xs[j] = xs[j], xs[i]
    return xs


# ------------------------------------------------------------------------------------------------ 1. parity, incremental
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_report_from_cache_incremental(backend, fixtures):
    c, oc = load_both(backend, synth.psp_templates(fixtures), synth.audit_constraints())
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(700, seed=23, mixed=True)
    for o in shuffled(list(nss.values()) + objs, 7):   # key order != slot order
        c.AddData(o), oc.add_data(o)
    memo = {}   # (the changed set below is reviewed again only where an object or its Namespace changed; the policies are the same)
    want = serial_loop(oc, c.cached, memo=memo, sig=text_sig)
    got = check(c, want, (20, 3, 1))
    assert sum(len(v["violations"]) for v in got.values()) > 10 and sum(v["total"] for v in got.values()) > sum(want[1].values()) > 100
    # (reviews without a Source: the two constraints that match on `source` answer with a match error per Pod -- autoreject results,
    #  which the audit counts and lists like any other)
    assert sum(1 for r, _ in want[0] if r.msg.startswith("unable to match constraints: ")) > 50
    assert pairs_agree(c)["n_chunks"] == 1
    # 7 pods change, two disappear, three appear: a second chunk, dead slots in the first
    rng = synth.SplitMix64(5)
    pods = [o for o in objs if o["kind"] == "Pod"]
    for k in range(7):
        o = json.loads(json.dumps(pods[rng.below(len(pods))]))
        o["spec"]["hostNetwork"] = True
        o["spec"]["containers"][0].setdefault("securityContext", {})["privileged"] = k % 2 == 0
        c.AddData(o), oc.add_data(o)
    for o in (pods[3], pods[11]):
        c.RemoveData(o), oc.remove_data(o)
    for o in synth.gen_objects(3, seed=99, start=5000):
        c.AddData(o), oc.add_data(o)
    want2 = serial_loop(oc, c.cached, memo=memo, sig=text_sig)
    check(c, want2, (20, 3, 1))
    assert pairs_agree(c)["n_chunks"] == 2 and want2[1] != want[1]
    # a constraint goes: its row goes, the others keep their lists
    k_ = synth.audit_constraints()[0]
    c.RemoveConstraint(k_), oc.remove_constraint(k_)
    got3 = check(c, serial_loop(oc, c.cached), (20, 3, 1))
    assert ckey(k_) not in got3 and len(got3) == len(synth.audit_constraints()) - 1
    pairs_agree(c)


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


def label_sig(o, ns=None):
    return tuple(sorted(o["metadata"]["labels"]))


def spread(count, below):
    """`count` distinct positions in [0, below), first and last included where count allows"""
    if count <= 0 or below <= 0:
        return set()
    return {0} if count == 1 else {(j * (below - 1)) // (count - 1) for j in range(count)}


def shape_patterns(n):
    """{constraint name: key positions that violate}: the shapes at which the two kernels can go wrong"""
    pats = {"none": set(), "all": set(range(n)), "first": {0}, "last": {n - 1}, "p63-p64": {p for p in (63, 64) if p < n}}
    for k in (1, 20):
        if n >= k:
            pats["exactly-%d" % k] = spread(k, n)
            pats["one-less-%d" % k] = spread(k - 1, n)
        for at in (63, 64, 4095, 4096):   # k + 1 violators, the k-th at position `at`: a word's last bit, the next word's first, ... of the second step
            if at + 1 < n and at >= k - 1:
                pats["kth-%d-at-%d" % (k, at)] = spread(k - 1, at) | {at, n - 1}
    return pats


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 4096, 4097, 4200])
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_shapes_where_the_kernels_can_go_wrong(backend, n):
    """one chunk of n objects; names obj-%05d inserted in REVERSE, so the key order is the slot order backwards; one constraint (= one
    bitmap row) per violation pattern; k = 1, 20 and beyond n.  n <= 130: the oracle reviews every object; beyond, one review per distinct
    label set (serial_loop), which n = 130 checks against the plain loop."""
    pats = shape_patterns(n)
    for name, pos in pats.items():
        assert all(0 <= p < n for p in pos), name
    for k in (1, 20):
        assert all(len(pats[x]) == k + 1 for x in pats if x.startswith("kth-%d-" % k))
        assert n < k or (len(pats["exactly-%d" % k]) == k and len(pats["one-less-%d" % k]) == k - 1)
    c, oc = load_both(backend, [tmpl("K8sNeedLabel", NEED_LABEL)], [need_label(x) for x in pats])
    for p in reversed(range(n)):
        o = labelled("obj-%05d" % p, "default", {x for x, pos in pats.items() if p in pos}, list(pats))
        c.AddData(o), oc.add_data(o)
    want = serial_loop(oc, c.cached, memo={}, sig=label_sig)
    if n <= 130:
        plain = serial_loop(oc, c.cached)
        assert plain[1] == want[1] and [(r.msg, ckey(r.constraint), o["metadata"]["name"]) for r, o in plain[0]] == [(r.msg, ckey(r.constraint), o["metadata"]["name"]) for r, o in want[0]]
    assert {k[2]: v for k, v in want[1].items()} == {x: len(pos) for x, pos in pats.items() if pos}
    check(c, want, (1, 20, n + 5))
    a = pairs_agree(c, 20)
    assert a["n_chunks"] == 1 and a["n_objects"] == n
    ids = {k["metadata"]["name"]: c.driver.constraint_id(k) for k in c.constraints.values()}
    for x, pos in pats.items():   # the device's own lists: exactly the 20 smallest positions, ascending, none flagged
        paths, overflow = a["lists"][ids[x]]
        assert not overflow and [p[-1] for p in paths] == ["obj-%05d" % p for p in sorted(pos)[:20]], x


# ------------------------------------------------------------------------------------------------ 3. masks
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_removed_replaced_and_excluded_objects_leave_the_lists(backend):
    c, oc = load_both(backend, [tmpl("K8sNeedLabel", NEED_LABEL)], [need_label("team")])
    objs = [labelled("obj-%03d" % i, "a-keep" if i < 15 else "a-skip", {"team"}, ["team"]) for i in range(20)]   # the twenty smallest keys: all violate
    objs += [labelled("obj-%03d" % i, "b-rest", {"team"} if i % 3 == 0 else set(), ["team"]) for i in range(20, 90)]
    for o in shuffled(objs, 3):
        c.AddData(o), oc.add_data(o)
    got = check(c, serial_loop(oc, c.cached), (20, 5))
    key = ckey(need_label("team"))
    assert [v["name"] for v in got[key]["violations"]] == ["obj-%03d" % i for i in range(5)]
    for o in objs[:10]:                      # half of them go
        c.RemoveData(o), oc.remove_data(o)
    for o in objs[10:15]:                    # a quarter is replaced by versions that carry the label
        fixed = labelled(o["metadata"]["name"], "a-keep", set(), ["team"])
        c.AddData(fixed), oc.add_data(fixed)
    entries = [{"excludedNamespaces": ["a-skip"], "processes": ["audit"]}]   # the rest is excluded from the audit process
    c.SetExcluder(entries)
    ox = OX.Excluder(entries)
    want = serial_loop(oc, c.cached, hidden=lambda o: ox.is_namespace_excluded("audit", o))
    got = check(c, want, (20, 5))
    assert [v["name"] for v in got[key]["violations"]][:2] == ["obj-021", "obj-024"] and got[key]["total_pairs"] == want[1][key] == 23
    pairs_agree(c)
    c.SetExcluder([])                        # the Config no longer excludes them: the five come back in front
    got = check(c, serial_loop(oc, c.cached), (20, 5))
    assert [v["name"] for v in got[key]["violations"]] == ["obj-%03d" % i for i in range(15, 20)] and got[key]["total_pairs"] == 28
    pairs_agree(c)


# ------------------------------------------------------------------------------------------------ 4. chunks
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_lists_merged_over_three_chunks(backend):
    names = ["every", "outer", "late"]
    c, oc = load_both(backend, [tmpl("K8sNeedLabel", NEED_LABEL)], [need_label(x) for x in names])
    # "every": the three smallest violators sit in three different chunks; "outer": chunk 2 has violators, all larger than the three
    # smallest of chunks 1 and 3; "late": chunk 2 has none at all
    waves = [[("obj-02", {"every", "outer"}), ("obj-05", {"outer"}), ("obj-10", {"every", "late"}), ("obj-11", set())],
             [("obj-01", {"every"}), ("obj-12", {"every", "outer"}), ("obj-13", {"outer"}), ("obj-14", set())],
             [("obj-03", {"every", "outer", "late"}), ("obj-04", {"late"}), ("obj-15", {"every", "late"})]]
    for i, wave in enumerate(waves):
        for name, violates in wave:
            o = labelled(name, "default", violates, names)
            c.AddData(o), oc.add_data(o)
        assert c.driver.ResidentSweep()["n_chunks"] == i + 1   # a sweep closes the chunk: the next additions open another
    got = check(c, serial_loop(oc, c.cached), (3, 1, 20))
    a = pairs_agree(c, 3)
    assert a["n_chunks"] == 3
    ids = {k["metadata"]["name"]: c.driver.constraint_id(k) for k in c.constraints.values()}
    assert {x: [p[-1] for p in a["lists"][ids[x]][0]] for x in names} == {"every": ["obj-01", "obj-02", "obj-03"], "outer": ["obj-02", "obj-03", "obj-05"],
                                                                        "late": ["obj-03", "obj-04", "obj-10"]}
    assert not any(a["lists"][ids[x]][1] for x in names)


# ------------------------------------------------------------------------------------------------ 6. plan groups
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_rows_of_further_plan_groups(backend, fixtures):
    with plan_group_max(L.load(hostemu=backend.startswith("hostemu")), 8):
        c, oc = load_both(backend, synth.psp_templates(fixtures), synth.psp_constraints())
        nss = synth.gen_namespaces()
        objs = synth.gen_objects(150, seed=41, mixed=True)
        for o in shuffled(list(nss.values()) + objs, 9):
            c.AddData(o), oc.add_data(o)
        want = serial_loop(oc, c.cached)
        got = check(c, want, (20, 2))
        pairs_agree(c)
        table = c.driver.engine.create_table([D.to_review_in(D.AugmentedUnstructured(D.Unstructured(objs[0]), None, ""))])
        try:
            assert table.eval().n_plan_groups == 4
        finally:
            table.free()
    assert len([k for k, v in got.items() if v["violations"]]) > 8   # rows of every group carry lists


# ------------------------------------------------------------------------------------------------ 7. edge calls
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_edge_calls(backend):
    c, oc = load_both(backend, [tmpl("K8sNeedLabel", NEED_LABEL)], [need_label("team"), need_label("owner")])
    lib = c.driver.engine.lib
    lib.gk_audit_free(None)
    ids = sorted(c.driver.constraint_id(k) for k in c.constraints.values())
    empty = c.driver.ResidentAudit(20, result_totals=True)   # an empty resident set
    assert empty["n_objects"] == 0 and empty["n_chunks"] == 0 and empty["pairs"] == {i: 0 for i in ids} == empty["results"]
    assert empty["lists"] == {i: ([], False) for i in ids}
    rep = c.AuditReportFromCache()
    assert all(v == {"total": 0, "total_pairs": 0, "violations": []} for v in rep.values()) and len(rep) == 2 and rep.totals_per_action == {}
    for i in range(70):
        o = labelled("obj-%02d" % i, "default", {"team"} if i % 2 else {"owner", "team"}, ["team", "owner"])
        c.AddData(o), oc.add_data(o)
    want = serial_loop(oc, c.cached)
    check(c, want, (20,))                                    # a call before any sweep brings the set up to date itself
    zero = c.driver.ResidentAudit(0)                         # k == 0: totals only
    assert zero["pairs"] == c.driver.ResidentSweep()["pairs"] and sorted(zero["pairs"].values()) == [35, 70]
    assert zero["lists"] == {i: ([], False) for i in ids} and zero["results"] is None
    rep0 = c.AuditReportFromCache(limit=0)
    assert sorted(v["total"] for v in rep0.values()) == [35, 70] and all(v["violations"] == [] for v in rep0.values())
    out = L.C.POINTER(L.gk_audit_out)()
    assert lib.gk_resident_audit(None, 20, 0, L.C.byref(out)) == L.GK_ERR_INVALID and lib.gk_resident_audit(c.driver.engine.handle, 20, 0, None) == L.GK_ERR_INVALID
