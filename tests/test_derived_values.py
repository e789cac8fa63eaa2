"""Derived value rows: a value COMPUTED from one review leaf compared with another review leaf, or with a value computed from another
leaf (`canon(c.resources.limits.cpu) > ratio * canon(c.resources.requests.cpu)`, `lower(mount.name) == lower(volume.name)`,
`to_number(annotations.max) < spec.replicas`).  pe.cpp compare_f names each computed side by a synthetic row beside its leaf,
<leaf>.$v<id>; the flattener writes the expression's value there (flatten.cpp Flattener::value_rows) and the row takes part in the
value ids and ranks like any leaf, so that the device relation is the integer compare of two ids it makes for two plain leaves.
Every case is compared with the oracle -- rendered results and raw device bitmaps -- on every backend.  Before this every
AddConstraint of section 1 raised "comparison between values derived from different review fields"."""
import os
import random
import re

import pytest

import value_order_util as U
from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from parity_util import BACKENDS, assert_parity, load_both, make_client, to_oracle_review

O = "input.review.object"


def raw(c, rv, **kw):
    table = c.driver.engine.create_table([D.to_review_in(r) for r in rv], keep_docs=False, **kw)
    try:
        return table.eval()
    finally:
        table.free()


def oracle_pairs_by_object(c, oc, objs, index):
    """{(constraint id, review)} of the oracle's violations for reviews[i] = objs[index[i]]: one Review per DISTINCT object"""
    ids = {(cons.get("kind"), cons["metadata"]["name"]): cid for cid, (cons, _, _) in c._active(D.AUDIT_EP).items()}
    per_obj = [{ids[(x.constraint["kind"], x.constraint["metadata"]["name"])] for x in oc.review(to_oracle_review(r), D.AUDIT_EP)} for r in U.reviews(objs)]
    return {(cid, i) for i, k in enumerate(index) for cid in per_obj[k]}


# ---------------------------------------------------------------------------------------------------------------- 1. library shapes
CANON = r'''
canon_cpu(x) = v { is_number(x); v := x * 1000 }
canon_cpu(x) = v { not is_number(x); endswith(x, "m"); v := to_number(replace(x, "m", "")) }
canon_cpu(x) = v { not is_number(x); not endswith(x, "m"); re_match("^[0-9]+(\\.[0-9]+)?$", x); v := to_number(x) * 1000 }
canon_mem(x) = v { is_number(x); v := x }
canon_mem(x) = v { not is_number(x); endswith(x, "Mi"); v := to_number(replace(x, "Mi", "")) * 1048576 }
canon_mem(x) = v { not is_number(x); endswith(x, "Gi"); v := to_number(replace(x, "Gi", "")) * 1073741824 }
input_containers[c] { c := input.review.object.spec.containers[_] }
input_containers[c] { c := input.review.object.spec.initContainers[_] }
'''
# (the bodies of canon() over one leaf are ONE value row a side -- pe.cpp merge_leaf_bodies -- so cpu and memory together take four of
#  the eight value slots an element scope has)
RATIO_REGO = "package k8scontainerratios\n" + CANON + '''
violation[{"msg": msg}] {
  c := input_containers[_]
  canon_cpu(c.resources.limits.cpu) > input.parameters.ratio * canon_cpu(c.resources.requests.cpu)
  msg := sprintf("container <%v> cpu limit <%v> is more than %v times its request <%v>", [c.name, c.resources.limits.cpu, input.parameters.ratio, c.resources.requests.cpu])
}
violation[{"msg": msg}] {
  c := input_containers[_]
  canon_mem(c.resources.limits.memory) > input.parameters.ratio * canon_mem(c.resources.requests.memory)
  msg := sprintf("container <%v> memory limit <%v> is more than %v times its request <%v>", [c.name, c.resources.limits.memory, input.parameters.ratio, c.resources.requests.memory])
}
'''
ABOVE_REGO = "package k8srequestabovelimit\n" + CANON + '''
violation[{"msg": msg}] {
  c := input.review.object.spec.containers[_]
  canon_cpu(c.resources.requests.cpu) > canon_cpu(c.resources.limits.cpu)
  msg := sprintf("container <%v> requests more cpu <%v> than its limit <%v>", [c.name, c.resources.requests.cpu, c.resources.limits.cpu])
}
'''
MOUNT_REGO = '''package k8smountwithoutvolume
has_volume(n) { lower(input.review.object.spec.volumes[_].name) == lower(n) }
violation[{"msg": msg}] {
  c := input.review.object.spec.containers[_]
  m := c.volumeMounts[_]
  not has_volume(m.name)
  msg := sprintf("container <%v> mounts <%v>, which is no volume of the pod", [c.name, m.name])
}
'''
MAX_REGO = '''package k8smaxreplicas
violation[{"msg": msg}] {
  o := input.review.object
  to_number(o.metadata.annotations.max) < o.spec.replicas
  msg := sprintf("%v replicas, the annotation allows %v", [o.spec.replicas, o.metadata.annotations.max])
}
'''
OWNER_REGO = '''package k8sownerlabel
violation[{"msg": "owner label and owner annotation differ"}] {
  m := input.review.object.metadata
  lower(m.labels.owner) != lower(m.annotations.owner)
}
'''
TWIN_REGO = '''package k8stwinnames
violation[{"msg": msg}] {
  cs := input.review.object.spec.containers
  a := cs[i]
  b := cs[j]
  i != j
  lower(a.name) == lower(b.name)
  msg := sprintf("container <%v> has a twin", [a.name])
}
'''


def params(kind, name=None, **p):
    k = U.cons(kind, name)
    k["spec"]["parameters"] = p
    return k


LIBRARY = {
    "ratio": ([U.tmpl("K8sContainerRatios", RATIO_REGO)], [params("K8sContainerRatios", ratio=4)]),
    "request-above-limit": ([U.tmpl("K8sRequestAboveLimit", ABOVE_REGO)], [U.cons("K8sRequestAboveLimit")]),
    "mount-without-volume": ([U.tmpl("K8sMountWithoutVolume", MOUNT_REGO)], [U.cons("K8sMountWithoutVolume")]),
    "max-annotation": ([U.tmpl("K8sMaxReplicas", MAX_REGO)], [U.cons("K8sMaxReplicas")]),
    "owner": ([U.tmpl("K8sOwnerLabel", OWNER_REGO)], [U.cons("K8sOwnerLabel")]),
    "twin-names": ([U.tmpl("K8sTwinNames", TWIN_REGO)], [U.cons("K8sTwinNames")]),
}
CPUS = ["100m", "500m", "2000m", 1, 2, 0.5, "1", "2", "0.25", "1.5", "abc", "", None, "250m"]
MEMS = ["64Mi", "128Mi", "1Gi", "2Gi", 1048576, 134217728, "1024Mi", "x", None, "0.5Gi"]
NAMES = ["data", "Data", "DATA", "cache", "Cache", "logs", "config-volume", "Config-Volume", "tmp"]


def library_objects(n=18, seed=11):
    """pods whose containers hold every spelling of a quantity, mounts and volumes that differ in case only, containers that do, owners
    and replica bounds as strings and numbers; every compared member now and then absent"""
    rng = random.Random(seed)
    objs = []
    for i in range(n):
        def container(ci):
            c = {"name": rng.choice(["app", "App", "sidecar", "init", "APP"]) if rng.random() < 0.5 else "c%d" % ci, "image": "i"}
            res = {}
            for side in ("limits", "requests"):
                for what, pool in (("cpu", CPUS), ("memory", MEMS)):
                    v = rng.choice(pool)
                    if v is not None:
                        res.setdefault(side, {})[what] = v
            if res:
                c["resources"] = res
            c["volumeMounts"] = [{"name": rng.choice(NAMES), "mountPath": "/m%d" % k} for k in range(rng.randrange(0, 3))]
            return c
        o = U.pod([container(ci) for ci in range(rng.randrange(0, 5))], "lib%d" % i, volumes=[{"name": rng.choice(NAMES)} for _ in range(rng.randrange(0, 4))])
        if rng.random() < 0.6:
            o["spec"]["initContainers"] = [container(9)]
        if rng.random() < 0.8:
            o["spec"]["replicas"] = rng.choice([1, 3, 5, 2.5, "4", 10])
        md = o["metadata"]
        if rng.random() < 0.8:
            md["labels"] = {"owner": rng.choice(["Team-A", "team-a", "TEAM-B", "platform-engineering", ""])}
        md["annotations"] = {}
        if rng.random() < 0.8:
            md["annotations"]["owner"] = rng.choice(["team-a", "Team-B", "Platform-Engineering", "", "x"])
        if rng.random() < 0.8:
            md["annotations"]["max"] = rng.choice(["3", "5", "2.5", "abc", "10", ""])
        objs.append(o)
    return objs


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", sorted(LIBRARY))
def test_library_shapes_load_and_agree_with_the_oracle(backend, shape, monkeypatch):
    monkeypatch.setenv("GK_RENDER_CHECK", "1")   # (both host evaluators render the messages; a difference is an error)
    c, oc = load_both(backend, *LIBRARY[shape])
    rv = U.reviews(library_objects())
    assert assert_parity(c, oc, rv) > 0
    ev = raw(c, rv)
    assert ev.host_evaluated == [] and not ev.too_big_reviews()


def test_ratio_by_hand():
    """the oracle is not the only witness: limit against 4 x request, every spelling of a cpu quantity"""
    c = make_client("hostemu")
    c.AddTemplate(LIBRARY["ratio"][0][0])
    c.AddConstraint(LIBRARY["ratio"][1][0])
    cases = [("500m", "100m", True), ("400m", "100m", False), (1, "250m", False), (1, "200m", True), ("2", 0.25, True), ("1", "0.25", False),
             ("abc", "1m", False), ("9", None, False), (None, "1m", False), ("1.5", "300m", True), (2, 0.5, False)]
    pods = []
    for i, (lim, req, _) in enumerate(cases):
        res = {}
        if lim is not None:
            res["limits"] = {"cpu": lim}
        if req is not None:
            res["requests"] = {"cpu": req}
        pods.append(U.pod([{"name": "c", "image": "i", "resources": res}], "h%d" % i))
    got = c.ReviewBatch(U.reviews(pods), D.AUDIT_EP)
    assert [len(g) == 1 for g in got] == [w for _, _, w in cases]
    assert got[0][0].msg == "container <c> cpu limit <500m> is more than 4 times its request <100m>"


# ---------------------------------------------------------------------------------------------------------------- 2. relations
RELS = {"Eq": "==", "Ne": "!=", "Lt": "<", "Le": "<=", "Gt": ">", "Ge": ">="}
FAMILIES = {   # name -> (bindings, left, right, message)
    "Num": ("", "to_number(s.a)", "to_number(s.b)", '"m"'),
    "Mix": ("", "to_number(s.a)", "lower(s.b)", '"m"'),
    "Plain": ("", "lower(s.a)", "s.b", '"m"'),
    "Elem": ("c := s.containers[_]\n  ", "lower(c.name)", "lower(s.owner)", 'sprintf("%v", [c.name])'),
}
NEGATED = ("Num", "Elem")   # `not <left> <rel> <right>`, all six relations


def relation_policy():
    templates, constraints = [], []
    for fam, (bind, left, right, msg) in FAMILIES.items():
        for r, op in RELS.items():
            variants = [("", "")] + ([("Not", "not ")] if fam in NEGATED else [])
            for tag, neg in variants:
                kind = "K8sDv%s%s%s" % (fam, tag, r)
                rego = 'package k\nviolation[{"msg": msg}] {\n  s := %s.spec\n  %s%s%s %s %s\n  msg := %s\n}\n' % (O, bind, neg, left, op, right, msg)
                templates.append(U.tmpl(kind, rego))
                constraints.append(U.cons(kind))
    # a derived value that is a non-empty ARRAY: no id can stand for it, the review is the host evaluator's
    templates.append(U.tmpl("K8sDvSplit", 'package k\nviolation[{"msg": "m"}] {\n  s := %s.spec\n  split(s.list, ",") != s.b\n}\n' % O))
    constraints.append(U.cons("K8sDvSplit"))
    return templates, constraints


LONG = 123456789012345678901234567890   # (no int64 and no double holds it)


def spec_pod(name, **spec):
    return U.pod(spec.pop("containers", []), name, **spec)


def names(n):
    return [{"name": "c%d" % i, "image": "i"} for i in range(n)]


# name -> spec members.  `a` / `b` feed Num, Mix and Plain; `containers` and `owner` feed Elem; `list` feeds the split
HANDCRAFTED = [
    ("no-a", dict(b="1")), ("no-b", dict(a="1")), ("neither", dict()),
    ("a-error", dict(a="abc", b="1")), ("b-error", dict(a="1", b="abc")), ("both-error", dict(a="abc", b="abc")),
    ("one-int-str", dict(a=1, b="1")), ("one-float-str", dict(a=1.0, b="1")), ("one-str-int", dict(a="1", b=1)), ("one-strfloat-int", dict(a="1.0", b=1)),
    ("one-str-str", dict(a="1", b="1.0")), ("two-ten", dict(a="2", b="10")), ("ten-two", dict(a="10", b="2")), ("neg", dict(a="-1", b="-2")),
    ("frac", dict(a="1.5", b="1")), ("exp", dict(a="1e3", b="1000")), ("num-num", dict(a=7, b=7.5)),
    ("empty-empty", dict(a="", b="")), ("empty-a", dict(a="", b="a")), ("a-empty", dict(a="a", b="")),
    ("long-equal", dict(a="ABCDEFGHIJ", b="abcdefghij")), ("long-last-byte", dict(a="ABCDEFGHIJ", b="abcdefghii")), ("short-long", dict(a="ABC", b="abcdefgh")),
    ("inline-7", dict(a="ABCDEFG", b="abcdefg")), ("heap-8", dict(a="ABCDEFGH", b="abcdefgh")),
    ("derived-meets-leaf", dict(a="ABC", b="abc", owner="abc", containers=[{"name": "ABC", "image": "i"}, {"name": "abd", "image": "i"}])),
    ("bool-b", dict(a="true", b=True)), ("false-b", dict(a="x", b=False)), ("null-b", dict(a="x", b=None)), ("bool-a", dict(a=True, b="true")),
    ("null-a", dict(a="x", b="x", owner="C1", containers=names(3))), ("empty-array-b", dict(a="x", b=[])), ("empty-object-a", dict(a={}, b="x")),
    ("upper-owner", dict(owner="C2", containers=names(4))), ("owner-absent", dict(containers=names(2))), ("owner-number", dict(owner=5, containers=names(2))),
    ("name-number", dict(owner="c1", containers=[{"name": 3, "image": "i"}, {"name": "C1", "image": "i"}, {"image": "i"}])),
    ("seventeen", dict(a="2", b="3", owner="C16", containers=names(17))),
    ("many", dict(a="2", b="3", owner="c255", containers=names(256))),
    ("inexact-a", dict(a=str(LONG), b="1")), ("inexact-b-plain", dict(a="x", b=LONG)), ("array-b", dict(a="x", b=[1])), ("array-a", dict(a=[1, 2], b="x")),
    ("split", dict(list="x,y", b="x")),
]
# what no value id can stand for: the host evaluator answers, and says so
HOST = ["many", "inexact-a", "inexact-b-plain", "array-b", "array-a", "split"]


def handcrafted_objects():
    return [spec_pod(name, **dict(spec)) for name, spec in HANDCRAFTED]


@pytest.mark.parametrize("backend", BACKENDS)
def test_six_relations_and_not_over_handcrafted_objects(backend):
    c, oc = load_both(backend, *relation_policy())
    objs = handcrafted_objects()
    rv = U.reviews(objs)
    assert assert_parity(c, oc, rv) > 300
    ev = raw(c, rv)
    assert not ev.too_big_reviews()
    assert [HANDCRAFTED[i][0] for i in ev.host_evaluated] == HOST          # nothing else leaves the device, nothing is refused
    assert ev.n_overflow >= 1                                               # the 17 containers took the large variant
    # by hand: a number is below every string, whatever they spell
    got = c.ReviewBatch(rv, D.AUDIT_EP)
    kinds = lambda name: sorted(r.constraint["kind"] for r in got[[n for n, _ in HANDCRAFTED].index(name)])
    assert [k for k in kinds("two-ten") if k.startswith("K8sDvMix")] == ["K8sDvMixLe", "K8sDvMixLt", "K8sDvMixNe"]
    assert [k for k in kinds("two-ten") if k.startswith("K8sDvNum") and "Not" not in k] == ["K8sDvNumLe", "K8sDvNumLt", "K8sDvNumNe"]
    assert [k for k in kinds("one-strfloat-int") if k.startswith("K8sDvNum") and "Not" not in k] == ["K8sDvNumEq", "K8sDvNumGe", "K8sDvNumLe"]
    assert [k for k in kinds("a-error") if k.startswith("K8sDvNum")] == ["K8sDvNumNot" + r for r in sorted(RELS)]   # undefined: every relation false, every `not` true
    assert [k for k in kinds("long-equal") if k.startswith("K8sDvPlain")] == ["K8sDvPlainEq", "K8sDvPlainGe", "K8sDvPlainLe"]


# ---------------------------------------------------------------------------------------------------------------- 3. geometries
GEOM_FAMILIES = ("Num", "Elem")


def geometry_policy():
    t, k = relation_policy()
    keep = [i for i, x in enumerate(k) if x["kind"].startswith(tuple("K8sDv" + f for f in GEOM_FAMILIES))]
    return [t[i] for i in keep], [k[i] for i in keep]


def device_objects():
    """the handcrafted objects the device answers (the host evaluator's are section 2's)"""
    return [o for (name, _), o in zip(HANDCRAFTED, handcrafted_objects()) if name not in HOST]


@pytest.mark.parametrize("backend", BACKENDS)
def test_admission_batch_of_65(backend):
    """64-review groups, the second one review long"""
    c, oc = load_both(backend, *geometry_policy())
    objs = device_objects()
    index = [i % len(objs) for i in range(65)]
    rv = U.reviews([objs[k] for k in index])
    ev = raw(c, rv)
    assert ev.n_tiles == 2 and ev.host_evaluated == [] and not ev.too_big_reviews()
    assert set(ev.pairs("viol")) == oracle_pairs_by_object(c, oc, objs, index) and ev.pairs("err") == []
    got = c.ReviewBatch(rv, D.AUDIT_EP)
    for g, k in zip(got, index):
        assert sorted(r.msg for r in g) == sorted(r.msg for r in oc.review(to_oracle_review(U.reviews([objs[k]])[0]), D.AUDIT_EP))


@pytest.mark.parametrize("backend", BACKENDS)
def test_sweep_table_of_8257(backend, monkeypatch):
    """32 full 256-review groups and a tail of 65: the last bitmap word holds one review.  Every bit of every constraint against the
    oracle, which is asked once per distinct object; on the device the plan-specialised kernel is checked against the bytecode kernel too"""
    monkeypatch.setenv("GK_RPT", "256")   # (what a table of 8192 reviews and more gets by itself while its policy set is one plan group)
    c, oc = load_both(backend, *geometry_policy())
    objs = device_objects()
    n = 8257
    index = [i % len(objs) for i in range(n)]
    table = c.driver.engine.create_table([D.to_review_in(r) for r in U.reviews([objs[k] for k in index])], keep_docs=False, resident=True)
    try:
        ev = table.eval()
        assert ev.n_tiles == 130 and ev.n_reviews == n and ev.host_evaluated == [] and not ev.too_big_reviews()
        want = oracle_pairs_by_object(c, oc, objs, index)
        assert set(ev.pairs("viol")) == want and len(want) > n and ev.pairs("err") == []
        if backend == "gpu":
            v = c.driver.VerifyTable(table)
            assert v.diff_total == 0 and v.diff_too_big == 0 and v.specialised_groups >= 1
    finally:
        table.free()


# ---------------------------------------------------------------------------------------------------------------- 4. ingest paths
def _digest(eng, rins, **env):
    os.environ["GK_TABLE_DIGEST"] = "1"
    for k, v in env.items():
        os.environ[k] = v
    try:
        t = eng.create_table(rins, keep_docs=False)
        try:
            ev = t.eval()
            return t.stats()["digest"], (ev.viol.tobytes(), ev.err.tobytes(), ev.too_big.tobytes(), tuple(ev.host_evaluated))
        finally:
            t.free()
    finally:
        for k in list(env) + ["GK_TABLE_DIGEST"]:
            os.environ.pop(k, None)


@pytest.mark.parametrize("backend", [b for b in BACKENDS if b.id in ("hostemu", "gpu")])
def test_ingest_paths_build_one_table(backend):
    """the one-pass parser over the structural index, the byte-at-a-time scanner, the general path and a pruned table: one digest for
    the three full tables, and the same words from all four (a pruned table holds fewer rows: its digest is its own)"""
    c, oc = load_both(backend, *relation_policy())
    objs = handcrafted_objects() + library_objects(6)
    rins = [D.to_review_in(r) for r in U.reviews(objs)]
    eng = c.driver.engine
    index = _digest(eng, rins)
    scan = _digest(eng, rins, GK_NO_INDEX="1")
    general = _digest(eng, rins, GK_SLOW_INGEST="1")
    pruned = _digest(eng, rins, GK_FORCE_PRUNE="1")
    assert index[0] != 0 and index[0] == scan[0] == general[0]
    assert index[1] == scan[1] == general[1] == pruned[1]
    assert any(index[1][0])


@pytest.mark.parametrize("backend", [b for b in BACKENDS if b.id in ("hostemu", "gpu")])
def test_admission_requests_and_the_namespace_document(backend):
    """AdmissionRequest documents (object and oldObject go through add_json_request) and a value derived from the review's Namespace
    (the $ns rows, replayed from the first review of a namespace where that is possible)"""
    rego = '''package k
violation[{"msg": "grew"}] {
  to_number(input.review.object.metadata.annotations.max) > to_number(input.review.oldObject.metadata.annotations.max)
}
violation[{"msg": "foreign owner"}] {
  lower(input.review.object.metadata.labels.owner) != lower(input.review.namespaceObject.metadata.labels.owner)
}
'''
    c, oc = load_both(backend, [U.tmpl("K8sDvRequest", rego)], [U.cons("K8sDvRequest")])
    objs = library_objects(14, seed=5)
    ns = {"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": "default", "labels": {"owner": "TEAM-A"}}}
    rv = []
    for i, o in enumerate(objs):
        r = {"uid": "u%d" % i, "kind": {"group": "", "version": "v1", "kind": "Pod"}, "operation": "UPDATE", "name": o["metadata"]["name"], "namespace": "default",
             "object": o, "oldObject": dict(objs[(i + 1) % len(objs)], metadata=dict(objs[(i + 1) % len(objs)]["metadata"], name=o["metadata"]["name"]))}
        rv.append(D.AugmentedReview(D.AdmissionRequest(r), ns, "Original"))
    assert assert_parity(c, oc, rv, D.GATOR_EP, namespaces=[ns] * len(rv)) > 4


# ---------------------------------------------------------------------------------------------------------------- 5. life cycle
def _plan_text_and_digest(client, drv, out_dir, n=1024):
    """tests/test_numeric_index.py::_configs2_text, plus the GK_TABLE_DIGEST of the table it sweeps"""
    for f in os.listdir(str(out_dir)):
        os.remove(os.path.join(str(out_dir), f))
    batch = synth.NativeBatch(drv.engine.lib, n, seed=synth.SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
    os.environ["GK_TABLE_DIGEST"] = "1"
    try:
        table = drv.engine.create_table_native(batch.reviews, n, keep_docs=False, resident=True)
        digest = table.stats()["digest"]
    finally:
        os.environ.pop("GK_TABLE_DIGEST", None)
    table.launch()
    table.eval(download=True, collect_only=True)
    table.free()
    return sorted(open(os.path.join(str(out_dir), f)).read() for f in os.listdir(str(out_dir)) if f.startswith("gk_plan_")), digest


def value_expression_lines(client):
    text = client.Dump()
    return text.split("value expressions:\n", 1)[1].splitlines() if "value expressions:\n" in text else []


def test_policy_set_is_what_it_was_once_the_constraint_has_gone(monkeypatch, tmp_path):
    """configs[2]'s policy, then the ratio constraints and the owner join added and removed: the plan text and the tables that remain
    are byte for byte those of before, and the dump lists the value expressions while they are loaded"""
    import test_self_join_plan_text as PT
    monkeypatch.setenv("GK_HOSTEMU_KERNEL", "jit")
    monkeypatch.setenv("GK_EMU_HIP_SOURCE_DIR", str(tmp_path))
    monkeypatch.setenv("GK_EMU_GRID", "8")
    drv = D.Driver(device=0, hostemu=True)
    client = D.Client(drv)
    templates, constraints = PT._policy(2, synth.load_fixtures())
    for t in templates:
        client.AddTemplate(t)
    for k in constraints:
        client.AddConstraint(k)
    before = _plan_text_and_digest(client, drv, tmp_path)
    assert before[0] and before[1] != 0 and value_expression_lines(client) == []
    added = [LIBRARY["ratio"], LIBRARY["owner"]]
    for ts, ks in added:
        for t in ts:
            client.AddTemplate(t)
        for k in ks:
            client.AddConstraint(k)
    lines = value_expression_lines(client)
    # (cpu and memory, limit and request, `containers` and `initContainers`: the three bodies of a canon() are one expression; two owners)
    assert len(lines) == 8 + 2 and all(re.fullmatch(r"review\.object\.\S+ \$v[0-9a-f]+ = .+", x) for x in lines), lines
    assert sum(1 for x in lines if x.endswith(" ordered")) == 8 and sum(1 for x in lines if " = lower($)" in x) == 2
    assert sum(1 for x in lines if "$pick(" in x and "initContainers[].resources.requests.memory" in x) == 1
    with_values = _plan_text_and_digest(client, drv, tmp_path)
    assert with_values[0] != before[0] and with_values[1] != before[1]
    ts, ks = added[0]
    client.RemoveConstraint(ks[0])
    assert len(value_expression_lines(client)) == 2                 # the owner join keeps its two
    client.RemoveTemplate(added[1][0][0])                           # (the template takes its constraint along)
    client.RemoveTemplate(ts[0])
    assert value_expression_lines(client) == []
    assert _plan_text_and_digest(client, drv, tmp_path) == before


@pytest.mark.parametrize("backend", [b for b in BACKENDS if b.id in ("hostemu", "gpu")])
def test_a_table_created_before_the_constraint_is_stale(backend):
    c, oc = load_both(backend, *LIBRARY["mount-without-volume"])
    objs = library_objects(8)
    rv = U.reviews(objs)
    old = c.driver.engine.create_table([D.to_review_in(r) for r in rv], keep_docs=False)
    old.eval()
    for t, k in zip(*LIBRARY["owner"]):
        c.AddTemplate(t), oc.add_template(t)
        c.AddConstraint(k), oc.add_constraint(k)
    with pytest.raises(D.EngineError, match="create it again"):
        old.eval()
    old.free()
    for r in rv:   # Client.Review after the policy change: the caller re-creates nothing
        assert sorted(x.msg for x in c.Review(r, D.AUDIT_EP)) == sorted(x.msg for x in oc.review(to_oracle_review(r), D.AUDIT_EP))
    assert assert_parity(c, oc, rv) > 0


def test_two_constraints_with_one_derivation_share_its_row():
    """the same derivation of the same leaf in two templates: one expression in the dump, one row per leaf in the table"""
    other = 'package k\nviolation[{"msg": "shouting"}] {\n  m := %s.metadata\n  lower(m.labels.owner) < upper(m.annotations.owner)\n}\n' % O
    objs = [o for o in library_objects(12) if "labels" in o["metadata"]]

    def rows(templates, constraints):
        c = make_client("hostemu")
        for t in templates:
            c.AddTemplate(t)
        for k in constraints:
            c.AddConstraint(k)
        t = c.driver.engine.create_table([D.to_review_in(r) for r in U.reviews(objs)], keep_docs=False)
        try:
            return t.stats()["n_rows"], value_expression_lines(c)
        finally:
            t.free()
    none = rows([], [])[0]
    one, lines1 = rows(*LIBRARY["owner"])
    two, lines2 = rows(LIBRARY["owner"][0] + [U.tmpl("K8sShout", other)], LIBRARY["owner"][1] + [U.cons("K8sShout")])
    n_label = len(objs)
    n_ann = sum(1 for o in objs if "owner" in o["metadata"]["annotations"])
    assert one - none == 2 * (n_label + n_ann) and len(lines1) == 2   # per leaf: its value row, and the dictionary row that says lower() is defined
    assert len(lines2) == 3 and two - one == n_ann                  # only upper(annotations.owner) is new: lower(labels.owner) is shared
    assert sum(1 for x in lines2 if "labels.owner" in x) == 1


# ---------------------------------------------------------------------------------------------------------------- 6. totals, resident set
def audit_policy():
    t, k = [], []
    for shape in ("ratio", "mount-without-volume", "owner", "twin-names"):
        t += LIBRARY[shape][0]
        k += LIBRARY[shape][1]
    return t, k


@pytest.mark.parametrize("backend", [b for b in BACKENDS if b.id in ("hostemu", "gpu")])
def test_result_totals_and_the_resident_set(backend):
    """AuditAggregate's totals are RESULT counts (a pod with two offending containers counts twice), and the resident set reports the
    same totals and lists for the same objects once they are synced"""
    import test_resident_audit as RA
    from oracle import audit as OA
    c, oc = load_both(backend, *audit_policy())
    objs = library_objects(24, seed=3)
    rv = U.reviews(objs)
    got = c.AuditAggregate(rv, limit=20)
    lists, totals, per_action, pairs = {}, {}, {}, {}
    for o, r in zip(objs, rv):
        res = oc.review(to_oracle_review(r), D.AUDIT_EP, None)
        OA.add_audit_responses(lists, totals, per_action, [(x, o) for x in res], limit=20)
        for k in {RA.ckey(x.constraint) for x in res}:
            pairs[k] = pairs.get(k, 0) + 1
    assert {k: v["total"] for k, v in got.items() if v["total"]} == totals and sum(totals.values()) > sum(pairs.values()) > 0
    assert {k: v["total_pairs"] for k, v in got.items() if v["total_pairs"]} == pairs and got.totals_per_action == per_action and not got.errors
    for k, q in lists.items():
        assert got[k]["violations"] == q.sorted(), k
    for o in objs:
        c.AddData(o), oc.add_data(o)
    rep = RA.check(c, RA.serial_loop(oc, c.cached), (20, 3))
    assert {k: v["total"] for k, v in rep.items() if v["total"]} == totals


# ---------------------------------------------------------------------------------------------------------------- 7. refusals that remain
REFUSED = {
    "arithmetic between two fields": ("s.a - s.b < 3", r"arithmetic '-' on review data"),
    "sizes of two containers": ("count(s.a) < count(s.b)", "comparison between these symbolic operands"),
    "a key against a derived value": ("some k\n  %s.metadata.labels[k]\n  k == lower(s.b)" % O, "comparison between values derived from different review fields"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_that_remain(case):
    body, text = REFUSED[case]
    c = make_client("hostemu")
    c.AddTemplate(U.tmpl("K8sRefused", 'package k\nviolation[{"msg": "m"}] {\n  s := %s.spec\n  %s\n}\n' % (O, body)))
    with pytest.raises(D.UnsupportedError, match="unsupported on the device plan: " + text):
        c.AddConstraint(U.cons("K8sRefused"))


# ---------------------------------------------------------------------------------------------------------------- 8. differential fuzz
LEAVES = {   # name -> (bindings, term); a and b are root leaves, the others elements of two arrays
    "a": ((), "s.a"), "b": ((), "s.b"), "owner": ((), "s.owner"),
    "cx": (("c",), "c.x"), "cy": (("c",), "c.y"), "vx": (("v",), "v.x"), "vy": (("v",), "v.y"),
}
BIND = {"c": "c := s.containers[_]", "v": "v := s.volumes[_]"}
DERIVE = {
    "identity": "%s", "lower": "lower(%s)", "upper": "upper(%s)", "trim": 'trim(%s, " ")', "to_number": "to_number(%s)",
    "to_number-replace": 'to_number(replace(%s, "m", ""))', "times": "%s * 3", "plus": "%s + 2", "sprintf": 'sprintf("%%v", [%s])',
}
FUZZ_POOL = ["1", "2", " 2", "10", "10m", "250m", "ABC", "abc", " abc ", "abcdefgh", "ABCDEFGH", "abcdefghij", "", 1, 2, 2.5, 10, -1, 0, 30, True, None, "3", "-1"]


def fuzz_template(rng, kind):
    la, lb = rng.sample(sorted(LEAVES), 2)
    da, db = rng.choice(sorted(DERIVE)), rng.choice(sorted(DERIVE))
    if da == "identity" and db == "identity":
        da = rng.choice(sorted(set(DERIVE) - {"identity"}))   # (two plain leaves are what tests/test_value_order.py fuzzes)
    op = rng.choice(sorted(RELS.values()))
    neg = rng.random() < 0.3
    lines = [BIND[v] for v in ("c", "v") if v in LEAVES[la][0] + LEAVES[lb][0]]
    lines.append("%s%s %s %s" % ("not " if neg else "", DERIVE[da] % LEAVES[la][1], op, DERIVE[db] % LEAVES[lb][1]))
    return U.tmpl(kind, 'package k\nviolation[{"msg": "m"}] {\n  s := %s.spec\n  %s\n}\n' % (O, "\n  ".join(lines)))


def fuzz_object(rng, name):
    def pick(d, k):
        if rng.random() < 0.85:
            d[k] = rng.choice(FUZZ_POOL)
    spec = {}
    for k in ("a", "b", "owner"):
        pick(spec, k)
    for arr in ("containers", "volumes"):
        items = []
        for i in range(rng.randrange(0, 4)):
            e = {"name": "%s%d" % (arr[0], i), "image": "i"}
            pick(e, "x"), pick(e, "y")
            items.append(e)
        spec[arr] = items
    return U.pod(spec.pop("containers"), name, **spec)


FUZZ_SEED, FUZZ_TEMPLATES, FUZZ_OBJECTS = 20261, 24, 48


def test_fuzz_generator_draws_every_derivation_and_relation():
    rng = random.Random(FUZZ_SEED)
    texts = [fuzz_template(rng, "K8sF")["spec"]["targets"][0]["rego"] for _ in range(FUZZ_TEMPLATES)]
    assert all(any(op in t for t in texts) for op in (" == ", " != ", " < ", " <= ", " > ", " >= ")) and any("not " in t for t in texts)
    assert all(any(w in t for t in texts) for w in ("lower(", "upper(", "trim(", "to_number(", "replace(", " * 3", " + 2", "sprintf(")) and any("c := " in t and "v := " in t for t in texts)


@pytest.mark.parametrize("backend", BACKENDS)
def test_differential_fuzz(backend):
    """24 templates x 48 objects from one seed; every template must be accepted (AddConstraint raises otherwise), every object's
    messages and every raw bit equal the oracle's, and nothing here needs the host evaluator"""
    rng = random.Random(FUZZ_SEED)
    templates, constraints = [], []
    for k in range(FUZZ_TEMPLATES):
        templates.append(fuzz_template(rng, "K8sFuzzDv%d" % k))
        constraints.append(U.cons("K8sFuzzDv%d" % k))
    objs = [fuzz_object(rng, "f%d" % i) for i in range(FUZZ_OBJECTS)]
    c, oc = load_both(backend, templates, constraints)
    rv = U.reviews(objs)
    assert assert_parity(c, oc, rv) > 200
    ev = raw(c, rv)
    assert ev.host_evaluated == [] and not ev.too_big_reviews()
