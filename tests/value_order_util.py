"""Shared by test_value_order.py: the templates, objects and value pool of the ordering tests (`a < b` between two review values,
cursors.hpp F_VCMP), and -- run as a script in a process of its own, because the row-group geometry (GK_RPT) and the generator's A/B
switches (GK_JIT_JOIN, GK_JIT_DNF) are read once per process --
usage: value_order_util.py geom <backend>    every layout's templates plus a body that mixes an equality join with an ordering literal in
                                             ONE plan, against the oracle (parity_util.assert_parity); prints the violation count and the
                                             SHA-256 of the raw violation / error / too_big words
backend: hostemu (with GK_HOSTEMU_KERNEL=jit: the emulated plan-specialised kernel, checked against the interpreter word by word) or gpu."""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gatekeeper_amd import driver as D   # noqa: E402

RELS = {"Lt": "<", "Le": "<=", "Gt": ">", "Ge": ">="}


def tmpl(kind, rego):
    return {"apiVersion": "templates.gatekeeper.sh/v1", "kind": "ConstraintTemplate", "metadata": {"name": kind.lower()},
            "spec": {"crd": {"spec": {"names": {"kind": kind}}}, "targets": [{"target": "admission.k8s.gatekeeper.sh", "rego": rego}]}}


def cons(kind, name=None):
    return {"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": kind, "metadata": {"name": name or "c-" + kind.lower()}, "spec": {}}


# one rule body per slot layout, `%s` = the relation
LAYOUTS = {
    # two root-scope values
    "RootRoot": '''violation[{"msg": msg}] {
  s := input.review.object.spec
  s.minReplicas %s s.maxReplicas
  msg := sprintf("min %%v max %%v", [s.minReplicas, s.maxReplicas])
}''',
    # an element's value against a root-scope value
    "ElemRoot": '''violation[{"msg": msg}] {
  c := input.review.object.spec.containers[_]
  c.resources.limits.count %s input.review.object.spec.maxCount
  msg := sprintf("container %%v", [c.name])
}''',
    # two members of one element: two slots, an unpacked scope
    "TwoMembers": '''violation[{"msg": msg}] {
  p := input.review.object.spec.containers[_].ports[_]
  p.containerPort %s p.hostPort
  msg := sprintf("port %%v host %%v", [p.containerPort, p.hostPort])
}''',
    # one member (a packed scope) against the element of an enclosing loop (packed as well): the volumeMounts x volumes shape
    "PackedOuter": '''violation[{"msg": msg}] {
  v := input.review.object.spec.volumes[_]
  p := input.review.object.spec.containers[_].ports[_]
  p.containerPort %s v.port
  msg := sprintf("port %%v volume %%v", [p.containerPort, v.name])
}''',
    # object against oldObject
    "OldNew": '''violation[{"msg": "replicas"}] {
  input.review.object.spec.replicas %s input.review.oldObject.spec.replicas
}''',
    # a self-join under alias cursors
    "SelfJoin": '''violation[{"msg": msg}] {
  c := input.review.object.spec.containers
  p1 := c[i].ports[_]
  p2 := c[j].ports[_]
  i != j
  p1.containerPort %s p2.containerPort
  msg := sprintf("%%v against %%v", [c[i].name, c[j].name])
}''',
    # the negated literal: true when a side is absent
    "Negated": '''violation[{"msg": "not"}] {
  s := input.review.object.spec
  not s.minReplicas %s s.maxReplicas
}''',
}
# an equality join and an ordering literal in one loop body: the general form, never the join form's xor
MIXED = '''violation[{"msg": msg}] {
  v := input.review.object.spec.volumes[_]
  c := input.review.object.spec.containers[_]
  p := c.ports[_]
  p.name == v.name
  p.containerPort %s v.port
  msg := sprintf("port %%v of %%v volume %%v", [p.containerPort, c.name, v.name])
}'''


def layout_templates(layout, body=None):
    """the four relations of one layout: four templates, one plan (the relations share the layout's value slots)"""
    return [tmpl("K8sOrd%s%s" % (layout, r), "package k\n" + (body or LAYOUTS[layout]) % op) for r, op in RELS.items()]


def layout_constraints(layout):
    return [cons("K8sOrd%s%s" % (layout, r)) for r in RELS]


# values chosen to break an id that is not a rank: numbers against their float spellings, strings that look like numbers, booleans
# and null, negative numbers, heap strings (> 7 bytes) that differ in their last byte, an inline string that is a prefix of a heap
# string.  No container and no inexact number: nothing here may need the host.
POOL = [5, 3, 3.0, 2.5, 1, 1.5, 2, "10", 9, "9", True, False, None, -1, -2, -2.5, 0, "", "abc", "abcdefg", "abcdefgh", "abcdefghij", "abcdefghii", "z"]


def pod(containers, name="p", **spec_extra):
    spec = {"containers": containers}
    spec.update(spec_extra)
    return {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": name, "namespace": "default"}, "spec": spec}


def random_pod(rng, name, pool=POOL):
    """at most four containers of at most three ports, at most three volumes, every compared member now and then absent"""
    def pick(d, k):
        if rng.random() < 0.85:
            d[k] = rng.choice(pool)
    cs = []
    for ci in range(rng.randrange(0, 5)):
        c = {"name": "c%d" % ci, "image": "i"}
        lim = {}
        pick(lim, "count")
        if rng.random() < 0.9:
            c["resources"] = {"limits": lim}
        ports = []
        for pi in range(rng.randrange(0, 4)):
            p = {"name": rng.choice(["a", "b", "vol-long-name"])}
            pick(p, "containerPort")
            pick(p, "hostPort")
            ports.append(p)
        if ports or rng.random() < 0.5:
            c["ports"] = ports
        cs.append(c)
    extra = {}
    for k in ("minReplicas", "maxReplicas", "maxCount", "replicas"):
        pick(extra, k)
    vols = []
    for vi in range(rng.randrange(0, 4)):
        v = {"name": rng.choice(["a", "b", "vol-long-name"])}
        pick(v, "port")
        vols.append(v)
    extra["volumes"] = vols
    return pod(cs, name, **extra)


def first_occurrence_pod():
    """the LARGER value occurs first in the document on every compared pair: ids in order of first occurrence would answer the opposite"""
    return pod([{"name": "c0", "image": "i", "resources": {"limits": {"count": 9}},
                 "ports": [{"name": "a", "containerPort": 9000, "hostPort": 80}, {"name": "b", "containerPort": "zz", "hostPort": "aa"}]},
                {"name": "c1", "image": "i", "resources": {"limits": {"count": 2}}, "ports": [{"name": "a", "containerPort": 70, "hostPort": 8000}]}],
               "first", minReplicas=7, maxReplicas=4, maxCount=5, replicas=3, volumes=[{"name": "a", "port": 100}, {"name": "b", "port": 60}])


def layout_objects(seed=1, n=10):
    rng = random.Random(seed)
    return [first_occurrence_pod()] + [random_pod(rng, "r%d" % i) for i in range(n)]


def reviews(objs):
    return [D.AugmentedUnstructured(D.Unstructured(o), None, "Original") for o in objs]


def update_reviews(objs):
    """AdmissionRequest UPDATEs: each object against the next one as its oldObject (the last one has none: CREATE)"""
    out = []
    for i, o in enumerate(objs):
        r = {"uid": "u%d" % i, "kind": {"group": "", "version": "v1", "kind": "Pod"}, "operation": "UPDATE" if i + 1 < len(objs) else "CREATE",
             "name": o["metadata"]["name"], "namespace": "default", "object": o}
        if i + 1 < len(objs):
            r["oldObject"] = dict(objs[i + 1], metadata=o["metadata"])
        out.append(D.AugmentedReview(D.AdmissionRequest(r), None, "Original"))
    return out


def geom(backend):
    import parity_util as P
    templates, constraints = [], []
    for layout in ("RootRoot", "TwoMembers", "PackedOuter", "SelfJoin", "Negated"):
        templates += layout_templates(layout)
        constraints += layout_constraints(layout)
    templates += layout_templates("Mixed", MIXED)
    constraints += layout_constraints("Mixed")
    c, oc = P.load_both(backend, templates, constraints)
    rv = reviews(layout_objects(seed=11, n=150))   # (more than one 64-review half of a row group, more than one 128-review group)
    total = P.assert_parity(c, oc, rv)
    table = c.driver.engine.create_table([D.to_review_in(r) for r in rv], keep_docs=False)
    ev = table.eval()
    assert ev.host_evaluated == [] and not ev.too_big_reviews()
    h = hashlib.sha256()
    for a in (ev.viol, ev.err, ev.too_big):
        h.update(a.tobytes())
    table.free()
    mixed = sum(1 for g in c.ReviewBatch(rv, D.AUDIT_EP) for r in g if r.constraint["kind"].startswith("K8sOrdMixed"))
    return total, mixed, h.hexdigest()


if __name__ == "__main__":
    assert sys.argv[1] == "geom" and os.environ.get("GK_RPT") in ("64", "128", "256")
    print("geom %d %d %s" % geom(sys.argv[2]))
