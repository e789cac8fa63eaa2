"""Seeded differential fuzz of self-join bodies (two iterations of one array, or of two arrays, related by their keys and their
values), product vs oracle on every backend (parity_util.assert_parity: rendered results and raw device bitmaps).  A body:
1-2 arrays at level 0 (`spec.containers`, `spec.initContainers`) or level 1 (`containers[_].env`, `.ports`), random per-side leaf
tests, a random key relation from == != < <= > >=, a value equality between the sides, optionally the whole join under `not`.
tools/self_join_fuzz.py runs the generator over a range of seeds."""
import random

import pytest

from gatekeeper_amd import driver as D
from parity_util import BACKENDS, assert_parity, load_both

RELS = ["==", "!=", "<", "<=", ">", ">="]
NAMES = ["a", "b", "c", None, 1, 1.0]
IMAGES = ["r/x", "r/y", "q/x", "z"]


def _leaf_test(rng, v):
    k = rng.randrange(5)
    if k == 0:
        return '%s.name == "%s"' % (v, rng.choice("abc"))
    if k == 1:
        return '%s.image != "%s"' % (v, rng.choice(IMAGES))
    if k == 2:
        return 'startswith(%s.image, "r/")' % v
    if k == 3:
        return '%s.n > %d' % (v, rng.randrange(3))
    return '%s.name' % v


def gen_template(rng, kind):
    level = rng.randrange(2)
    two = rng.random() < 0.3
    if level == 0:
        arr_a = "input.review.object.spec.containers"
        arr_b = "input.review.object.spec.initContainers" if two else arr_a
        head = ["xa := %s" % arr_a, "xb := %s" % arr_b, "a := xa[i]", "b := xb[j]"]
    else:
        sub_a = rng.choice(["env", "ports"])
        sub_b = ("ports" if sub_a == "env" else "env") if two else sub_a
        if rng.random() < 0.5:   # one container: two iterations of one of its arrays (the keys of one array are related)
            head = ["c := input.review.object.spec.containers[_]", "a := c.%s[i]" % sub_a, "b := c.%s[j]" % sub_a]
        else:                    # two containers: nested scopes under two cursors, the containers' keys related
            head = ["cs := input.review.object.spec.containers", "a := cs[i].%s[_]" % sub_a, "b := cs[j].%s[_]" % sub_b]
    body = list(head)
    body.append("i %s j" % rng.choice(RELS))
    if rng.random() < 0.8:
        body.append("a.%s == b.%s" % (rng.choice(["name", "name", "n"]), rng.choice(["name", "n"])))
    for v in ("a", "b"):
        for _ in range(rng.randrange(3)):
            body.append(_leaf_test(rng, v))
    rego = "package k\n"
    if rng.random() < 0.25:
        rego += "clash {\n  %s\n}\n" % "\n  ".join(body)
        rego += 'violation[{"msg": "no clash"}] {\n  input.review.object.kind == "Pod"\n  not clash\n}\n'
    else:
        msg = rng.choice(['sprintf("%v and %v", [i, j])', 'sprintf("name %v", [a.name])', '"clash"'])
        rego += 'violation[{"msg": msg}] {\n  %s\n  msg := %s\n}\n' % ("\n  ".join(body), msg)
    return {"apiVersion": "templates.gatekeeper.sh/v1", "kind": "ConstraintTemplate", "metadata": {"name": kind.lower()},
            "spec": {"crd": {"spec": {"names": {"kind": kind}}}, "targets": [{"target": "admission.k8s.gatekeeper.sh", "rego": rego}]}}


def _item(rng):
    it = {}
    if rng.random() < 0.9:
        it["name"] = rng.choice(NAMES)
    if rng.random() < 0.8:
        it["image"] = rng.choice(IMAGES)
    if rng.random() < 0.6:
        it["n"] = rng.choice([0, 1, 2, 2.0, 3])
    return it


def gen_object(rng, i):
    def items(k):
        return [_item(rng) for _ in range(rng.randrange(k + 1))]
    cs = []
    for _ in range(rng.randrange(5)):
        c = _item(rng)
        if rng.random() < 0.7:
            c["env"] = items(4)
        if rng.random() < 0.5:
            c["ports"] = items(3)
        cs.append(c)
    spec = {"containers": cs}
    if rng.random() < 0.5:
        spec["initContainers"] = items(3)
    return {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "p%d" % i, "namespace": "default"}, "spec": spec}


def run(backend, seed, n_templates=6, n_objects=24):
    """-> (templates loaded, violations compared); raises on a difference"""
    rng = random.Random(seed)
    templates = [gen_template(rng, "K8sSelfJoin%d" % k) for k in range(n_templates)]
    constraints = [{"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": t["spec"]["crd"]["spec"]["names"]["kind"],
                    "metadata": {"name": "c%d" % k}, "spec": {}} for k, t in enumerate(templates)]
    objs = [gen_object(rng, i) for i in range(n_objects)]
    c, oc = load_both(backend, templates, constraints)
    return len(templates), assert_parity(c, oc, [D.AugmentedUnstructured(D.Unstructured(o), None, "Original") for o in objs])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_self_join_fuzz(backend, seed):
    n, _ = run(backend, 7100 + seed)
    assert n == 6
