"""Shared by test_numeric_index.py: the templates and objects of the numeric-index tests (`cs[0]`, `cs[count(cs) - 1]`, `cs[i]; i > 0`:
pe.cpp index_elem, cursors.hpp F_KIMM / F_KEND), and -- run as a script in a process of its own, because the row-group geometry (GK_RPT)
is read once per process --
usage: numeric_index_util.py geom <backend>    the whole rule set in ONE plan over 150 objects against the oracle (parity_util.assert_parity);
                                               prints the violation count and the SHA-256 of the raw violation / error / too_big words
       numeric_index_util.py fuzz <backend> <first seed> <seeds>    the differential fuzz of test_numeric_index.py, one plan per call
backend: hostemu (with GK_HOSTEMU_KERNEL=jit: the emulated plan-specialised kernel, checked against the interpreter word by word) or gpu."""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gatekeeper_amd import driver as D   # noqa: E402
from value_order_util import cons, pod, reviews, tmpl   # noqa: E402,F401

# one template per accepted form: kind -> rule
RULES = {
    # P[k] with a string test on a member
    "First": '''violation[{"msg": msg}] {
  c := input.review.object.spec.containers[0]
  startswith(c.image, "bad/")
  msg := sprintf("first container %v runs %v", [c.name, c.image])
}''',
    # P[count(P) - m] through a local variable
    "Last": '''violation[{"msg": "the last container is the sidecar"}] {
  cs := input.review.object.spec.containers
  cs[count(cs) - 1].name == "sidecar"
}''',
    # an index under `not`
    "NoSecond": '''violation[{"msg": "no second container"}] {
  input.review.object.kind == "Pod"
  not input.review.object.spec.containers[1]
}''',
    # P[i] with a relation on the iteration's key, and the key in the message
    "Later": '''violation[{"msg": msg}] {
  cs := input.review.object.spec.containers
  cs[i].image == "pause"
  i > 0
  msg := sprintf("container %d runs pause", [i])
}''',
    # an array of scalars
    "Args": '''violation[{"msg": "privileged"}] {
  input.review.object.spec.args[0] == "--privileged"
}''',
    # a nested iteration below the indexed element
    "Ports": '''violation[{"msg": "the first container listens on 80"}] {
  input.review.object.spec.containers[0].ports[_].containerPort == 80
}''',
    # a self-join with one indexed side
    "Differ": '''violation[{"msg": "an image differs from the first container's"}] {
  cs := input.review.object.spec.containers
  cs[0].image != cs[_].image
}''',
    # the same index as two separate terms: one binding
    "Twice": '''violation[{"msg": "nginx first"}] {
  input.review.object.spec.containers[0].name == "main"
  input.review.object.spec.containers[0].image == "nginx"
}''',
}
KINDS = sorted(RULES)


def kind_of(rule):
    return "K8sIdx" + rule


def rule_templates(rules=None):
    return [tmpl(kind_of(r), "package k\n" + RULES[r]) for r in (rules or KINDS)]


def rule_constraints(rules=None):
    return [cons(kind_of(r)) for r in (rules or KINDS)]


def ctr(name, image, *ports):
    c = {"name": name, "image": image}
    if ports:
        c["ports"] = [{"containerPort": p} for p in ports]
    return c


def basic_objects():
    """containers absent, [], one, two and three elements, an element that is a string, one that is {}, and (LAST) an OBJECT with a member "0\""""
    objs = [
        {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "absent", "namespace": "default"}, "spec": {"args": ["--privileged"]}},
        pod([], "empty", args=[]),
        pod([ctr("main", "bad/a", 80)], "one", args=["-v", "--privileged"]),
        pod([ctr("main", "nginx", 8080, 80), ctr("sidecar", "pause")], "two", args=["--privileged", "-v"]),
        pod([ctr("a", "pause", 81), ctr("b", "pause", 80), ctr("sidecar", "bad/z")], "three"),
        pod(["text", ctr("sidecar", "pause")], "string-element"),
        pod([{}, ctr("x", "pause"), {}], "empty-element", args="--privileged"),
        pod([ctr("main", "nginx"), ctr("main", "nginx"), ctr("c", "pause"), ctr("sidecar", "nginx")], "four"),
        pod({"0": ctr("main", "bad/o", 80)}, "object-with-0"),
    ]
    return objs


# (object, rule) -> violates, by hand from the Rego (the oracle is not the only witness)
BY_HAND = {
    ("absent", "NoSecond"): True, ("absent", "Args"): True, ("absent", "First"): False,
    ("empty", "NoSecond"): True, ("empty", "Last"): False,
    ("one", "First"): True, ("one", "Ports"): True, ("one", "Args"): False, ("one", "Differ"): False, ("one", "NoSecond"): True,
    ("two", "Twice"): True, ("two", "Last"): True, ("two", "Later"): True, ("two", "Ports"): True, ("two", "Differ"): True, ("two", "NoSecond"): False,
    ("three", "Later"): True, ("three", "Ports"): False, ("three", "Last"): True, ("three", "First"): False,
    ("string-element", "Last"): True, ("string-element", "Differ"): False, ("string-element", "Later"): True,
    ("empty-element", "Later"): True, ("empty-element", "Last"): False, ("empty-element", "Args"): False,
    ("four", "Twice"): True, ("four", "Differ"): True, ("four", "Last"): True,
}


def random_pod(rng, name):
    """containers absent now and then, else 0..4 elements (a few of them no objects), args of 0..3 scalars"""
    spec = {}
    if rng.random() < 0.9:
        cs = []
        for ci in range(rng.randrange(0, 5)):
            r = rng.random()
            if r < 0.06:
                cs.append(rng.choice(["text", {}, 7]))
                continue
            c = {}
            if rng.random() < 0.9:
                c["name"] = rng.choice(["main", "sidecar", "a", "b"])
            if rng.random() < 0.9:
                c["image"] = rng.choice(["nginx", "pause", "bad/a", "bad/b-long-image-name"])
            if rng.random() < 0.6:
                c["ports"] = [{"containerPort": rng.choice([80, 81, 8080, "80"])} for _ in range(rng.randrange(0, 3))]
            cs.append(c)
        spec["containers"] = cs
    if rng.random() < 0.8:
        spec["args"] = [rng.choice(["--privileged", "-v", 1, True]) for _ in range(rng.randrange(0, 4))]
    return {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": name, "namespace": "default"}, "spec": spec}


def result_words(c, rv):
    """(the Eval, host_evaluated, SHA-256 of the raw violation / error / too_big words) of a table of the reviews"""
    table = c.driver.engine.create_table([D.to_review_in(r) for r in rv], keep_docs=False)
    try:
        ev = table.eval()
        h = hashlib.sha256()
        for a in (ev.viol, ev.err, ev.too_big):
            h.update(a.tobytes())
        return list(ev.host_evaluated), [int(r) for r in ev.too_big_reviews()], h.hexdigest()
    finally:
        table.free()


def geom(backend):
    import parity_util as P
    c, oc = P.load_both(backend, rule_templates(), rule_constraints())
    rng = random.Random(23)
    rv = reviews(basic_objects()[:-1] + [random_pod(rng, "r%d" % i) for i in range(142)])   # (more than one 128-review group)
    total = P.assert_parity(c, oc, rv)
    host, big, digest = result_words(c, rv)
    assert host == [] and big == []
    return total, digest


# ---------------------------------------------------------------------------------------------------------------- differential fuzz
PATHS = {"cs": "input.review.object.spec.containers", "args": "input.review.object.spec.args"}


def fuzz_template(rng, kind):
    """one accepted form with a random k / m in 0..3: P[k], P[count(P) - m], P[i] with i <op> k (either operand order), under `not`, below a
    nested iteration, as one side of a self-join, or twice in one body"""
    k, m = rng.randrange(0, 4), rng.randrange(0, 4)
    form = rng.choice(["const", "end", "rel", "not", "nested", "join", "twice", "args", "argsend", "relflip"])
    head, lines = '{"msg": "m"}', []
    if form == "const":
        lines = ['c := %s[%d]' % (PATHS["cs"], k), 'c.image == "%s"' % rng.choice(["nginx", "pause"])]
        head, lines = '{"msg": msg}', lines + ['msg := sprintf("%v", [c.name])']
    elif form == "end":
        lines = ['cs := %s' % PATHS["cs"], 'cs[count(cs) - %d].name == "%s"' % (m, rng.choice(["main", "sidecar"]))]
    elif form in ("rel", "relflip"):
        op = rng.choice(["==", "!=", "<", "<=", ">", ">="])
        kk = rng.choice([str(k), str(k), "%d.5" % k])
        lines = ['cs := %s' % PATHS["cs"], 'startswith(cs[i].image, "bad/")', ("i %s %s" % (op, kk)) if form == "rel" else ("%s %s i" % (kk, op))]
        head, lines = '{"msg": msg}', lines + ['msg := sprintf("%d", [i])']
    elif form == "not":
        lines = ['input.review.object.kind == "Pod"', 'not %s[%d].name' % (PATHS["cs"], k)]
    elif form == "nested":
        lines = ['%s[%d].ports[_].containerPort == 80' % (PATHS["cs"], k)]
    elif form == "join":
        lines = ['cs := %s' % PATHS["cs"], 'cs[%d].image %s cs[_].image' % (k, rng.choice(["==", "!="]))] if rng.random() < 0.5 else \
                ['cs := %s' % PATHS["cs"], 'cs[count(cs) - %d].name == cs[%d].name' % (max(m, 1), k)]
    elif form == "twice":
        lines = ['%s[%d].name == "main"' % (PATHS["cs"], k), '%s[%d].image == "nginx"' % (PATHS["cs"], k)]
    elif form == "args":
        lines = ['%s[%d] == "%s"' % (PATHS["args"], k, rng.choice(["--privileged", "-v"]))]
    else:
        lines = ['a := %s' % PATHS["args"], 'a[count(a) - %d] == "-v"' % m]
    return tmpl(kind, "package k\nviolation[%s] {\n  %s\n}\n" % (head, "\n  ".join(lines)))


def run_fuzz(backend, seeds, per_seed=4, n_objs=10):
    """one plan for all the seeds' templates, one batch of objects; every generated template must compile (AddConstraint raises otherwise)"""
    import parity_util as P
    templates, constraints, objs = [], [], []
    for seed in seeds:
        rng = random.Random(seed)
        for j in range(per_seed):
            kind = "K8sIdxFuzz%dx%d" % (seed, j)
            templates.append(fuzz_template(rng, kind))
            constraints.append(cons(kind))
        objs += [random_pod(rng, "s%d-%d" % (seed, i)) for i in range(n_objs)]
    c, oc = P.load_both(backend, templates, constraints)
    rv = reviews(objs)
    total = P.assert_parity(c, oc, rv)
    host, big, _ = result_words(c, rv)
    assert host == [] and big == []
    return total


if __name__ == "__main__":
    if sys.argv[1] == "geom":
        assert os.environ.get("GK_RPT") in ("64", "128", "256")
        print("geom %d %s" % geom(sys.argv[2]))
    else:
        assert sys.argv[1] == "fuzz"
        print("fuzz %d" % run_fuzz(sys.argv[2], range(int(sys.argv[3]), int(sys.argv[3]) + int(sys.argv[4]))))
