"""Self-joins: two independent iterations of one array in one rule body (`a := cs[_]; b := cs[_]`, `cs[i] .. cs[j]; i != j`).
The device plan walks the second iteration with a loop cursor of its own (cursors.hpp) and relates the two keys with F_KCMP; every
case is compared with the oracle -- rendered results and raw device bitmaps (parity_util.assert_parity) -- on every backend, and the
violation counts (the oracle's) are pinned.  Before loop cursors the inner loop reset the outer one: the repro answered nothing."""
import pytest

from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from parity_util import BACKENDS, assert_parity, load_both


def tmpl(kind, rego):
    return {"apiVersion": "templates.gatekeeper.sh/v1", "kind": "ConstraintTemplate", "metadata": {"name": kind.lower()},
            "spec": {"crd": {"spec": {"names": {"kind": kind}}}, "targets": [{"target": "admission.k8s.gatekeeper.sh", "rego": rego}]}}


def cons(kind, name="c", match=None):
    spec = {} if match is None else {"match": match}
    return {"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": kind, "metadata": {"name": name}, "spec": spec}


def pod(containers, name="p", kind="Pod", spec_extra=None):
    spec = {"containers": containers}
    spec.update(spec_extra or {})
    return {"apiVersion": "v1", "kind": kind, "metadata": {"name": name, "namespace": "default"}, "spec": spec}


def reviews(objs):
    return [D.AugmentedUnstructured(D.Unstructured(o), None, "Original") for o in objs]


def run(backend, kinds, objs, match=None):
    c, oc = load_both(backend, [tmpl(k, REGO[k]) for k in kinds], [cons(k, "c-" + k.lower(), match) for k in kinds])
    return assert_parity(c, oc, reviews(objs))


REGO = {}
REGO["K8sDupImage"] = '''package k
violation[{"msg": msg}] {
  a := input.review.object.spec.containers[_]
  b := input.review.object.spec.containers[_]
  a.name == b.name
  a.image != b.image
  msg := sprintf("container name %v used twice", [a.name])
}
'''
REGO["K8sDupSides"] = '''package k
violation[{"msg": msg}] {
  a := input.review.object.spec.containers[_]
  b := input.review.object.spec.containers[_]
  a.image == "a"
  b.image == "b"
  a.name == b.name
  msg := sprintf("container name %v used by images a and b", [a.name])
}
'''
REGO["K8sDupName"] = '''package k
violation[{"msg": msg}] {
  c := input.review.object.spec.containers
  c[i].name == c[j].name
  i != j
  msg := sprintf("container name %v used twice", [c[i].name])
}
'''
REGO["K8sDupEnv"] = '''package k
violation[{"msg": msg}] {
  c := input.review.object.spec.containers[_]
  e1 := c.env[i]
  e2 := c.env[j]
  i != j
  e1.name == e2.name
  msg := sprintf("container %v declares env %v twice", [c.name, e1.name])
}
'''
REGO["K8sPortClash"] = '''package k
violation[{"msg": msg}] {
  c := input.review.object.spec.containers
  p1 := c[i].ports[_]
  p2 := c[j].ports[_]
  i < j
  p1.containerPort == p2.containerPort
  msg := sprintf("containerPort %v declared by %v and %v", [p1.containerPort, c[i].name, c[j].name])
}
'''
REGO["K8sDupPairs"] = '''package k
violation[{"msg": msg}] {
  c := input.review.object.spec.containers
  c[i].name == c[j].name
  i < j
  msg := sprintf("containers %v and %v share the name %v", [i, j, c[i].name])
}
'''
REGO["K8sNoTwin"] = '''package k
twin(a) {
  b := input.review.object.spec.containers[_]
  b.name == a.name
  b.image != a.image
}
violation[{"msg": msg}] {
  a := input.review.object.spec.containers[_]
  a.image == "solo"
  not twin(a)
  msg := sprintf("container %v has no twin", [a.name])
}
'''
REGO["K8sDupMount"] = '''package k
violation[{"msg": msg}] {
  m := input.review.object.spec.containers[_].volumeMounts
  m[i].mountPath == m[j].mountPath
  i != j
  msg := sprintf("mountPath %v mounted twice", [m[i].mountPath])
}
'''
REGO["K8sHostPortClash"] = '''package k
violation[{"msg": msg}] {
  c := input.review.object.spec.containers
  c[i].ports[_].hostPort == c[j].ports[_].hostPort
  i > j
  msg := sprintf("hostPort clash between %v and %v", [c[j].name, c[i].name])
}
'''

REPRO = pod([{"name": "app", "image": "a:1"}, {"name": "app", "image": "b:1"}])


@pytest.mark.parametrize("backend", BACKENDS)
def test_regression_two_iterations_of_one_array(backend, monkeypatch):
    """the issue's repro and its per-side-filter variant: accepted before, and answered with nothing"""
    monkeypatch.setenv("GK_RENDER_CHECK", "1")   # (both host evaluators render the messages; a difference is an error)
    objs = [REPRO,
            pod([{"name": "app", "image": "a"}, {"name": "app", "image": "b"}, {"name": "x", "image": "b"}]),
            pod([{"name": "app", "image": "a"}, {"name": "other", "image": "b"}]),
            pod([{"name": "app", "image": "a"}])]
    assert run(backend, ["K8sDupImage"], objs) == 2
    assert run(backend, ["K8sDupSides"], objs) == 1
    c, oc = load_both(backend, [tmpl("K8sDupImage", REGO["K8sDupImage"])], [cons("K8sDupImage")])
    got = c.ReviewBatch(reviews([REPRO]), D.AUDIT_EP)
    assert [r.msg for r in got[0]] == ["container name app used twice"]


SPORTS = pod([{"name": "a", "image": "i", "ports": [{"containerPort": 80}, {"containerPort": 80}]},
              {"name": "b", "image": "j", "ports": [{"containerPort": 80.0}, {"containerPort": 81, "hostPort": 81}]},
              {"name": "c", "image": "k", "ports": [{"containerPort": 81, "hostPort": 81}]}])
SENV = pod([{"name": "a", "image": "i", "env": [{"name": "X", "value": "1"}, {"name": "Y"}, {"name": "X", "value": "2"}],
             "volumeMounts": [{"name": "v", "mountPath": "/d"}, {"name": "w", "mountPath": "/d"}]},
            {"name": "b", "image": "i", "env": [{"name": "Y"}], "volumeMounts": [{"name": "v", "mountPath": "/e"}]},
            {"name": "a", "image": "j", "env": [{"name": "X"}, {"name": "Z"}]}])


@pytest.mark.parametrize("backend", BACKENDS)
def test_idioms(backend, monkeypatch):
    monkeypatch.setenv("GK_RENDER_CHECK", "1")
    objs = [REPRO, SPORTS, SENV, pod([{"name": "solo1", "image": "solo"}, {"name": "solo1", "image": "x"}, {"name": "solo2", "image": "solo"}])]
    assert run(backend, ["K8sDupName"], objs) == 3
    assert run(backend, ["K8sDupEnv"], objs) == 1          # env inside ONE container (nested scope, same parent): X in `a`, not Y across
    assert run(backend, ["K8sPortClash"], objs) == 2       # 80 (a) vs 80.0 (b), 81 (b) vs 81 (c); a's own duplicate 80 is not a clash
    assert run(backend, ["K8sHostPortClash"], objs) == 1
    assert run(backend, ["K8sDupMount"], objs) == 1
    assert run(backend, ["K8sNoTwin"], objs) == 1          # a self-join under `not`: solo2
    assert run(backend, ["K8sDupPairs", "K8sDupName", "K8sPortClash"], objs) == 8


@pytest.mark.parametrize("backend", BACKENDS)
def test_each_pair_once(backend):
    c, oc = load_both(backend, [tmpl("K8sDupPairs", REGO["K8sDupPairs"])], [cons("K8sDupPairs")])
    objs = [pod([{"name": "a", "image": "1"}, {"name": "b", "image": "1"}, {"name": "a", "image": "2"}, {"name": "a", "image": "3"}])]
    assert assert_parity(c, oc, reviews(objs)) == 3
    got = c.ReviewBatch(reviews(objs), D.AUDIT_EP)
    assert sorted(r.msg for r in got[0]) == ["containers 0 and 2 share the name a", "containers 0 and 3 share the name a",
                                              "containers 2 and 3 share the name a"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_with_match_block(backend):
    objs = [REPRO, pod(REPRO["spec"]["containers"], name="d", kind="Deployment"), SENV]
    match = {"kinds": [{"apiGroups": [""], "kinds": ["Pod"]}]}
    assert run(backend, ["K8sDupName", "K8sDupImage"], objs, match=match) == 4


def _n(k, image="i"):
    return [{"name": "c%d" % (i // 2), "image": "%s%d" % (image, i)} for i in range(k)]


@pytest.mark.parametrize("backend", BACKENDS)
def test_edges(backend):
    objs = [pod([]), pod(_n(1)), pod(_n(2)), pod(_n(8)), pod(_n(12)), pod(_n(40)),          # 0, 1, 2, the default capacity, beyond it
            pod([{"name": None, "image": "a"}, {"name": None, "image": "b"}]),                # null == null
            pod([{"image": "a"}, {"name": "x", "image": "b"}, {"image": "c"}]),              # a key missing on one side (or both)
            pod([{"name": 1, "image": "a"}, {"name": 1.0, "image": "b"}, {"name": "1", "image": "c"}]),   # 1 == 1.0, never "1"
            pod([{"name": {"n": 1}, "image": "a"}, {"name": {"n": 1}, "image": "b"}]),      # non-empty containers: the host answers
            pod([{"name": [], "image": "a"}, {"name": [], "image": "b"}, {"name": {}, "image": "c"}]),
            {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "o", "namespace": "default"},   # an OBJECT where the array is iterated
             "spec": {"containers": {"x": {"name": "app", "image": "a"}, "y": {"name": "app", "image": "b"}}}}]
    assert run(backend, ["K8sDupImage", "K8sDupName", "K8sDupPairs"], objs) == 108


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("policy", ["configs2", "corpus"])
def test_one_plan_with_the_synthetic_sets(backend, policy):
    """self-join constraints in ONE plan with configs[2]'s 50 constraints / the 200-template corpus, over the synthetic stream"""
    fx = synth.load_fixtures()
    if policy == "configs2":
        templates, constraints = synth.psp_templates(fx), synth.audit_constraints()
    else:
        templates, constraints = synth.corpus(fx, 200 if backend != "hostemu-gen" else 60)
    kinds = ["K8sDupName", "K8sPortClash", "K8sDupEnv", "K8sNoTwin"]
    templates = list(templates) + [tmpl(k, REGO[k]) for k in kinds]
    constraints = list(constraints) + [cons(k, "sj-" + k.lower()) for k in kinds]
    c, oc = load_both(backend, templates, constraints)
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(48, seed=5, mixed=True)
    for i, o in enumerate(objs):   # some duplicates for the self-joins to find
        cs = (o.get("spec") or {}).get("containers")
        if i % 3 == 0 and isinstance(cs, list) and cs:
            cs.append(dict(cs[0], image="dup/" + str(i), ports=[{"containerPort": 8080}]))
            cs[0]["ports"] = [{"containerPort": 8080}]
    objs += [REPRO, SPORTS, SENV]
    rv = [D.AugmentedUnstructured(D.Unstructured(o), synth.namespace_for(o, nss), "Original") for o in objs]
    assert assert_parity(c, oc, rv) > 0
    got = c.ReviewBatch(rv, D.AUDIT_EP)
    assert sum(1 for g in got for r in g if r.constraint["metadata"]["name"].startswith("sj-")) > 16


REFUSALS = [
    ('''package k
violation[{"msg": "m"}] {
  cs := input.review.object.spec.containers
  a := cs[_].ports[i]
  b := cs[_].ports[j]
  i < j
  a.containerPort == b.containerPort
}
''', "key relation between elements of different nested arrays"),
    ('''package k
violation[{"msg": "m"}] {
  l := input.review.object.metadata.labels
  l[k1]
  l[k2]
  startswith(k1, "app")
  k1 != k2
}
''', "key relation on an object-key iteration"),
    ('''package k
violation[{"msg": "m"}] {
  c := input.review.object.spec.containers[i]
  v := input.review.object.spec.volumes[i]
  c.name == v.name
}
''', "review data indexed by a symbolic key"),
    ('''package k
violation[{"msg": "m"}] {
  c := input.review.object.spec.containers[i]
  c.ports[i].containerPort == 80
}
''', "review data indexed by a symbolic key"),
]


@pytest.mark.parametrize("rego,why", REFUSALS)
def test_refusals_that_remain(rego, why):
    c, _ = load_both("hostemu", [], [])
    c.AddTemplate(tmpl("K8sRefused", rego))
    with pytest.raises(D.UnsupportedError, match=why):
        c.AddConstraint(cons("K8sRefused"))


def test_running_out_of_cursor_ids():
    """31 element scopes of their own plus containers: the self-join's alias cursor would be the 33rd id"""
    rules = []
    for k in range(31):
        rules.append('''violation[{"msg": "x%d"}] {
  v := input.review.object.spec.x%d[_]
  v.a == 1
  v.b == 2
}''' % (k, k))
    rules.append(REGO["K8sDupName"].split("\n", 1)[1])
    c, _ = load_both("hostemu", [], [])
    c.AddTemplate(tmpl("K8sMany", "package k\n" + "\n".join(rules)))
    with pytest.raises(D.UnsupportedError, match="self-joins need more loop cursors than the plan has ids"):
        c.AddConstraint(cons("K8sMany"))
