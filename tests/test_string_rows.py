"""The device's string ROW predicates (csrc/vm_core.hpp: str_prefix_c, str_at_c / swin, str_contains_short, str_eq_c, str_cmp_c) at every
length class of constant and string: inline strings (<= 7 bytes), header-only strings (<= 12), heap words beyond byte 12; constants of at
most 7, at most 12 and more than 12 bytes with every remainder; the match at every word alignment, ending in the string's last byte, inside
the header and across its border; zero padding behind the last byte against NUL bytes in the string.

Since the promotion of string tests to dictionary expressions (lower.cpp PROMOTION) the HOST answers these tests per distinct value and the
device tests a bit; the rows remain the product's answer behind a full dictionary and under a filtered key iteration, which is how these
tests reach them: str_rows_util.fill_dictionaries() first, str_rows_util.require_rows() as the guard that they stay there.  One probe string
per review and place (one container image: element scope; one annotation: review-level bits), so one raw bit is one predicate on one
string; the raw violation bitmap must EQUAL the pair set of Python `bytes` arithmetic -- a lost bit renders nothing and raises nothing, only
this comparison sees it -- and a 1-in-8 sample goes through parity_util.assert_parity, so that rendering is covered too."""
import functools

import pytest

import str_rows_util as S
from parity_util import BACKENDS, assert_parity, load_both

SQUEEZED = (2, 4, 2)   # element capacities as tests/test_step_overhead.py squeezes them: Pods of five containers take the big path


@functools.lru_cache(maxsize=None)
def probe_objs():
    """one Pod per probe string: the string is the image of its only container and its `probe` annotation"""
    return tuple(S.pod(i, [s], s) for i, s in enumerate(S.probe_strings()))


@functools.lru_cache(maxsize=None)
def big_objs():
    """a 200-string subset (every 12th probe) as Pods of five containers; the annotation holds the Pod's third string"""
    strs = S.probe_strings()[::12][:200]
    return tuple(S.pod(i // 5, strs[i:i + 5], strs[min(i + 2, len(strs) - 1)]) for i in range(0, len(strs), 5))


def load_family(backend, family, **kw):
    c, oc = load_both(backend, [], [], **kw)
    S.fill_dictionaries(c, [S.IMAGE, S.PROBE], oc)
    templates, constraints, what = S.family_policy(S.FAMILIES[family])
    for t in templates:
        c.AddTemplate(t)
        oc.add_template(t)
    for k in constraints:
        c.AddConstraint(k)
        oc.add_constraint(k)
    for test in S.FAMILIES[family]:
        for place, dst in (("Elem", 1), ("Rev", 0)):
            S.require_rows(c, S.kind_of(test, place), S.OPS[test], len(S.CONSTANTS), dsts=(dst,))
    return c, oc, what


@pytest.mark.parametrize("family", list(S.FAMILIES))
@pytest.mark.parametrize("backend", BACKENDS)
def test_family_at_every_length_class(backend, family):
    c, oc, what = load_family(backend, family)
    objs = probe_objs()
    assert len(objs) > 2000
    n = S.assert_raw_pairs(c, objs, what)
    assert n > len(S.CONSTANTS) * 2                       # (every constant holds on some probe, in both places)
    assert assert_parity(c, oc, S.reviews_of(objs[3::8])) > 0


@pytest.mark.parametrize("family", list(S.FAMILIES))
@pytest.mark.parametrize("backend", BACKENDS)
def test_family_on_the_big_path(backend, family):
    """squeezed element capacities: every Pod has more containers than the accumulators hold and is evaluated by the big variant"""
    c, oc, what = load_family(backend, family, elem_cap=SQUEEZED)
    assert S.assert_raw_pairs(c, big_objs(), what, overflow=True) > 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_under_a_filtered_key_iteration(backend):
    """`v := labels[key]; startswith(key, "a"); <test>(v, P)`: a dictionary expression cannot stand under a key iteration with key filters,
    so the lowering keeps prefix, suffix and contains on the rows without any filler.  Every fourth probe string as the value of a label the
    filter lets through; the constant itself -- a hit of every test -- under a key it does not."""
    tests = ("prefix", "suffix", "contains")
    templates, constraints, what = S.family_policy(tests, places=("Label",))
    c, oc = load_both(backend, templates, constraints)
    for t in tests:
        S.require_rows(c, S.kind_of(t, "Label"), S.OPS[t], len(S.CONSTANTS), dsts=(0,), filled=False)
    strs = S.probe_strings()[::4]
    objs = [S.pod(i, ["x"], labels={"app": s, "b": S.CONSTANTS[i % len(S.CONSTANTS)], "a2": ""}) for i, s in enumerate(strs)]
    assert S.assert_raw_pairs(c, objs, what) > 3 * len(S.CONSTANTS)
    assert assert_parity(c, oc, S.reviews_of(objs[1::8])) > 0


# ---------------------------------------------------------------------------------------------- P_STR_IN_SET: the match layer's string sets
KINDS_OF_MATCH = [   # all members inline (<= 7 bytes), mixed, all on the heap; the empty group; a wildcard next to a set
    [{"apiGroups": [""], "kinds": ["Pod", "Secret", "Service"]}],
    [{"apiGroups": ["", "apps"], "kinds": ["Pod", "Job", "Ingress"]}],
    [{"apiGroups": ["apps", "batch", "networking.k8s.io"], "kinds": ["Deployment", "Job", "StatefulSet", "Ingress"]}],
    [{"apiGroups": ["networking.k8s.io", "storage.k8s.io"], "kinds": ["StatefulSet", "ReplicationController", "NetworkPolicy"]}],
    [{"apiGroups": ["*"], "kinds": ["Pod", "ReplicationController"]}],
    [{"apiGroups": ["apps"], "kinds": ["*"]}, {"apiGroups": [""], "kinds": ["Service", "ReplicationController"]}],
    [{"apiGroups": ["batch"], "kinds": ["CronJobs", "CronJob"]}],           # 8 and 7 bytes
    [{"apiGroups": ["policy"], "kinds": ["PodDisruptionBudget", "Pod"]}],
]
MATCH_FILLERS = 31   # two expressions each (kind, group) in the 62-bit space the match facts of a candidate share


def gvk_probes():
    groups = ["", "apps", "batch", "networking.k8s.io", "storage.k8s.io", "app", "appss", "networking.k8s.i", "networking.k8s.iox", "policy", "Apps"]
    kinds = ["Pod", "Secret", "Service", "Job", "Ingress", "Deployment", "StatefulSet", "ReplicationController", "NetworkPolicy", "CronJob", "CronJobs", "PodDisruptionBudget",
             "Po", "Pods", "pod", "Servic", "Services", "Deploymen", "Deployments", "ReplicationControlle", "ReplicationControllers", "StatefulSeT", "Ingres\u00e9", "X"]
    return [(g, k) for g in groups for k in kinds]


@pytest.mark.parametrize("backend", BACKENDS)
def test_match_sets_behind_a_full_match_dictionary(backend):
    """spec.match.kinds: the kind and the group of a review against constant string sets.  As loaded these are expressions of the match
    facts' dictionary; behind 31 filler constraints with kinds and groups of their own the sets are row predicates (P_STR_IN_SET: members
    of at most 7 bytes inline, longer ones by hash and offset).  The template always violates, so the raw violation bitmap is the match:
    it must equal plain set membership of (group, kind), near misses of every member included."""
    always = S.template("K8sAlways", ["true"])
    c, oc = load_both(backend, [always], [])
    cons = []
    for i in range(MATCH_FILLERS):
        cons.append(S.constraint("K8sAlways", "fill%02d" % i, {}))
        cons[-1]["spec"]["match"] = {"kinds": [{"apiGroups": ["fill%02d.example" % i], "kinds": ["Fill%02d" % i]}]}
    for i, kinds in enumerate(KINDS_OF_MATCH):
        cons.append(S.constraint("K8sAlways", "set%d" % i, {}))
        cons[-1]["spec"]["match"] = {"kinds": kinds}
    for k in cons:
        c.AddConstraint(k)
        oc.add_constraint(k)
    # (kind and group of the object and of the old object: four sets per constraint, fewer where a wildcard stands)
    S.require_rows(c, "K8sAlways", S.P_STR_IN_SET, len(cons), dsts=(0,), min_preds=2 * len(KINDS_OF_MATCH))
    probes = gvk_probes()
    objs = [{"apiVersion": (g + "/v1") if g else "v1", "kind": k, "metadata": {"name": "o%d" % i, "namespace": "default"}} for i, (g, k) in enumerate(probes)]
    want = {(("K8sAlways", "set%d" % j), i) for i, (g, k) in enumerate(probes) for j, kinds in enumerate(KINDS_OF_MATCH)
            if any(("*" in e["apiGroups"] or g in e["apiGroups"]) and ("*" in e["kinds"] or k in e["kinds"]) for e in kinds)}
    ev, viol, err = S.raw_pairs(c, objs)
    assert ev.host_evaluated == [] and not ev.too_big_reviews() and not err
    assert viol == want, "raw bitmap != set membership: only device %r, only reference (LOST) %r" % (sorted(viol - want)[:6], sorted(want - viol)[:6])
    assert len(want) > 40
    assert assert_parity(c, oc, S.reviews_of(objs[::3])) > 0
