"""Ordering relations between two review values (tests/test_value_order.py) on the paths and values its tests leave out: the edges of
the order itself (a: int64 against double, inline against heap strings, bytes >= 0x80 and NUL) answered by a reference that is not the
oracle (tests/rego_order_ref.py); ranks that need more than 8 of the packed id's 16 bits (b); the large-variant kernel, loops with
nothing to walk around an ordering literal and a resident table's plan variant (c); every ingest path -- table, native table, pruned
table, spool, AdmissionRequests, the resident set (d); RESULT totals, top-k and several plan groups (e); policy changes (f); and the
differential fuzz of test_value_order.py on the values of (a) with larger pods (g).  Every case is bit-exact against a reference;
where a case is ABOUT something -- the device's answer, overflow into the large variant, wide ranks, every relation in the fuzz --
that condition is asserted, or the case would show nothing."""
import functools
import json
import os
import random
import re

import pytest

import rego_order_ref as R
import test_value_order as V
import value_order_paths_util as P
import value_order_util as U
from gatekeeper_amd import _lib as L
from gatekeeper_amd import driver as D
from oracle import values as OV
from parity_util import BACKENDS, assert_parity, key, load_both, plan_group_max, to_oracle_review

PREFIX = "K8sOrd"


def raw(c, rv, namespaces=None, **kw):
    """the raw words of one evaluation of a table created now -> (viol, err, too_big, EvalResult)"""
    table = c.driver.engine.create_table([D.to_review_in(r, namespaces[i] if namespaces else None) for i, r in enumerate(rv)], keep_docs=False, **kw)
    try:
        ev = table.eval()
    finally:
        table.free()
    return ev


def words(ev):
    return (ev.viol.tobytes(), ev.err.tobytes(), ev.too_big.tobytes(), tuple(int(x) for x in ev.constraint_ids))


def device_kinds(c, ev, review, ep=D.AUDIT_EP):
    """the kinds of the constraints whose raw violation bit is set for one review, sorted"""
    active = {cid: cons.get("kind") for cid, (cons, _, _) in c._active(ep).items()}
    return sorted(active[cid] for cid, r in ev.pairs("viol") if r == review and cid in active)


def load_layouts(backend, layouts, **kw):
    templates, constraints = [], []
    for layout in layouts:
        templates += U.layout_templates(layout, U.MIXED if layout == "Mixed" else None)
        constraints += U.layout_constraints(layout)
    return load_both(backend, templates, constraints, **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. the reference
S20 = "abcdefghijklmnopqrst"
HEAP = "abcdefghij"   # (a heap string: more than the 7 bytes an inline string holds)
# (a) the edges of the order, all answered on the device: numbers first, then strings, then the empty containers against a heap string
EDGES = [(-9223372036854775808, -9.223372036854775808e18), (9007199254740993, 9007199254740992.0), (0.1, 1e-1), (5e-324, 0), (-0.0, 0), (100, 1e2),
         (-2.5, -2), (1.7976931348623157e308, 1e300), (9223372036854775807, 9223372036854775806), (-9223372036854775808, -9223372036854775807.5),
         (9007199254740993, 9007199254740994.0), (4611686018427387904.0, 4611686018427387905), (-5e-324, 0), (0.5, -0.5),
         ("abcdefg", "abcdefgh"), ("abcdefgh", "abcdefg"), (S20, S20[:12] + "N" + S20[13:]), (S20[:12] + "L" + S20[13:], S20),
         (S20, S20[:16] + "R" + S20[17:]), (S20[:16] + "P" + S20[17:], S20), ("é", "z"), ("a\u0000", "a"), ("a\u0000b", "a\u0000"), ("", "\u0000"),
         ("éabcdefgh", "zabcdefgh"), ("abcdefg\u0000", "abcdefg"), ("￿", "\U00010000"),
         ([], HEAP), ({}, HEAP), (HEAP, []), (HEAP, {}), ([], {})]
# ... and the pairs with a number the flattener cannot vouch for: an integral number beyond int64 may be the float64 of a longer
# text, so it carries no rank and the review is answered by the host evaluator -- with the reference's answer
EDGES_HOST = [(9223372036854775807, 9223372036854775808.0), (1e19, 9223372036854775807), (-9223372036854775808, -1e19), (1e19, "1e19")]
RANK_SEED, N_WIDE = 7, 640


def wide_values():
    return P.many_values(RANK_SEED, N_WIDE)


def test_reference_order_on_the_basic_pairs_and_the_oracle_against_it():
    """the reference against the twelve hand-written pairs, then the oracle against the reference on every pair the tests below use"""
    for a, b, want in V.BASIC:
        assert R.sign(a, b) == want and R.sign(b, a) == -want, (a, b)
    vals = wide_values()
    ordered = sorted(vals, key=functools.cmp_to_key(R.sign))
    pairs = [(a, b) for a, b, _ in V.BASIC + V.MORE] + EDGES + EDGES_HOST + list(zip(ordered, ordered[1:])) + list(zip(vals, vals[1:]))
    flat = [v for p in EDGES for v in p]
    pairs += [(a, b) for a in flat for b in flat]
    wrong = [(a, b) for a, b in pairs if OV.compare(OV.from_json(a), OV.from_json(b)) != R.sign(a, b)]
    assert wrong == []
    # the order is one: antisymmetric everywhere, and sorting by it leaves no neighbour out of place
    assert all(R.sign(a, b) == -R.sign(b, a) for a, b in pairs)
    assert all(R.sign(a, b) < 0 for a, b in zip(ordered, ordered[1:]))


# ---------------------------------------------------------------------------------------------------------------- a. order edges
@pytest.mark.parametrize("backend", BACKENDS)
def test_order_edges_on_the_device(backend):
    """one review per pair; the relations that hold come from the reference, the oracle is compared as well"""
    c, oc = load_layouts(backend, ["RootRoot"])
    rv = U.reviews([U.pod([], "o%d" % i, minReplicas=a, maxReplicas=b) for i, (a, b) in enumerate(EDGES)])
    assert_parity(c, oc, rv)
    ev = raw(c, rv)
    assert ev.host_evaluated == [] and not ev.too_big_reviews()      # a pair that leaves the device tests nothing
    for i, (a, b) in enumerate(EDGES):
        assert device_kinds(c, ev, i) == [PREFIX + "RootRoot" + r for r in R.relations(a, b)], (a, b)
    assert {R.sign(a, b) for a, b in EDGES} == {-1, 0, 1}
    # inexact numbers: the host evaluator's answer, which is the reference's as well
    rv = U.reviews([U.pod([], "h%d" % i, minReplicas=a, maxReplicas=b) for i, (a, b) in enumerate(EDGES_HOST)])
    assert_parity(c, oc, rv)
    ev = raw(c, rv)
    assert ev.host_evaluated == list(range(len(EDGES_HOST))) and not ev.too_big_reviews()
    for i, (a, b) in enumerate(EDGES_HOST):
        assert device_kinds(c, ev, i) == [PREFIX + "RootRoot" + r for r in R.relations(a, b)], (a, b)


# ---------------------------------------------------------------------------------------------------------------- b. ranks beyond 8 bits
GK_VID_FIRST = 6          # (plan.hpp: the first id of an interned value; ranks count from it)
WIDE = (8, 18)            # containers x ports per container of a wide pod: 144 ports, 288 values
WIDE_CAP = (8, 144, 8)    # ... and the element capacity that keeps them in LDS: 144 ports at nesting level 1
# The device numbers the elements of one array path within a review with 8 bits (plan.hpp RF_TOO_BIG: more than 255 ports in one pod
# go to the host evaluator), and the accumulators of 64 reviews must fit a CU's 160 KiB of LDS (kernels.hip dev_plan_create: about
# 768 B per port of capacity for these plans).  16 containers x 20 ports -- 320 ports, 640 values -- is therefore NOT a case for the
# device: it is kept below as one the host answers.  8 x 18 is: 288 values and two volumes, ranks 6 .. 295.
LDS_ROOM = 128 * 1024


def wide_pods(shape=WIDE):
    """three pods over the same values, v[0] < v[1] < ..: `up` pairs v[i] with v[i + n / 2] as (containerPort, hostPort) and holds
    two volumes above every value, `down` is its mirror image with two volumes below every value, `mix` pairs v[i] with v[i + 3] -- the larger
    one first in every other pair -- with two volumes among the largest values.  In `up` no `>` and no `>=` holds anywhere, in `down`
    no `<` and no `<=`: a rank cut to its low 8 bits turns v[100] < v[244] into 106 > 250 - 256 and is seen in the raw bitmaps, not
    only in the messages."""
    n = 2 * shape[0] * shape[1]
    v = sorted(wide_values()[:n], key=functools.cmp_to_key(R.sign))
    h = n // 2
    rng = random.Random(RANK_SEED)
    up = P.ports_pod(rng, "up", [(v[i], v[i + h]) for i in range(h)], shape[0], ["~volume-a", "~volume-bcdefgh"])
    down = P.ports_pod(rng, "down", [(v[i + h], v[i]) for i in range(h)], shape[0], [-10 ** 15, -10 ** 15 - 0.5])
    near = [(v[6 * j + t], v[6 * j + 3 + t]) for j in range(n // 6) for t in range(3)] + [(v[k], v[k + n % 6 // 2]) for k in range(n - n % 6, n - n % 6 // 2)]
    mix = P.ports_pod(rng, "mix", [(b, a) if i % 2 else (a, b) for i, (a, b) in enumerate(near)], shape[0], [v[-3], v[-30]])
    return [up, down, mix]


def ports(o, containers=None):
    return [p for c in (o["spec"]["containers"] if containers is None else containers) for p in c.get("ports", [])]


def ref_kinds(layout, o):
    """the constraints of one layout a pod violates, from the reference over its elements"""
    if layout == "TwoMembers":
        signs = {R.sign(p["containerPort"], p["hostPort"]) for p in ports(o) if "containerPort" in p and "hostPort" in p}
    elif layout == "PackedOuter":
        signs = {R.sign(p["containerPort"], v["port"]) for v in o["spec"].get("volumes", []) if "port" in v for p in ports(o) if "containerPort" in p}
    else:
        assert layout == "SelfJoin"
        cs = o["spec"]["containers"]
        signs = {R.sign(p1["containerPort"], p2["containerPort"]) for i in range(len(cs)) for j in range(len(cs)) if i != j
                 for p1 in ports(o, [cs[i]]) if "containerPort" in p1 for p2 in ports(o, [cs[j]]) if "containerPort" in p2}
    return sorted(PREFIX + layout + r for r, f in R.RELATIONS.items() if any(f(s) for s in signs))


def test_wide_pods_hold_ranks_beyond_8_bits():
    """the conditions of the device test below, from the value list: in every pod compared pairs with both ranks above 255 or pairs that
    straddle 255 (both kinds among the three), and pairs whose order flips when a rank keeps its low 8 bits only"""
    both, straddle = 0, 0
    for o in wide_pods():
        vals = {json.dumps(x): x for p in ports(o) for x in (p["containerPort"], p["hostPort"])}
        vals.update((json.dumps(x["port"]), x["port"]) for x in o["spec"]["volumes"])
        vals = sorted(vals.values(), key=functools.cmp_to_key(R.sign))
        assert len(vals) == 2 * WIDE[0] * WIDE[1] + (0 if o["metadata"]["name"] == "mix" else 2)
        assert all(R.sign(a, b) < 0 for a, b in zip(vals, vals[1:]))          # pairwise different: one rank each
        rank = {json.dumps(x): GK_VID_FIRST + i for i, x in enumerate(vals)}
        compared = [(rank[json.dumps(p["containerPort"])], rank[json.dumps(p["hostPort"])]) for p in ports(o)]
        compared += [(rank[json.dumps(p["containerPort"])], rank[json.dumps(x["port"])]) for x in o["spec"]["volumes"] for p in ports(o)]
        both += sum(1 for a, b in compared if a > 255 and b > 255)
        straddle += sum(1 for a, b in compared if min(a, b) <= 255 < max(a, b))
        assert any((a < b) != ((a & 255) < (b & 255)) for a, b in compared[:len(ports(o))])      # ... among the TwoMembers pairs
        assert any((a < b) != ((a & 255) < (b & 255)) for a, b in compared[len(ports(o)):])      # ... and among PackedOuter's
    assert both >= 10 and straddle >= 10
    up, down, mix = wide_pods()
    assert ref_kinds("TwoMembers", up) == [PREFIX + "TwoMembers" + r for r in ("Le", "Lt")] == [k.replace("PackedOuter", "TwoMembers") for k in ref_kinds("PackedOuter", up)]
    assert ref_kinds("PackedOuter", down) == [PREFIX + "PackedOuter" + r for r in ("Ge", "Gt")] == [k.replace("TwoMembers", "PackedOuter") for k in ref_kinds("TwoMembers", down)]
    assert len(ref_kinds("TwoMembers", mix)) == 4


@pytest.mark.parametrize("backend", BACKENDS)
def test_ranks_beyond_8_bits(backend):
    c, oc = load_layouts(backend, ["TwoMembers", "PackedOuter"], elem_cap=WIDE_CAP)
    objs = wide_pods()
    rv = U.reviews(objs)
    assert_parity(c, oc, rv)
    ev = raw(c, rv)
    assert ev.host_evaluated == [] and not ev.too_big_reviews() and ev.n_overflow == 0 and 0 < ev.lds_bytes <= LDS_ROOM
    for i, o in enumerate(objs):
        assert device_kinds(c, ev, i) == sorted(ref_kinds("TwoMembers", o) + ref_kinds("PackedOuter", o)), o["metadata"]["name"]
    # 16 containers x 20 ports: more ports than the device numbers -- the host evaluator's answer, which is the reference's as well
    c, oc = load_layouts(backend, ["TwoMembers", "PackedOuter"])
    objs = wide_pods((16, 20))
    rv = U.reviews(objs)
    assert_parity(c, oc, rv)
    ev = raw(c, rv)
    assert ev.host_evaluated == [0, 1, 2] and not ev.too_big_reviews()
    for i, o in enumerate(objs):
        assert device_kinds(c, ev, i) == sorted(ref_kinds("TwoMembers", o) + ref_kinds("PackedOuter", o)), o["metadata"]["name"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_self_join_on_a_cut_of_the_wide_pods(backend):
    """phase 2 of a self-join is quadratic: 6 containers x 6 ports of each wide pod, plus one pod in which all ports of a container
    agree and the containers ascend, and one in which all ports agree -- `<=` and `>=` alone"""
    c, oc = load_layouts(backend, ["SelfJoin"], elem_cap=(8, 36, 8))
    objs = []
    for o in wide_pods():
        cut = [dict(k, ports=k["ports"][:6]) for k in o["spec"]["containers"][:6]]
        objs.append(U.pod(cut, o["metadata"]["name"] + "-cut"))
    v = sorted(wide_values(), key=functools.cmp_to_key(R.sign))
    objs.append(U.pod([{"name": "c%d" % i, "image": "i", "ports": [{"name": "a", "containerPort": v[100 * i + 50]}] * 2} for i in range(6)], "steps"))
    objs.append(U.pod([{"name": "c%d" % i, "image": "i", "ports": [{"name": "a", "containerPort": v[300]}]} for i in range(3)], "equal"))
    rv = U.reviews(objs)
    assert_parity(c, oc, rv)
    ev = raw(c, rv)
    assert ev.host_evaluated == [] and not ev.too_big_reviews() and ev.n_overflow == 0
    for i, o in enumerate(objs):
        assert device_kinds(c, ev, i) == ref_kinds("SelfJoin", o), o["metadata"]["name"]
    assert ref_kinds("SelfJoin", objs[-1]) == [PREFIX + "SelfJoin" + r for r in ("Ge", "Le")]


# ---------------------------------------------------------------------------------------------------------------- c. large variant, empty loops
SMALL_CAP = (4, 4, 4)
C_LAYOUTS = ["TwoMembers", "PackedOuter", "SelfJoin", "Negated", "Mixed"]


def overflow_batch(wide=(12, 6)):
    """70 reviews under an element capacity of 4: pods that fit, two pods of 12 containers x 6 ports that do not (or of `wide`), and
    pods in which a loop around an ordering literal has nothing to walk -- no `volumes` member, `volumes: []`, containers with `ports: []`"""
    rng = random.Random(31)
    objs = []
    for i in range(70):
        k = i % 7
        if k in (0, 1, 2):
            o = U.random_pod(rng, "fit%d" % i)
        elif k == 3:
            o = P.wide_pod(rng, "wide%d" % i, *(wide if i in (3, 45) else (3, 1)), minReplicas=rng.choice(U.POOL), maxReplicas=rng.choice(U.POOL))
        elif k == 4:
            o = P.wide_pod(rng, "novol%d" % i, 1 + i % 3, 2 + i % 2)
            del o["spec"]["volumes"]
        elif k == 5:
            o = P.wide_pod(rng, "emptyvol%d" % i, 2 + i % 3, 3, volumes=[])
        else:
            o = P.wide_pod(rng, "noports%d" % i, 3, 2)
            for cont in o["spec"]["containers"][:(3 if i % 2 else 2)]:
                cont["ports"] = []
        objs.append(o)
    return objs


# The bytecode interpreter, which the large variant runs on both device backends, walks a self-join over the 72 ports of a 12 x 6 pod in
# 4.3 s per evaluation on the MI355X (profiles/value_order.md; every other layout of this plan: 25 ms).  The self-join therefore sees
# the whole batch with 6 x 2 pods in their place (still beyond the capacity: asserted), with every comparison of this case, and the
# 12 x 6 pods in ONE evaluation of its own below.
C_PLANS = {"joins": (["TwoMembers", "PackedOuter", "Negated", "Mixed"], (12, 6)), "self-join": (["SelfJoin"], (6, 2))}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("plan", sorted(C_PLANS))
def test_large_variant_empty_loops_and_the_resident_variant(backend, plan):
    layouts, wide = C_PLANS[plan]
    c, oc = load_layouts(backend, layouts, elem_cap=SMALL_CAP)
    rv = U.reviews(overflow_batch(wide))
    assert assert_parity(c, oc, rv) > 100
    plain = raw(c, rv)
    assert plain.n_overflow >= 2                   # the wide pods take the large variant, or this case shows nothing
    assert plain.host_evaluated == [] and not plain.too_big_reviews()
    resident = raw(c, rv, resident=True)           # a plan variant sized for the table's largest arrays
    assert resident.host_evaluated == [] and words(resident) == words(plain)


@pytest.mark.parametrize("backend", BACKENDS)
def test_self_join_of_12_by_6_pods_in_the_large_variant(backend):
    """one evaluation, its raw words against the oracle's pairs"""
    c, oc = load_layouts(backend, ["SelfJoin"], elem_cap=SMALL_CAP)
    objs = overflow_batch()
    rv = U.reviews([o for o in objs if o["metadata"]["name"] in ("wide3", "wide45")] + objs[:6])
    ev = raw(c, rv)
    assert ev.n_overflow >= 2 and ev.host_evaluated == [] and not ev.too_big_reviews()
    want = oracle_pairs(c, oc, rv, [None] * len(rv))
    assert set(ev.pairs("viol")) == want and ev.pairs("err") == [] and len({r for _, r in want}) >= 3


# ---------------------------------------------------------------------------------------------------------------- d. ingest paths
NAMESPACES = {"team-a": P.namespace("team-a", env="prod", tier="gold"), "team-b": P.namespace("team-b", env="dev")}
NS_REGO = '''package k
violation[{"msg": msg}] {
  input.review.namespaceObject.metadata.labels.env == "prod"
  s := input.review.object.spec
  s.minReplicas < s.maxReplicas
  msg := sprintf("prod: min %v below max %v", [s.minReplicas, s.maxReplicas])
}
'''


def ingest_objects():
    """the 40 objects, dealt into two labelled Namespaces: every review carries its Namespace, so that the rows memoised per Namespace
    sit next to the review's ranked rows"""
    return P.in_namespaces(U.layout_objects(seed=5, n=39), sorted(NAMESPACES))


def load_ingest(backend):
    c, oc = load_layouts(backend, ["TwoMembers", "RootRoot"])
    t, k = U.tmpl("K8sOrdNs", NS_REGO), U.cons("K8sOrdNs")
    k["spec"] = {"match": {"namespaceSelector": {"matchExpressions": [{"key": "env", "operator": "Exists"}]}}}
    c.AddTemplate(t), oc.add_template(t), c.AddConstraint(k), oc.add_constraint(k)
    return c, oc


def native_array(rins):
    arr = (L.gk_review_in * len(rins))()
    for a, r in zip(arr, rins):
        D.Engine._fill(a, r)
    return arr


def oracle_pairs(c, oc, rv, nss, ep=D.AUDIT_EP):
    """{(constraint id, review)} of the oracle's violations"""
    ids = {(cons.get("kind"), cons["metadata"]["name"]): cid for cid, (cons, _, _) in c._active(ep).items()}
    return {(ids[(x.constraint["kind"], x.constraint["metadata"]["name"])], i) for i, r in enumerate(rv) for x in oc.review(to_oracle_review(r), ep, nss[i])}


@pytest.mark.parametrize("backend", BACKENDS)
def test_ingest_paths_agree(backend, tmp_path):
    c, oc = load_ingest(backend)
    eng = c.driver.engine
    objs = ingest_objects()
    nss = [NAMESPACES[o["metadata"]["namespace"]] for o in objs]
    rv = P.reviews(objs, nss)
    assert assert_parity(c, oc, rv, namespaces=nss) > 100
    want = oracle_pairs(c, oc, rv, nss)
    assert any(c._active(D.AUDIT_EP)[cid][0]["kind"] == "K8sOrdNs" for cid, _ in want)
    rins = [D.to_review_in(r, ns) for r, ns in zip(rv, nss)]
    seen = {}

    def take(name, table):
        try:
            ev = table.eval()
            assert ev.host_evaluated == [] and not ev.too_big_reviews(), name
            assert set(ev.pairs("viol")) == want and ev.pairs("err") == [], name
            seen[name] = words(ev)
        finally:
            table.free()

    take("table", eng.create_table(rins, keep_docs=False))
    take("table-docs", eng.create_table(rins, keep_docs=True))
    arr = native_array(rins)
    take("native", eng.create_table_native(arr, len(rins)))
    take("native-text", eng.create_table_native(arr, len(rins), resident=True, keep_text=True))
    take("pruned", eng.create_table_native(arr, len(rins), pruned=True))
    take("pruned-text", eng.create_table_native(arr, len(rins), resident=True, keep_text=True, pruned=True))
    # the spool: pkg/audit's files, the Namespaces from the cache
    for ns in NAMESPACES.values():
        c.AddData(ns)
    for lo in range(0, len(objs), 16):
        d = tmp_path / ("Pod_%d" % (lo // 16))
        d.mkdir()
        for i, o in enumerate(objs[lo:lo + 16]):
            (d / ("%d" % i)).write_text(json.dumps(o))
    table, info = eng.create_table_spool(str(tmp_path), "Pod", 3)
    assert info["n_reviews"] == len(objs) and info["names"] == ["Pod_%d/%d" % (i // 16, i % 16) for i in range(len(objs))]
    take("spool", table)
    for ns in NAMESPACES.values():
        c.RemoveData(ns)
    assert len(set(seen.values())) == 1, sorted(seen)          # one review shape: the same words on every path
    # AdmissionRequests: every object against the next one as its oldObject
    urv = P.update_reviews(objs, nss)
    assert assert_parity(c, oc, urv, D.GATOR_EP, namespaces=nss) > 100
    ev = raw(c, urv, nss)
    assert ev.host_evaluated == [] and set(ev.pairs("viol")) == oracle_pairs(c, oc, urv, nss, D.GATOR_EP)


def audit_from_cache_agrees(c, oc):
    """tests/test_resident.py: one sweep over everything AddData'd against the oracle's serial loop -> (results, the sweep's figures)"""
    got, sweep = c.AuditFromCache()
    ns_map = {o["metadata"]["name"]: o for o in c.cached.values() if o.get("kind") == "Namespace"}
    n = 0
    for path, o in c.cached.items():
        ns = ns_map.get(o["metadata"].get("namespace") or "")
        want = oc.review(to_oracle_review(D.AugmentedUnstructured(D.Unstructured(o), ns, "")), D.AUDIT_EP, ns)
        assert not isinstance(got[path], Exception), (path, got[path])
        assert sorted(key(r) for r in got[path]) == sorted(key(r) for r in want), path
        n += len(want)
    return n, sweep


@pytest.mark.parametrize("backend", BACKENDS)
def test_resident_set_with_ordering_templates(backend):
    c, oc = load_ingest(backend)
    objs = ingest_objects()
    for o in list(NAMESPACES.values()) + objs:
        c.AddData(o), oc.add_data(o)
    n0, s0 = audit_from_cache_agrees(c, oc)
    assert n0 > 100 and s0["flattened"] == len(objs) + 2 and s0["beyond_limits"] == 0
    # one object replaced: the larger value first where the smaller one was
    old = objs[0]
    new = json.loads(json.dumps(old))
    new["spec"].update(minReplicas="zz", maxReplicas="zzz")
    new["spec"]["containers"][0]["ports"][0].update(containerPort=-1, hostPort=-0.5)
    c.AddData(new), oc.add_data(new)
    path = D.process_data(new)
    assert c.driver.ResidentReview(path) is None                # (changed since the sweep)
    n1, s1 = audit_from_cache_agrees(c, oc)
    assert s1["flattened"] == 1 and n1 != n0
    ns = NAMESPACES[new["metadata"]["namespace"]]
    want = oc.review(to_oracle_review(D.AugmentedUnstructured(D.Unstructured(new), ns, "")), D.AUDIT_EP, ns)
    rows = c.driver.ResidentReview(path)
    assert sorted(r["msg"] for r in rows) == sorted(x.msg for x in want) and "min zz max zzz" in [r["msg"] for r in rows]


# ---------------------------------------------------------------------------------------------------------------- e. aggregation
def aggregation_objects():
    """150 objects; in every tenth one two containers share a name (review.$dup: equal message keys, equal messages)"""
    objs = U.layout_objects(seed=9, n=149)
    for o in objs[5::10]:
        cs = o["spec"]["containers"]
        if len(cs) >= 2:
            cs[1] = dict(cs[1], name=cs[0]["name"])
    return objs


def aggregate(backend, group_max):
    with plan_group_max(L.load(hostemu=backend.startswith("hostemu")), group_max):
        c, oc = load_layouts(backend, ["SelfJoin", "ElemRoot"])
        objs = aggregation_objects()
        rv = U.reviews(objs)
        table = c.driver.engine.create_table([D.to_review_in(r) for r in rv], resident=True, process="audit")
        try:
            ev = table.eval()
            assert ev.host_evaluated == [] and not ev.too_big_reviews()
            assert ev.n_plan_groups == (8 if group_max else 1)
            totals, top = table.totals(), table.topk(5)
        finally:
            table.free()
    active = c._active(D.AUDIT_EP)
    want_results, want_reviews = {cid: 0 for cid in active}, {cid: [] for cid in active}
    ids = {cons["kind"]: cid for cid, (cons, _, _) in active.items()}
    for i, r in enumerate(rv):
        for x in oc.review(to_oracle_review(r), D.AUDIT_EP):
            cid = ids[x.constraint["kind"]]
            want_results[cid] += 1
            if i not in want_reviews[cid]:
                want_reviews[cid].append(i)
    assert totals == {cid: (want_results[cid], len(want_reviews[cid])) for cid in active}
    assert sum(want_results.values()) > sum(len(v) for v in want_reviews.values()) > 300      # several results per pair
    name = lambda i: objs[i]["metadata"]["name"].encode()
    for cid in active:
        got, overflow = top[cid]
        assert not overflow and sorted(name(i) for i in got) == sorted(name(i) for i in want_reviews[cid])[:5], cid
    return totals, {int(cid): ev.viol[row].tobytes() for row, cid in enumerate(ev.constraint_ids)}


@pytest.mark.parametrize("backend", BACKENDS)
def test_totals_and_topk_in_one_plan_and_in_one_plan_group_per_constraint(backend):
    dup = [o for o in aggregation_objects() if len({k["name"] for k in o["spec"]["containers"]}) < len(o["spec"]["containers"])]
    assert len(dup) >= 5
    one = aggregate(backend, 0)
    assert aggregate(backend, 1) == one


# ---------------------------------------------------------------------------------------------------------------- f. policy changes
def both(c, oc, templates, constraints, add=True):
    if add:
        for t in templates:
            c.AddTemplate(t), oc.add_template(t)
        for k in constraints:
            c.AddConstraint(k), oc.add_constraint(k)
    else:
        for k in constraints:
            c.RemoveConstraint(k), oc.remove_constraint(k)
        for t in templates:
            c.RemoveTemplate(t), oc.remove_template(t)


@pytest.mark.parametrize("backend", BACKENDS)
def test_an_ordering_template_comes_goes_and_comes_again(backend):
    c, oc = load_both(backend, [U.tmpl("K8sEqJoin", V.EQ_REGO)], [U.cons("K8sEqJoin")])
    rv = U.reviews(U.layout_objects(seed=4, n=30))
    ordering = U.layout_templates("TwoMembers") + U.layout_templates("RootRoot"), U.layout_constraints("TwoMembers") + U.layout_constraints("RootRoot")
    n_eq = assert_parity(c, oc, rv)
    both(c, oc, *ordering)
    n_all = assert_parity(c, oc, rv)
    assert n_all > n_eq > 0 and raw(c, rv).host_evaluated == []
    both(c, oc, *ordering, add=False)
    assert assert_parity(c, oc, rv) == n_eq and raw(c, rv).host_evaluated == [] and raw(c, rv).n_constraints == 1
    both(c, oc, *ordering)
    assert assert_parity(c, oc, rv) == n_all and raw(c, rv).host_evaluated == []


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_resident_set_rebuilds_itself_when_an_ordering_template_arrives(backend):
    c, oc = load_both(backend, [U.tmpl("K8sEqJoin", V.EQ_REGO)], [U.cons("K8sEqJoin")])
    objs = U.layout_objects(seed=4, n=30)
    for o in objs:
        c.AddData(o), oc.add_data(o)
    n_eq, s0 = audit_from_cache_agrees(c, oc)
    assert n_eq > 0 and s0["flattened"] == len(objs)
    both(c, oc, U.layout_templates("TwoMembers") + U.layout_templates("RootRoot"), U.layout_constraints("TwoMembers") + U.layout_constraints("RootRoot"))
    n_all, s1 = audit_from_cache_agrees(c, oc)                  # no object added again: its ids become ranks all the same
    assert n_all > n_eq and s1["n_objects"] == len(objs) and s1["beyond_limits"] == 0


# ---------------------------------------------------------------------------------------------------------------- g. fuzz on new ground
EDGE_POOL = [v for pair in EDGES for v in pair]
FUZZ_SEEDS = [range(200, 206), range(206, 212)]


def fuzz_plan(seeds, per_seed=4, n_objs=10):
    templates, constraints, objs = [], [], []
    for seed in seeds:
        rng = random.Random(seed)
        for k in range(per_seed):
            kind = "K8sFuzz%dx%d" % (seed, k)
            templates.append(V.fuzz_template(rng, kind))
            constraints.append(U.cons(kind))
        objs += [P.random_pod(rng, "s%d-%d" % (seed, i), EDGE_POOL) for i in range(n_objs)]
    return templates, constraints, objs


def test_fuzz_plans_hold_every_relation():
    """the conditions the fuzz relies on, on the CPU: over the seeds 200..211 each of the four relations and `not` occur, and every plan
    holds pods beyond four containers and three ports"""
    bodies = []
    for seeds in FUZZ_SEEDS:
        templates, _, objs = fuzz_plan(seeds)
        bodies += [t["spec"]["targets"][0]["rego"].split("msg :=")[0] for t in templates]
        assert max(len(o["spec"]["containers"]) for o in objs) > 4 and max(len(k.get("ports", [])) for o in objs for k in o["spec"]["containers"]) > 3
    for op in ("<", "<=", ">", ">="):
        assert any(re.search(r" %s " % re.escape(op), b) for b in bodies), op
    assert any("not " in b for b in bodies)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("seeds", FUZZ_SEEDS, ids=["200", "206"])
def test_fuzz_on_the_edge_values(backend, seeds):
    templates, constraints, objs = fuzz_plan(seeds)
    c, oc = load_both(backend, templates, constraints)
    rv = U.reviews(objs)
    assert assert_parity(c, oc, rv) > 100
    ev = raw(c, rv)
    assert ev.host_evaluated == [] and not ev.too_big_reviews()
