"""Ordering comparisons between two review values (`spec.minReplicas > spec.maxReplicas`, `p1.containerPort < p2.containerPort`).
pe.cpp compare_f makes them the value-pair atom carrying its relation, lower.cpp F_VCMP + CmpOp on the slots F_VEQ uses, and the
flattener turns a review's value ids into RANKS under Rego's total order as soon as the registry holds an ordered pattern
(flatten.cpp Flattener::rank_review), so that the device relation is one unsigned compare of two ids.  Every case is compared with
the oracle -- rendered results and raw device bitmaps (parity_util.assert_parity) -- on every backend; the violation counts (the
oracle's) are pinned, and a hand-written table pins the basic pairs so that the oracle is not the only witness.  Before this the
first test's AddConstraint raised "ordering comparison between two review values"."""
import os
import random
import re
import subprocess
import sys

import pytest

import test_jit_source as J
import value_order_util as U
from gatekeeper_amd import driver as D
from parity_util import BACKENDS, assert_parity, load_both, make_client, to_oracle_review

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_evaluated(c, rv):
    table = c.driver.engine.create_table([D.to_review_in(r) for r in rv], keep_docs=False)
    try:
        ev = table.eval()
        assert not ev.too_big_reviews()
        return list(ev.host_evaluated)
    finally:
        table.free()


# ---------------------------------------------------------------------------------------------------------------- 1. the refusal that is gone
HPA_REGO = '''package k
violation[{"msg": msg}] {
  s := input.review.object.spec
  s.minReplicas > s.maxReplicas
  msg := sprintf("minReplicas %v above maxReplicas %v", [s.minReplicas, s.maxReplicas])
}
'''


def hpa(lo, hi, name="h"):
    spec = {}
    if lo is not None:
        spec["minReplicas"] = lo
    if hi is not None:
        spec["maxReplicas"] = hi
    return {"apiVersion": "autoscaling/v2", "kind": "HorizontalPodAutoscaler", "metadata": {"name": name, "namespace": "d"}, "spec": spec}


@pytest.mark.parametrize("backend", BACKENDS)
def test_min_above_max_loads_and_agrees_with_the_oracle(backend, monkeypatch):
    monkeypatch.setenv("GK_RENDER_CHECK", "1")   # (both host evaluators render the messages; a difference is an error)
    c, oc = load_both(backend, [U.tmpl("K8sMinMax", HPA_REGO)], [U.cons("K8sMinMax")])
    objs = [hpa(5, 3), hpa(3, 5), hpa(3, 3), hpa(10, 9), hpa(9, 10), hpa(None, 3), hpa(3, None), hpa(2, 1.5)]
    assert assert_parity(c, oc, U.reviews(objs)) == 3
    got = c.ReviewBatch(U.reviews(objs), D.AUDIT_EP)
    assert [r.msg for r in got[0]] == ["minReplicas 5 above maxReplicas 3"] and got[1] == [] and got[5] == [] and len(got[7]) == 1


# ---------------------------------------------------------------------------------------------------------------- 2. slot layouts
LAYOUT_COUNTS = {"RootRoot": 16, "ElemRoot": 32, "TwoMembers": 48, "PackedOuter": 50, "OldNew": 12, "SelfJoin": 72, "Negated": 28}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("layout", sorted(U.LAYOUTS))
def test_slot_layouts_all_four_relations(backend, layout, monkeypatch):
    """the four relations of a layout in one plan (they share the layout's value slots); the first object holds the LARGER value first"""
    monkeypatch.setenv("GK_RENDER_CHECK", "1")
    c, oc = load_both(backend, U.layout_templates(layout), U.layout_constraints(layout))
    objs = U.layout_objects()
    rv, ep = (U.update_reviews(objs), D.GATOR_EP) if layout == "OldNew" else (U.reviews(objs), D.AUDIT_EP)
    assert assert_parity(c, oc, rv, ep) == LAYOUT_COUNTS[layout]
    assert host_evaluated(c, rv) == []
    if layout == "RootRoot":   # minReplicas 7, maxReplicas 4 in that order in the document: `>` and `>=`, nothing else
        got = c.ReviewBatch(rv[:1], ep)[0]
        assert sorted(r.constraint["kind"] for r in got) == ["K8sOrdRootRootGe", "K8sOrdRootRootGt"]


# ---------------------------------------------------------------------------------------------------------------- 3. order semantics
LONG = 123456789012345678901234567890   # (not an int64, not a double: ROW_INEXACT)
# the twelve basic pairs, by hand: sign of compare(a, b) under Rego's total order (null < boolean < number < string < array < object)
BASIC = [(5, 3, 1), (3, 5, -1), (3, 3.0, 0), (3, 2.5, 1), ("10", 9, 1), ("10", "9", -1), (True, 1, -1), (None, False, -1),
         (-1, -2, 1), ("abcdefghij", "abcdefghii", 1), ("abc", "abcdefgh", -1), ([], "z", 1)]
# ... and pairs answered by the oracle alone
MORE = [(1.5, 1, None), (1.5, 2, None), (False, True, None), (None, None, None), ("", "a", None), ("abcdefg", "abcdefgh", None),
        ("abcdefgh", "abcdefg", None), ([], {}, None), ({}, [], None), ([], [], None), ({}, "z", None), (0, -0.5, None),
        (9007199254740993, 9007199254740992, None), (-9223372036854775808, 9223372036854775807, None), (1e300, 5, None)]
NEED_HOST = [([1], "z"), ("z", [1]), ({"a": 1}, 3), (LONG, 3), (3, LONG), (LONG, "x")]


@pytest.mark.parametrize("backend", BACKENDS)
def test_order_semantics(backend):
    c, oc = load_both(backend, U.layout_templates("RootRoot"), U.layout_constraints("RootRoot"))
    pairs = BASIC + MORE
    rv = U.reviews([U.pod([], "o%d" % i, minReplicas=a, maxReplicas=b) for i, (a, b, _) in enumerate(pairs)])
    assert assert_parity(c, oc, rv) == 54
    assert host_evaluated(c, rv) == []          # empty containers are ranked, nothing here needs the host
    got = c.ReviewBatch(rv, D.AUDIT_EP)
    for (a, b, sign), g in zip(pairs, got):
        if sign is None:
            continue
        want = {-1: ["Le", "Lt"], 0: ["Ge", "Le"], 1: ["Ge", "Gt"]}[sign]
        assert sorted(r.constraint["kind"][len("K8sOrdRootRoot"):] for r in g) == want, (a, b, g)
    # a non-empty container or an inexact number on an ordered path: answered by the host evaluator (with Rego's answer), reported so
    rv = U.reviews([U.pod([], "h%d" % i, minReplicas=a, maxReplicas=b) for i, (a, b) in enumerate(NEED_HOST)])
    assert assert_parity(c, oc, rv) == 12
    assert host_evaluated(c, rv) == list(range(len(NEED_HOST)))


# ---------------------------------------------------------------------------------------------------------------- 4. nothing else moves
EQ_REGO = '''package k
violation[{"msg": msg}] {
  p := input.review.object.spec.containers[_].ports[_]
  p.containerPort == p.hostPort
  msg := sprintf("port %v", [p.containerPort])
}
violation[{"msg": "same"}] {
  s := input.review.object.spec
  s.minReplicas == s.maxReplicas
}
'''
# GK_TABLE_DIGEST of _digest_table's table under the equality template alone, taken on the commit before ordering relations existed
PARENT_DIGEST = 9609778620673426070


def _digest_table(c):
    rins = [D.to_review_in(r) for r in U.reviews(U.layout_objects(seed=4, n=40))]
    os.environ["GK_TABLE_DIGEST"] = "1"
    try:
        t = c.driver.engine.create_table(rins, keep_docs=False)
        st = t.stats()
        t.free()
    finally:
        os.environ.pop("GK_TABLE_DIGEST", None)
    return st["digest"]


def test_tables_are_what_they_were_without_an_ordering_template():
    other = make_client("hostemu")   # an engine of the same process that DOES hold one: registries are per engine
    for t, k in zip(U.layout_templates("TwoMembers"), U.layout_constraints("TwoMembers")):
        other.AddTemplate(t)
        other.AddConstraint(k)
    c = make_client("hostemu")
    c.AddTemplate(U.tmpl("K8sEqJoin", EQ_REGO))
    c.AddConstraint(U.cons("K8sEqJoin"))
    assert _digest_table(c) == PARENT_DIGEST
    # ... and the ids DO move once an ordering relation reads the same paths (or this test would show nothing)
    for t, k in zip(U.layout_templates("TwoMembers"), U.layout_constraints("TwoMembers")):
        c.AddTemplate(t)
        c.AddConstraint(k)
    assert _digest_table(c) != PARENT_DIGEST


@pytest.mark.parametrize("backend", BACKENDS)
def test_an_ordering_template_makes_earlier_tables_stale(backend):
    """the equality join registered the paths as value paths already: the ordering relation on the SAME paths still makes the table
    flattened before it stale (its ids are in order of first occurrence); a table created again answers both templates"""
    c, oc = load_both(backend, [U.tmpl("K8sEqJoin", EQ_REGO)], [U.cons("K8sEqJoin")])
    objs = U.layout_objects(seed=4, n=12)
    rv = U.reviews(objs)
    old = c.driver.engine.create_table([D.to_review_in(r) for r in rv], keep_docs=False)
    old.eval()
    before = c.ReviewBatch(rv, D.AUDIT_EP)     # (the batcher holds a table of its own)
    for layout in ("TwoMembers", "RootRoot"):
        for t, k in zip(U.layout_templates(layout), U.layout_constraints(layout)):
            c.AddTemplate(t)
            oc.add_template(t)
            c.AddConstraint(k)
            oc.add_constraint(k)
    with pytest.raises(D.EngineError, match="create it again"):
        old.eval()
    old.free()
    # Client.Review after the policy change: the caller re-creates nothing
    for o, r, b in zip(objs, rv, before):
        want = sorted(x.msg for x in oc.review(to_oracle_review(r), D.AUDIT_EP))
        assert sorted(x.msg for x in c.Review(r, D.AUDIT_EP)) == want
        assert sorted(x.msg for x in b) == sorted(x.msg for x in oc.review(to_oracle_review(r), D.AUDIT_EP) if x.constraint["kind"] == "K8sEqJoin")
    # a table created now: the equality join on ranked ids and the ordering relations, rendered results and raw bitmaps
    assert assert_parity(c, oc, rv) == 111


# ---------------------------------------------------------------------------------------------------------------- 5. row-group geometries
def _geom(backend, rpt, **kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GK_JIT_")}
    env.update({k: str(v) for k, v in kw.items()})
    env["GK_RPT"] = str(rpt)
    if backend == "hostemu":
        env.update(GK_HOSTEMU_KERNEL="jit", GK_EMU_GRID="8")   # the emulated plan-specialised kernel, checked word by word against the interpreter
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "value_order_util.py"), "geom", backend], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.split()[-4:]


GEOM_COUNTS = ["geom", "3125", "278"]   # (violations of the whole plan | of the body that mixes an equality join with an ordering literal)


@pytest.mark.parametrize("backend", [pytest.param("hostemu", id="hostemu-gen"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")])
@pytest.mark.parametrize("rpt", [64, 128, 256])
def test_row_group_geometries(backend, rpt):
    """every layout plus the mixed body in one plan over 151 objects, against the oracle in a process of its own per geometry; at the
    sweep geometries with the join form and the DNF form on and off: the same words (both forms decline a body with an ordering literal)"""
    on = _geom(backend, rpt)
    assert on[:3] == GEOM_COUNTS
    if rpt >= 128:
        assert _geom(backend, rpt, GK_JIT_JOIN=0, GK_JIT_DNF=0) == on


# ---------------------------------------------------------------------------------------------------------------- 6. differential fuzz
SIDES = {   # a fixed menu of compared paths: name -> (the bindings it needs, its term)
    "min": ((), "input.review.object.spec.minReplicas"), "max": ((), "input.review.object.spec.maxReplicas"),
    "cnt": ((), "input.review.object.spec.maxCount"), "lim": (("c",), "c.resources.limits.count"),
    "cp": (("c", "p"), "p.containerPort"), "hp": (("c", "p"), "p.hostPort"), "vp": (("v",), "v.port"),
}
BIND = {"v": "v := input.review.object.spec.volumes[_]", "c": "c := input.review.object.spec.containers[_]", "p": "p := c.ports[_]"}


def fuzz_template(rng, kind):
    a, b = rng.sample(sorted(SIDES), 2)
    op = rng.choice(["<", "<=", ">", ">=", "<", ">", "==", "!="])
    neg = rng.random() < 0.35
    lines = [BIND[v] for v in ("v", "c", "p") if v in SIDES[a][0] + SIDES[b][0]]
    if rng.random() < 0.3 and "c" in SIDES[a][0] + SIDES[b][0]:
        lines.append('c.name != "c0"')
    lines.append("%s%s %s %s" % ("not " if neg else "", SIDES[a][1], op, SIDES[b][1]))
    head = '{"msg": "m"}' if neg else '{"msg": msg}'
    if not neg:
        lines.append('msg := sprintf("%%v %s %%v", [%s, %s])' % (op, SIDES[a][1], SIDES[b][1]))
    return U.tmpl(kind, "package k\nviolation[%s] {\n  %s\n}\n" % (head, "\n  ".join(lines)))


def run_fuzz(backend, seeds, per_seed=4, n_objs=10):
    """one plan for all the seeds' templates, one batch of objects from the pool (no container, no inexact number)"""
    templates, constraints, objs = [], [], []
    for seed in seeds:
        rng = random.Random(seed)
        for k in range(per_seed):
            kind = "K8sFuzz%dx%d" % (seed, k)
            templates.append(fuzz_template(rng, kind))
            constraints.append(U.cons(kind))
        objs += [U.random_pod(rng, "s%d-%d" % (seed, i)) for i in range(n_objs)]
    c, oc = load_both(backend, templates, constraints)   # (every generated template must compile: AddConstraint raises otherwise)
    rv = U.reviews(objs)
    total = assert_parity(c, oc, rv)
    assert host_evaluated(c, rv) == []                   # no review may be host-completed
    return total


def test_fuzz_generator_emits_ordering_relations_in_every_shape():
    """the conditions the fuzz relies on, on the CPU: ordering relations dominate, `not` and every side of the menu occur"""
    texts = [fuzz_template(random.Random(s), "K8sF")["spec"]["targets"][0]["rego"] for s in range(40)]
    assert sum(1 for t in texts if re.search(r" (<|<=|>|>=) ", t.split("msg :=")[0])) >= 20
    assert any("not " in t for t in texts) and all(any(SIDES[s][1] in t for t in texts) for s in SIDES)


@pytest.mark.parametrize("first", [0, 10, 20])
def test_fuzz_interpreter(first):
    assert run_fuzz("hostemu", range(first, first + 10)) > 100


def test_fuzz_generated_plan_code():
    assert run_fuzz("hostemu-gen", range(30, 40)) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu", "gpu-interp"])
@pytest.mark.parametrize("first", [100, 106])
def test_fuzz_device(backend, first):
    assert run_fuzz(backend, range(first, first + 6)) > 60


# ---------------------------------------------------------------------------------------------------------------- 7. hiprtc offline
def _meta_int(code, key):
    """an unsigned integer of the code object's msgpack metadata, -1 if not found (test_jit_source._scratch_bytes, any key)"""
    i = code.find(key)
    if i < 0:
        return -1
    i += len(key)
    v = code[i]
    if v < 0x80:
        return v
    return {0xCC: lambda: code[i + 1], 0xCD: lambda: int.from_bytes(code[i + 1:i + 3], "big"), 0xCE: lambda: int.from_bytes(code[i + 1:i + 5], "big")}.get(v, lambda: -1)()


@pytest.mark.parametrize("rpt", [64, 256])
def test_plan_text_compiles_for_gfx950_without_scratch_within_its_register_budget(monkeypatch, tmp_path, rpt):
    """the plan-specialised text of test 2's templates through hiprtc, no device needed: it compiles, uses no scratch, and stays within
    the VGPRs its launch bounds leave a wave (512 per SIMD over the waves per SIMD the text asks for, in granules of 8)"""
    rtc = J._hiprtc()
    if rtc is None:
        pytest.skip("libhiprtc.so is not installed")

    def run():
        for layout in sorted(U.LAYOUTS):
            c = make_client("hostemu")
            for t, k in zip(U.layout_templates(layout), U.layout_constraints(layout)):
                c.AddTemplate(t)
                c.AddConstraint(k)
            objs = U.layout_objects()
            rv, ep = (U.update_reviews(objs), D.GATOR_EP) if layout == "OldNew" else (U.reviews(objs), D.AUDIT_EP)
            c.ReviewBatch(rv, ep)
    texts = J._dump_sources(monkeypatch, tmp_path, run, env=[("GK_RPT", rpt)])
    # (layouts whose plans differ in nothing but the paths their rows come from share one text)
    assert sum(1 for _, text in texts if re.search(r"xa_ (<|<=|>|>=) xb_", text)) >= 5
    for name, text in texts:
        ok, log, code = J.compile_gfx950(rtc, text)
        assert ok, "%s does not compile for gfx950:\n%s" % (name, log[-3000:])
        _, waves = (int(x) for x in re.search(r"__launch_bounds__\((\d+), (\d+)\)", text).groups())
        budget = 512 // waves // 8 * 8   # (the second launch bound: waves per SIMD)
        assert _meta_int(code, b".private_segment_fixed_size") == 0, "%s: %d bytes of scratch per lane" % (name, _meta_int(code, b".private_segment_fixed_size"))
        assert 0 < _meta_int(code, b".vgpr_count") <= budget, "%s: %d VGPRs, budget %d" % (name, _meta_int(code, b".vgpr_count"), budget)
