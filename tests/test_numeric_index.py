"""Numeric indices into review arrays: `cs[0]`, `cs[count(cs) - 1]`, `not cs[1]`, `cs[i]; i > 0`.
pe.cpp index_elem makes `P[k]` an iteration over P with one condition on its key (Atom::KEYCMP with a number), lower.cpp a test of the loop
cursor's ordinal against the constant (cursors.hpp F_KIMM) or against the lane's own element count (F_KEND), and at sweep geometry the
generated code writes only the copy of the element the index selects (codegen_forms.hpp index_range).  Every case is compared with the
oracle -- rendered results and raw device bitmaps (parity_util.assert_parity) -- on every backend; the oracle's violation counts are
pinned, and a hand-written table pins (object, rule) pairs so that the oracle is not the only witness.  Before this the first test's
AddConstraint raised "numeric index into review data"."""
import os
import random
import re
import subprocess
import sys

import pytest

import numeric_index_util as U
import test_jit_source as J
import test_result_totals as RT
import test_self_join_plan_text as PT
from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from parity_util import BACKENDS, assert_parity, load_both, make_client, to_oracle_review
from test_value_order import _meta_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- 1. loads and agrees
@pytest.mark.parametrize("backend", BACKENDS)
def test_indexed_rules_load_and_agree_with_the_oracle(backend, monkeypatch):
    monkeypatch.setenv("GK_RENDER_CHECK", "1")   # (both host evaluators render the messages; a difference is an error)
    c, oc = load_both(backend, U.rule_templates(), U.rule_constraints())
    objs = U.basic_objects()
    rv = U.reviews(objs)
    assert assert_parity(c, oc, rv) == 23
    # the OBJECT with a member "0" sits where the plan iterates elements: beyond the device, answered by the host evaluator, reported so
    host, big, _ = U.result_words(c, rv)
    assert host == [len(objs) - 1] and big == []
    got = c.ReviewBatch(rv, D.AUDIT_EP)
    for (name, rule), want in sorted(U.BY_HAND.items()):
        g = got[[o["metadata"]["name"] for o in objs].index(name)]
        assert any(r.constraint["kind"] == U.kind_of(rule) for r in g) == want, (name, rule, g)
    by_name = {o["metadata"]["name"]: g for o, g in zip(objs, got)}
    assert sorted(r.msg for r in by_name["three"] if r.constraint["kind"] == "K8sIdxLater") == ["container 1 runs pause"]
    assert [r.msg for r in by_name["one"] if r.constraint["kind"] == "K8sIdxFirst"] == ["first container main runs bad/a"]
    assert [r.constraint["kind"] for r in by_name["object-with-0"]] == ["K8sIdxNoSecond"]   # (a numeric index into an object is undefined)


# ---------------------------------------------------------------------------------------------------------------- 2. capacity edges
def _edge(rule, path, index):
    return U.tmpl("K8sEdge" + rule, 'package k\nviolation[{"msg": "%s"}] {\n  a := input.review.object.spec.%s\n  a[%s]%s == "x"\n}\n' % (
        rule, path, index, ".name" if path == "containers" else ""))


EDGE_RULES = {"A7": ("args", "7"), "A8": ("args", "8"), "AEnd": ("args", "count(a) - 1"), "A255": ("args", "255"), "A256": ("args", "256"),
              "C7": ("containers", "7"), "C8": ("containers", "8"), "CEnd": ("containers", "count(a) - 1"), "CEnd2": ("containers", "count(a) - 2")}


def edge_objects():
    """arrays of 8 and 9 elements (the default capacity of a top-level scope is 8) with the "x" at 6, 7, 8 or nowhere, in `args` and in
    `containers`; then `args` of 256 elements -- beyond the device's 255 -- with the "x" last, and of 257 with the "x" at 256"""
    objs = []
    for n in (8, 9):
        for at in (6, 7, 8, None):
            if at is not None and at >= n:
                continue
            marks = ["x" if i == at else "y%d" % i for i in range(n)]
            objs.append(U.pod([{"name": m, "image": "i"} for m in marks], "n%d-at%s" % (n, at), args=marks))
    objs.append(U.pod([], "long-256", args=["y"] * 255 + ["x"]))
    objs.append(U.pod([], "long-257", args=["y"] * 256 + ["x"]))
    return objs


@pytest.mark.parametrize("backend", BACKENDS)
def test_capacity_edges(backend):
    templates = [_edge(r, *EDGE_RULES[r]) for r in sorted(EDGE_RULES)]
    c, oc = load_both(backend, templates, [U.cons("K8sEdge" + r) for r in sorted(EDGE_RULES)])
    objs = edge_objects()
    rv = U.reviews(objs)
    # a table that is not resident: default capacities, the nine-element arrays take the large-capacity path
    assert assert_parity(c, oc, rv) == 16   # (by hand: 1 + 4 + 0 + 0 + 3 + 4 + 0 + 2 + 2)
    host, big, _ = U.result_words(c, rv)
    assert host == [len(objs) - 2, len(objs) - 1] and big == []     # (more than 255 elements: the host evaluator, with Rego's answer)
    got = {o["metadata"]["name"]: sorted(r.msg for r in g) for o, g in zip(objs, c.ReviewBatch(rv, D.AUDIT_EP))}
    assert got["n8-at7"] == ["A7", "AEnd", "C7", "CEnd"] and got["n9-at8"] == ["A8", "AEnd", "C8", "CEnd"] and got["n9-at7"] == ["A7", "C7", "CEnd2"]
    assert got["n8-atNone"] == [] and got["long-256"] == ["A255", "AEnd"]
    # (index 256 is never defined on the device -- the 256-element array has none, the plan folds the test to false -- and the 257-element
    #  array, where Rego defines it, is the host evaluator's)
    assert got["long-257"] == ["A256", "AEnd"]
    # the same pods in a RESIDENT table, whose capacities are fitted to them
    table = c.driver.engine.create_table([D.to_review_in(r) for r in rv], keep_docs=False, resident=True)
    try:
        ev = table.eval()
        active = {cid: cons.get("kind") for cid, (cons, _, _) in c._active(D.AUDIT_EP).items()}
        dev = {(active[cid][len("K8sEdge"):], objs[r]["metadata"]["name"]) for cid, r in ev.pairs("viol") if cid in active}
        assert not ev.too_big_reviews()
    finally:
        table.free()
    assert dev == {(m, name) for name, msgs in got.items() for m in msgs}


# ---------------------------------------------------------------------------------------------------------------- 3. row-group geometries
def _script(backend, what, *args, **env_kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GK_JIT_")}
    env.update({k: str(v) for k, v in env_kw.items()})
    if backend == "hostemu":
        env.update(GK_HOSTEMU_KERNEL="jit", GK_EMU_GRID="8")   # the emulated plan-specialised kernel, checked word by word against the interpreter
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "numeric_index_util.py"), what, backend] + [str(a) for a in args],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.split()


GEOM = ["geom", "264", "65329ac24212fb2abb7d33bebbdbfed282274ade1b0232aa24a9c1aa546dbd48"]   # (the oracle's count | the raw result words)


@pytest.mark.parametrize("backend", [pytest.param("hostemu", id="hostemu-gen"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")])
@pytest.mark.parametrize("rpt", [64, 128, 256])
def test_row_group_geometries(backend, rpt):
    """the whole rule set in one plan over 150 objects, against the oracle in a process of its own per geometry: the same words at every
    geometry (the indexed form of a loop exists at the sweep geometries only)"""
    assert _script(backend, "geom", GK_RPT=rpt)[-3:] == GEOM


# ---------------------------------------------------------------------------------------------------------------- 4. nothing else moves
def _configs2_text(client, drv, out_dir, n=1024):
    for f in os.listdir(str(out_dir)):
        os.remove(os.path.join(str(out_dir), f))
    batch = synth.NativeBatch(drv.engine.lib, n, seed=synth.SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
    table = drv.engine.create_table_native(batch.reviews, n, keep_docs=False, resident=True)
    table.launch()
    table.eval(download=True, collect_only=True)
    table.free()
    return sorted(open(os.path.join(str(out_dir), f)).read() for f in os.listdir(str(out_dir)) if f.startswith("gk_plan_"))


def test_other_plans_keep_their_text_around_an_indexed_template(monkeypatch, tmp_path):
    """configs[2]'s policy, then an indexed template added and removed: the plan that remains is byte for byte the plan of before"""
    monkeypatch.setenv("GK_HOSTEMU_KERNEL", "jit")
    monkeypatch.setenv("GK_EMU_HIP_SOURCE_DIR", str(tmp_path))
    monkeypatch.setenv("GK_EMU_GRID", "8")
    fx = synth.load_fixtures()
    drv = D.Driver(device=0, hostemu=True)
    client = D.Client(drv)
    templates, constraints = PT._policy(2, fx)
    for t in templates:
        client.AddTemplate(t)
    for k in constraints:
        client.AddConstraint(k)
    before = _configs2_text(client, drv, tmp_path)
    assert before and not any(re.search(r"e\d+ == 0u\)", t) for t in before)
    t, k = U.rule_templates(["First"])[0], U.rule_constraints(["First"])[0]
    client.AddTemplate(t)
    client.AddConstraint(k)
    with_index = _configs2_text(client, drv, tmp_path)
    assert with_index != before and any(re.search(r"e\d+ == 0u\)", t) for t in with_index)   # (the index test of F_KIMM, in its one copy)
    client.RemoveConstraint(k)
    client.RemoveTemplate(t)
    assert _configs2_text(client, drv, tmp_path) == before


# ---------------------------------------------------------------------------------------------------------------- 5. refusals that remain
REFUSED = {
    "numeric index into a nested array": ['input.review.object.spec.containers[_].ports[0].containerPort == 80',
                                          'p := input.review.object.spec.containers[_].ports[i]\n  i > 0\n  p.containerPort == 80',
                                          'c := input.review.object.spec.containers[_]\n  c.ports[count(c.ports) - 1].containerPort == 80',
                                          'input.review.object.spec.rules[_].http.paths[0].path == "/"'],
    r"arithmetic '\+' on review data": ['cs := input.review.object.spec.containers\n  cs[i].image == "a"\n  cs[i + 1].image == "b"'],
    "index counted on another review value": ['cs := input.review.object.spec.containers\n  cs[count(input.review.object.spec.volumes) - 1].image == "b"'],
    "review data indexed by a symbolic key": ['cs := input.review.object.spec.containers\n  cs[input.review.object.spec.n].image == "b"'],
}


@pytest.mark.parametrize("message", sorted(REFUSED))
def test_refusals_that_remain(message):
    for body in REFUSED[message]:
        c = make_client("hostemu")
        c.AddTemplate(U.tmpl("K8sRefused", 'package k\nviolation[{"msg": "m"}] {\n  %s\n}\n' % body))
        with pytest.raises(D.UnsupportedError, match="unsupported on the device plan: " + message):
            c.AddConstraint(U.cons("K8sRefused"))


def test_constants_that_are_no_index_are_undefined_not_refused():
    """a negative, fractional or non-numeric constant, an index at or beyond the end counted from it, an index beyond the device's 255"""
    bodies = ['input.review.object.spec.containers[-1].image == "nginx"', 'input.review.object.spec.containers[1.5].image == "nginx"',
              'cs := input.review.object.spec.containers\n  cs[count(cs)].image == "nginx"', 'cs := input.review.object.spec.containers\n  cs[count(cs) - 0].image == "nginx"',
              'cs := input.review.object.spec.containers\n  cs[count(cs) - 5].image == "nginx"', 'input.review.object.spec.containers[300].image == "nginx"',
              'input.review.object.spec.containers[i].image == "nginx"\n  i == "0"', 'input.review.object.spec.containers[i].image == "nginx"\n  i == 0.5']
    templates = [U.tmpl("K8sNever%d" % i, 'package k\nviolation[{"msg": "m"}] {\n  %s\n}\n' % b) for i, b in enumerate(bodies)]
    c, oc = load_both("hostemu", templates, [U.cons("K8sNever%d" % i) for i in range(len(bodies))])
    assert assert_parity(c, oc, U.reviews(U.basic_objects()[:-1])) == 0


# ---------------------------------------------------------------------------------------------------------------- 6. RESULT totals
@pytest.mark.parametrize("backend", BACKENDS)
def test_result_totals_of_indexed_rules(backend):
    """gk_table_totals against the oracle's per-constraint result counts (test_result_totals.run_totals asserts the equality): an indexed
    binding yields at most one result, `cs[i]; i > 0` one per element"""
    templates = {U.kind_of(r): ("package k\n" + U.RULES[r], {}) for r in U.KINDS}
    objs = U.basic_objects() + [U.pod([U.ctr("a", "pause"), U.ctr("b", "pause"), U.ctr("c", "pause"), U.ctr("sidecar", "pause")], "pauses")]
    refused, want, want_pairs, _, _ = RT.run_totals(backend, templates, objs)
    assert refused == set()
    assert want == {"K8sIdxArgs": 2, "K8sIdxDiffer": 3, "K8sIdxFirst": 1, "K8sIdxLast": 5, "K8sIdxLater": 8, "K8sIdxNoSecond": 4, "K8sIdxPorts": 2, "K8sIdxTwice": 2}
    assert want["K8sIdxLater"] > len(want_pairs["K8sIdxLater"]) and want["K8sIdxFirst"] == len(want_pairs["K8sIdxFirst"])


# ---------------------------------------------------------------------------------------------------------------- 7. hiprtc offline
@pytest.mark.parametrize("rpt", [64, 256])
def test_plan_text_compiles_for_gfx950_without_scratch_within_its_register_budget(monkeypatch, tmp_path, rpt):
    """the plan-specialised text of test 1's templates through hiprtc, no device needed: it compiles, uses no scratch, and stays within
    the VGPRs its launch bounds leave a wave (512 per SIMD over the waves per SIMD the text asks for, in granules of 8)"""
    rtc = J._hiprtc()
    if rtc is None:
        pytest.skip("libhiprtc.so is not installed")

    def run():
        c = make_client("hostemu")
        for t, k in zip(U.rule_templates(), U.rule_constraints()):
            c.AddTemplate(t)
            c.AddConstraint(k)
        c.ReviewBatch(U.reviews(U.basic_objects()), D.AUDIT_EP)
    texts = J._dump_sources(monkeypatch, tmp_path, run, env=[("GK_RPT", rpt)])
    assert any(re.search(r"e\d+ == 0u\)", text) for _, text in texts) and any(re.search(r"e\d+ \+ 1u == ", text) for _, text in texts)
    for name, text in texts:
        ok, log, code = J.compile_gfx950(rtc, text)
        assert ok, "%s does not compile for gfx950:\n%s" % (name, log[-3000:])
        _, waves = (int(x) for x in re.search(r"__launch_bounds__\((\d+), (\d+)\)", text).groups())
        budget = 512 // waves // 8 * 8   # (the second launch bound: waves per SIMD)
        assert _meta_int(code, b".private_segment_fixed_size") == 0, "%s: %d bytes of scratch per lane" % (name, _meta_int(code, b".private_segment_fixed_size"))
        assert 0 < _meta_int(code, b".vgpr_count") <= budget, "%s: %d VGPRs, budget %d" % (name, _meta_int(code, b".vgpr_count"), budget)


def test_an_indexed_loop_is_one_copy_at_sweep_geometry(monkeypatch, tmp_path):
    """`cs[0]` with a string test: the unrolled text holds the body for element 0 alone, where `cs[_]` holds one copy per element of the capacity"""
    def text_of(index):
        rego = 'package k\nviolation[{"msg": "m"}] {\n  c := input.review.object.spec.containers[%s]\n  startswith(c.image, "bad/")\n  c.name == "main"\n}\n' % index
        sub = tmp_path / ("t" + index.strip("_"))
        sub.mkdir()

        def run():
            c = make_client("hostemu")
            c.AddTemplate(U.tmpl("K8sOne", rego))
            c.AddConstraint(U.cons("K8sOne"))
            c.ReviewBatch(U.reviews(U.basic_objects()[:-1]), D.AUDIT_EP)
        texts = J._dump_sources(monkeypatch, sub, run, env=[("GK_RPT", 256)])
        assert len(texts) == 1
        return texts[0][1].split("void jit_formula_part")[1]
    indexed, iterated = text_of("0"), text_of("_")
    copies = lambda t: len(re.findall(r"constexpr uint32_t e0 = \d+u;", t))   # noqa: E731
    assert copies(indexed) == 1 and "constexpr uint32_t e0 = 0u;" in indexed
    assert copies(iterated) == 0 or copies(iterated) >= 4   # (the iterated body is a conjunction: one masked compare per element, or a copy each)
    assert len(re.findall(r"W\d+_\d+ = acc\.load", indexed)) == 1


# ---------------------------------------------------------------------------------------------------------------- 8. differential fuzz
def test_fuzz_generator_emits_every_form():
    texts = [U.fuzz_template(random.Random(s), "K8sF")["spec"]["targets"][0]["rego"] for s in range(80)]
    for needle in (r"containers\[\d\]\n", r"count\(cs\) - \d", r"\bi (==|!=|<|<=|>|>=) \d", r"\d(\.5)? (==|!=|<|<=|>|>=) i", r"not ", r"ports\[_\]", r"cs\[_\]\.image",
                   r"count\(a\) - \d", r"args\[\d\]", r"\d\.5"):
        assert any(re.search(needle, t) for t in texts), needle


FUZZ_COUNTS = {0: 775, 10: 779, 20: 1026, 30: 731, 100: 382}   # the oracle's violation counts per batch of seeds (assert_parity compares every result)


@pytest.mark.parametrize("first", [0, 10, 20, 30])
def test_fuzz_interpreter(first):
    assert U.run_fuzz("hostemu", range(first, first + 10)) == FUZZ_COUNTS[first]


@pytest.mark.parametrize("first", [0, 10, 20, 30])
def test_fuzz_generated_plan_code(first):
    assert U.run_fuzz("hostemu-gen", range(first, first + 10)) == FUZZ_COUNTS[first]


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["gpu", "gpu-interp"])
def test_fuzz_device(backend):
    """8 seeds in one process of its own, under a time limit"""
    assert int(_script(backend, "fuzz", 100, 8)[-1]) == FUZZ_COUNTS[100]
