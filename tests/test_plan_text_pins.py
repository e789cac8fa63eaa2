"""Pins of the plan-specialised text (csrc/codegen.cpp and its headers) where test_self_join_plan_text's and test_dnf_form's hashes do not
reach: plans with alias cursors, key relations (F_KCMP) and ordering relations (F_VCMP) at every row-group geometry, configs[2] under
each of the generator's switches, the 64-review text of configs[2] and of the corpus, and a corpus forced into several plan groups.
The procedure is test_self_join_plan_text.plan_text_sha256's (the GPU-less build writes every launch's text to GK_EMU_HIP_SOURCE_DIR);
each case runs in a process of its own, because the geometry and most switches are read once per process.  The hashes cover the whole
text handed to hiprtc, so a change to plan.hpp, vm_core.hpp, kernel_body.inc or the generator's output re-pins them, as it re-pins
test_self_join_plan_text's:  python tests/test_plan_text_pins.py  prints the hashes of the tree it runs in."""
import glob
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import pytest   # noqa: E402

# case -> (what, GK_RPT, environment).  what: "relations" | "selfjoin" (the self-joins of one array alone: a plan small enough for the
# unrolled form, where an alias cursor's loop is the one loop that stays a loop) | a benchmark policy set (2, 4) | "groups" (configs[4], plan groups of <= 64)
CASES = {
    "relations-64": ("relations", 64, {}),
    "relations-128": ("relations", 128, {}),
    "relations-256": ("relations", 256, {}),
    "selfjoin-64": ("selfjoin", 64, {}),
    "selfjoin-256": ("selfjoin", 256, {}),
    "configs2-256-conj0": (2, 256, {"GK_JIT_CONJ": 0}),
    "configs2-256-join0": (2, 256, {"GK_JIT_JOIN": 0}),
    "configs2-256-roll0": (2, 256, {"GK_JIT_ROLL": 0}),
    "configs2-256-preload0": (2, 256, {"GK_JIT_PRELOAD": 0}),
    "configs2-256-prelive16": (2, 256, {"GK_JIT_PRE_LIVE": 16}),
    "configs2-256-reslanes0": (2, 256, {"GK_JIT_RES_LANES": 0}),
    "configs2-64": (2, 64, {}),
    "corpus-64": (4, 64, {}),
    "corpus-128-groups": ("groups", 128, {}),
}

SHA256 = {
    "relations-64": "7f160b2804112db695017f3f35af6a09ad3eed3c6f5f0378fefded4c9a6e38a9",
    "relations-128": "e65fa613264909f0121e2aa38340e25c1c43a0b8e9591618b97de34378053e5b",
    "relations-256": "44e44487a10675694f461a3826248ea59beb286a6ef591b4693246ce574479b3",
    "selfjoin-64": "f6a48ce72992cb9a01e61a5cbb8e41898c3ad0632b4752bcb560ec59f47eddfb",
    "selfjoin-256": "90425fe4857b3011a4960198d629af6977f59f3d03c0363bba1a6fd4a0e2cab6",
    "configs2-256-conj0": "c44adafc812f55e40c9a0b3eab3f89ff58b147c4d06efa67f325cdd32ee4224e",
    "configs2-256-join0": "d6049a35f8d1689889f839018367c65128c07283f4b214cbbeb63e72c42af2dc",
    "configs2-256-roll0": "a45bbe013d73b36c438bc9f4efcb4d20ad3c457b9ad586ad39d37abc1f0677cd",
    "configs2-256-preload0": "96d8db74aecef8d2cd3dc180a55a4eb47638f4aca35a9359eb9ef8eaa39d383b",
    "configs2-256-prelive16": "29b2292066ef1d29f621c3792d7f512cfa50f770611cf5fafbbf1d61d45b2d4e",
    "configs2-256-reslanes0": "71b688d258983e1d7378ddca835d00ab3e0288fa7456610ee23006559e80ddd3",
    "configs2-64": "01cf31db45b7c6a8d447b9860e0a907466f0312bc3243789ce5e4bcb5e03fd6c",
    "corpus-64": "70b02f3f4dc7ecc46b85d8346e66271fa4d185342e8bf0a8786b45876d016ab0",
    "corpus-128-groups": "8bc3283182a625c484c9e1694dafd09eb8812738d16491b0dbf73595c4fa5ec6",
}


def _texts(out_dir):
    return sorted({open(f).read() for f in glob.glob(os.path.join(str(out_dir), "gk_plan_*.hip"))})


def _alias_loop(text):
    """a run-time loop inside a run-time loop with the same bound: two cursors over one scope, the inner one an alias cursor's"""
    open_loops = []   # (indentation, scope) of the loops around the line
    for m in re.finditer(r"^( *)\{ const uint32_t n\d+ = GK_UNI\(bounds\[(\d+)\]\);$", text, re.M):
        ind, scope = len(m.group(1)), m.group(2)
        open_loops = [l for l in open_loops if l[0] < ind]
        if any(l[1] == scope for l in open_loops):
            return True
        open_loops.append((ind, scope))
    return False


def _relations(out_dir, layouts=("RootRoot", "TwoMembers", "PackedOuter", "SelfJoin", "Negated", "Mixed"),
               kinds=("K8sDupImage", "K8sDupName", "K8sDupPairs", "K8sPortClash")):   # a name self-join, i != j, i < j, ports against ports
    """value_order_util.geom's policy set (every slot layout of the ordering relations, and the body that mixes an equality join with
    one) with test_self_join's templates in one engine, over 150 objects -> the hash, as plan_text_sha256 computes it"""
    import test_self_join as S
    import value_order_util as U
    from gatekeeper_amd import driver as D
    os.environ.update(GK_HOSTEMU_KERNEL="jit", GK_EMU_HIP_SOURCE_DIR=str(out_dir), GK_EMU_GRID="8")
    templates, constraints = [], []
    for layout in layouts:
        templates += U.layout_templates(layout, U.MIXED if layout == "Mixed" else None)
        constraints += U.layout_constraints(layout)
    for kind in kinds:
        templates.append(S.tmpl(kind, S.REGO[kind]))
        constraints.append(S.cons(kind, "sj-" + kind.lower()))
    client = D.Client(D.Driver(device=0, hostemu=True))
    for t in templates:
        client.AddTemplate(t)
    for k in constraints:
        client.AddConstraint(k)
    rv = U.reviews(U.layout_objects(seed=11, n=149))
    table = client.driver.engine.create_table([D.to_review_in(r) for r in rv], keep_docs=False)
    table.eval()
    table.free()
    texts = _texts(out_dir)
    assert texts, "the emulated evaluation produced no plan-specialised source"
    h = hashlib.sha256()
    for t in texts:
        h.update(hashlib.sha256(t.encode()).digest())
    return h.hexdigest()


def _child(case, out_dir):
    import test_self_join_plan_text as T
    what = CASES[case][0]
    if what == "relations":
        return _relations(out_dir)
    if what == "selfjoin":
        return _relations(out_dir, (), ("K8sDupImage", "K8sDupName", "K8sDupPairs"))   # (two loops deep: the four-deep ones exceed the unrolled form's budget)
    if what == "groups":
        from gatekeeper_amd import _lib
        from parity_util import plan_group_max
        with plan_group_max(_lib.load(hostemu=True), 64):
            return T.plan_text_sha256(4, out_dir)
    return T.plan_text_sha256(what, out_dir)


def case_sha256(case, out_dir):
    _, rpt, switches = CASES[case]
    env = {k: v for k, v in os.environ.items() if not k.startswith("GK_JIT_")}
    env.update({k: str(v) for k, v in switches.items()})
    env["GK_RPT"] = str(rpt)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child", case, str(out_dir)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.split()[-1]


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_text_unchanged(case, tmp_path):
    assert case_sha256(case, tmp_path) == SHA256[case]
    texts = _texts(tmp_path)
    if CASES[case][0] == "relations":   # what these pins are for is in the text they cover
        parts = "\n".join(t[t.index("void jit_formula_part("):] for t in texts)
        assert _alias_loop(parts), "no alias-cursor loop"
        assert re.search(r"= \(uint32_t\)\(e\d+ != e\d+\);", parts) and re.search(r"= \(uint32_t\)\(e\d+ < e\d+\);", parts), "no key relation"
        assert re.search(r"\(xa_ (<|<=|>|>=) xb_\)", parts), "no ordering relation"
    if CASES[case][0] == "selfjoin":
        parts = "\n".join(t[t.index("void jit_formula_part("):] for t in texts)
        assert re.search(r"constexpr uint32_t e\d+ = ", parts) and re.search(r"\{ const uint32_t n\d+ = GK_UNI\(bounds\[\d+\]\);", parts), "no alias-cursor loop among unrolled copies"
        assert re.search(r"= \(uint32_t\)\(e\d+ (!=|<) e\d+\);", parts), "no key relation"
    if CASES[case][0] == "groups":
        assert len(texts) >= 3, "one plan group only"


if __name__ == "__main__":
    if sys.argv[1:2] == ["child"]:
        print("sha", _child(sys.argv[2], sys.argv[3]))
    else:   # prints the hashes of the tree it runs in
        import tempfile
        for name in sorted(CASES):
            with tempfile.TemporaryDirectory() as d:
                print('    "%s": "%s",' % (name, case_sha256(name, d)))
