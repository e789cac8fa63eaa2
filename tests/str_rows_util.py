"""Helpers of the tests that reach the device's string ROW predicates (csrc/vm_core.hpp: str_prefix_c, str_at_c / swin, str_contains_short,
str_eq_c, str_cmp_c, the SplitMask family, the DFA walk of P_REGEX).  The lowering promotes every test on a string leaf's bytes to a
dictionary expression (lower.cpp PROMOTION) that the HOST evaluates per distinct value; the rows stay the answer where the leaf's dictionary
is full (62 expressions per leaf; one shared 62-bit space for all the review facts).  fill_dictionaries() fills it with 62 filler
expressions, so that whatever is loaded AFTERWARDS is lowered to row predicates, and require_rows() asserts from engine.dump() that it was.
The reference of the probes is Python `bytes` arithmetic on the UTF-8 encodings, nothing of the product or the oracle."""
import collections
import re

from gatekeeper_amd import driver as D

# plan.hpp PredOp
P_CMP, P_STR_PREFIX, P_STR_SUFFIX, P_STR_CONTAINS, P_STR_IN_SET, P_SPLIT_CMP, P_SPLIT_COUNT, P_SPLIT_PREFIX, P_REGEX, P_BITS = 3, 5, 6, 7, 8, 9, 10, 14, 15, 16
DICT_BITS = 62

IMAGE = "input.review.object.spec.containers[_].image"          # an element leaf: a dictionary of its own
PROBE = "input.review.object.metadata.annotations.probe"       # a review fact: review.$r.$d, one dictionary for all such leaves
FILL_KIND = "K8sStrRowsFill"
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 19, 20, 33)


def template(kind, bodies):
    """one violation rule per body; a body without a msg assignment gets a constant one"""
    rego = "package %s\n" % kind.lower() + "".join('violation[{"msg": msg}] {\n  %s\n}\n' % (b if "msg :=" in b else b + '\n  msg := "%s rule %d"' % (kind, i))
                                                 for i, b in enumerate(bodies))
    return {"apiVersion": "templates.gatekeeper.sh/v1", "kind": "ConstraintTemplate", "metadata": {"name": kind.lower()},
            "spec": {"crd": {"spec": {"names": {"kind": kind}}}, "targets": [{"target": "admission.k8s.gatekeeper.sh", "rego": rego}]}}


def constraint(kind, name, params):
    return {"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": kind, "metadata": {"name": name}, "spec": {"parameters": params}}


def fill_policy(leaves):
    """the filler template (contains(<leaf>, input.parameters.p) per leaf) and its 62 constraints; no probe string holds a filler constant"""
    return (template(FILL_KIND, ["contains(%s, input.parameters.p)" % leaf for leaf in leaves]),
            [constraint(FILL_KIND, "fill%02d" % i, {"p": "\x01fill%02d\x02" % i}) for i in range(DICT_BITS)])


def fill_dictionaries(client, leaves, oracle=None):
    """loads the fillers into `client` (and into the oracle client, where one is compared with it); to be called BEFORE the policies under test"""
    t, cons = fill_policy(leaves)
    client.AddTemplate(t)
    if oracle is not None:
        oracle.add_template(t)
    for k in cons:
        client.AddConstraint(k)
        if oracle is not None:
            oracle.add_constraint(k)


def rows_loader(leaves, guard):
    """a stand-in for parity_util.load_both that loads the same policies BEHIND full dictionaries of `leaves` and then calls guard(client)
    (the require_rows of the caller); a test module's own load_both is replaced by it to run that module's tests on the row path"""
    from parity_util import load_both

    def load(backend, templates, constraints, data=(), validate=True, **kw):
        c, oc = load_both(backend, [], [], **kw)
        fill_dictionaries(c, leaves, oc)
        for t in templates:
            c.AddTemplate(t)
            oc.add_template(t)
        for k in constraints:
            c.AddConstraint(k, validate=validate)
            oc.add_constraint(k, validate=validate)
        for d in data:
            c.AddData(d)
            oc.add_data(d)
        guard(c)
        return c, oc
    return load


_PRED = re.compile(r"^pred (\d+) op=(\d+) dst=(\d+) scope=(\d+) bit=(\d+) ?(.*)$", re.M)
_CONS = re.compile(r"^constraint (\d+) ([^/\s]+)/(\S+) viol: (.*)$", re.M)


def preds_of(client):
    """[(index, op, dst, pattern text)] of the primary plan"""
    return [(int(i), int(op), int(dst), pat) for i, op, dst, _, _, pat in _PRED.findall(client.driver.engine.dump())]


def ops_of(client):
    """histogram {(op, dst): predicates} of the primary plan"""
    return collections.Counter((op, dst) for _, op, dst, _ in preds_of(client))


def require_rows(client, kind, op, n, dsts=(0, 1), min_preds=None, filled=True):
    """The guard of these tests: the n constraints of `kind` are loaded and the plan holds at least n predicates `op` on EVERY destination in
    `dsts` (0: review-level bits, 1: element scope) -- a test and its negation share one predicate, so kinds may share theirs (min_preds: another
    lower bound, where a constraint holds several tests) -- and NONE
    of what was loaded after the fillers became a bit of a dictionary row: every P_BITS predicate of the plan is one of the DICT_BITS
    fillers of its row (filled=False, for tests the lowering keeps on the rows without fillers: the plan holds no P_BITS predicate at all).
    Fails (never skips) when the promotion rule or the size of a dictionary changes."""
    dump = client.driver.engine.dump()
    names = [m[2] for m in _CONS.findall(dump) if m[1] == kind]
    assert len(names) == n, "%d constraints of %s loaded, %d expected" % (len(names), kind, n)
    preds = preds_of(client)
    ops = collections.Counter((o, dst) for _, o, dst, _ in preds)
    rows = collections.Counter(pat for _, o, _, pat in preds if o == P_BITS)
    assert (rows and all(pat.endswith(".$d") and k == DICT_BITS for pat, k in rows.items())) if filled else not rows, (
        "dictionary predicates %r: the fillers are %d per dictionary row, and nothing under test may add one" % (dict(rows), DICT_BITS))
    n = n if min_preds is None else min_preds
    for dst in dsts:
        assert ops.get((op, dst), 0) >= n, "%s: %d row predicates op=%d on dst=%d, %d expected (plan: %r): the tests under test left the rows" % (
            kind, ops.get((op, dst), 0), op, dst, n, dict(ops))
    return ops


# ---------------------------------------------------------------------------------------------- probes and their reference
def const_of(m):
    """distinct alphabetic content per length (no x, y, z: the pads of the probe strings)"""
    return "".join("abcdefghijklmnopqrstuvw"[(m * 5 + i * 7) % 23] for i in range(m))


CONSTANTS = [const_of(m) for m in LENGTHS]
POSITIONS = (0, 3, 4, 7, 8, 11, 12, 15, 16)
POSTS = (0, 1, 2, 3, 5, 9, 40)


def probes_for(p, pres=range(14)):
    out = [p, p[:-1], p + "x", "x" + p, p + "\u0000", "\u0000" + p, ""]
    out += ["y" * pre + p + "z" * post for pre in pres for post in POSTS]
    for k in sorted({k for k in POSITIONS if k < len(p)} | {len(p) - 1}):
        m = p[:k] + chr(ord(p[k]) ^ 1) + p[k + 1:]          # the neighbour letter: one bit of one byte
        out += [m, "yy" + m, "yyyyy" + m, m + "zzz", p[:k] + "é" + p[k + 1:]]   # (U+00E9: bytes C3 A9, above every ASCII byte)
    out += [p[:-1] + p, p[0] * 3 + p]
    return out


def probe_strings(constants=CONSTANTS, pres=range(14)):
    """every probe of every constant, distinct, in a fixed order"""
    return list(dict.fromkeys(s for p in constants for s in probes_for(p, pres)))


def b(s):
    return s.encode("utf-8")


# name -> (Rego test of (x, p), the same on bytes); Rego orders strings bytewise (unsigned), as Python orders bytes
TESTS = {
    "prefix": ("startswith({x}, {p})", lambda s, p: s.startswith(p)),
    "notprefix": ("not startswith({x}, {p})", lambda s, p: not s.startswith(p)),
    "suffix": ("endswith({x}, {p})", lambda s, p: s.endswith(p)),
    "contains": ("contains({x}, {p})", lambda s, p: p in s),
    "eq": ("{x} == {p}", lambda s, p: s == p),
    "ne": ("{x} != {p}", lambda s, p: s != p),
    "lt": ("{x} < {p}", lambda s, p: s < p),
    "le": ("{x} <= {p}", lambda s, p: s <= p),
    "gt": ("{x} > {p}", lambda s, p: s > p),
    "ge": ("{x} >= {p}", lambda s, p: s >= p),
}
OPS = {"prefix": P_STR_PREFIX, "notprefix": P_STR_PREFIX, "suffix": P_STR_SUFFIX, "contains": P_STR_CONTAINS,
       "eq": P_CMP, "ne": P_CMP, "lt": P_CMP, "le": P_CMP, "gt": P_CMP, "ge": P_CMP}
FAMILIES = {"prefix": ("prefix", "notprefix"), "suffix": ("suffix",), "contains": ("contains",), "equality": ("eq", "ne"), "ordering": ("lt", "le", "gt", "ge")}
# one kind per test and place, so that one raw bit is one predicate on one string
# (the element rule's message names the container: the predicate lives in the element scope, dst=1, as the library's image tests do)
# (Label: a key iteration with a key filter -- a dictionary expression cannot stand under one, so these tests stay on the rows without fillers)
PLACES = {"Elem": 'c := input.review.object.spec.containers[_]\n  v := c.image\n  msg := sprintf("image of %v", [c.name])', "Rev": "v := " + PROBE,
          "Label": 'v := input.review.object.metadata.labels[key]\n  startswith(key, "a")'}


def kind_of(test, place):
    return "K8sStr%s%s" % (test.capitalize(), place)


def family_policy(tests, constants=CONSTANTS, places=("Elem", "Rev")):
    """-> templates, constraints, {(kind, name): (test, place, constant)}"""
    templates, constraints, what = [], [], {}
    for t in tests:
        for place in places:
            kind = kind_of(t, place)
            templates.append(template(kind, [PLACES[place] + "\n  " + TESTS[t][0].format(x="v", p="input.parameters.p")]))
            for p in constants:
                name = "m%02d" % len(p)
                constraints.append(constraint(kind, name, {"p": p}))
                what[(kind, name)] = (t, place, p)
    return templates, constraints, what


def pod(i, images, probe=None, labels=None):
    md = {"name": "p%d" % i, "namespace": "default"}
    if labels is not None:
        md["labels"] = labels
    if probe is not None:
        md["annotations"] = {"probe": probe}
    return {"apiVersion": "v1", "kind": "Pod", "metadata": md, "spec": {"containers": [{"name": "c%d" % j, "image": s} for j, s in enumerate(images)]}}


def reviews_of(objs):
    return [D.AugmentedUnstructured(D.Unstructured(o), None, "Original") for o in objs]


def want_pairs(what, objs):
    """the reference: {((kind, name), review)} -- the test holds on the annotation / on ANY container image of the review"""
    out = set()
    for key, (t, place, p) in what.items():
        fn, pb = TESTS[t][1], b(p)
        for i, o in enumerate(objs):
            if place == "Label":
                vals = [v for k, v in o["metadata"].get("labels", {}).items() if k.startswith("a")]
            elif place == "Rev":
                vals = [o["metadata"]["annotations"]["probe"]] if "probe" in o["metadata"].get("annotations", {}) else []
            else:
                vals = [c["image"] for c in o["spec"]["containers"]]
            if any(fn(b(s), pb) for s in vals):
                out.add((key, i))
    return out


def raw_pairs(client, objs, ep=D.AUDIT_EP):
    """one table of the reviews, one eval(): -> (EvalResult, {((kind, name), review)} of the raw violation bitmap, the same of the error bitmap)"""
    table = client.driver.engine.create_table([D.to_review_in(r, None) for r in reviews_of(objs)], keep_docs=False)
    try:
        ev = table.eval()
    finally:
        table.free()
    active = {cid: (cons.get("kind"), (cons.get("metadata") or {}).get("name")) for cid, (cons, _, _) in client._active(ep).items()}
    return ev, {(active[cid], r) for cid, r in ev.pairs("viol")}, {(active[cid], r) for cid, r in ev.pairs("err")}


def assert_raw_pairs(client, objs, what, overflow=False):
    ev, viol, err = raw_pairs(client, objs)
    assert ev.host_evaluated == [] and not ev.too_big_reviews()
    if overflow:
        assert ev.n_overflow > 0, "no review took the big path: the case shows nothing"
    viol = {(k, r) for k, r in viol if k[0] != FILL_KIND}
    want = want_pairs(what, objs)

    def show(pairs):
        return [(k, r, what[k][2], [c["image"] for c in objs[r]["spec"]["containers"]]) for k, r in sorted(pairs)[:6]]
    assert viol == want, "raw violation bitmap != bytes reference: %d only on the device %r, %d only in the reference (LOST bits) %r" % (
        len(viol - want), show(viol - want), len(want - viol), show(want - viol))
    assert not err, sorted(err)[:5]
    return len(want)
