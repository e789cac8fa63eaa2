"""Helper of test_cold_args.py, run as a script in a process of its own on the GPU (GK_JIT_COLD_ARGS, GK_JIT_COLD_ARGS_MIN and GK_FUSED_TOTALS
are read once per process).  Runs every case of that file on the device and prints one JSON object: case name -> figures."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import review_words_util as U  # noqa: E402
from gatekeeper_amd import driver as D  # noqa: E402
from gatekeeper_amd import synth  # noqa: E402

REVIEWS = (1, 63, 64, 65, 255, 257, 513)
CONSTRAINTS = (1, 50, 64, 65, 130)


def client_with(n_constraints):
    """configs[2]'s templates with its 50 constraints cut or repeated (under new names) to n_constraints"""
    c = D.Client(D.Driver(device=0, hostemu=False))
    templates, constraints = U.policy("configs2")
    for t in templates:
        c.AddTemplate(t)
    for k in repeated(constraints, n_constraints):
        c.AddConstraint(k)
    return c


def plain_words(ev):
    return hashlib.sha256(b"".join(a.tobytes() for a in (ev.viol, ev.err, ev.too_big, ev.counts))).hexdigest()


def verified(c, t, want_match):
    v = c.driver.VerifyTable(t, want_match=want_match)
    return bool(v.ok) and int(v.specialised_groups) > 0 and int(v.specialised_groups) == int(v.n_plan_groups) and int(v.diff_total) == 0 and int(v.diff_too_big) == 0


def oracle_parity(c, templates, constraints, n, seed):
    """parity_util.assert_parity of n generated objects: rendered results and raw device bitmaps against the Python oracle"""
    from oracle import client as OC
    from parity_util import assert_parity
    oc = OC.Client()
    for t in templates:
        oc.add_template(t)
    for k in constraints:
        oc.add_constraint(k)
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(n, seed=seed, mixed=True)
    rv = [D.AugmentedUnstructured(D.Unstructured(o), synth.namespace_for(o, nss), "Original") for o in objs]
    refused = []
    total = assert_parity(c, oc, rv, refused=refused)
    table = c.driver.engine.create_table([D.to_review_in(r, None) for r in rv], keep_docs=False)   # (which kernel evaluated such a table)
    try:
        return {"results": total, "refused": len(refused), "hash": "%016x" % table.eval().kernel_text_hash}
    finally:
        table.free()


def repeated(constraints, n_constraints):
    out = []
    for i in range(n_constraints):
        k = json.loads(json.dumps(constraints[i % len(constraints)]))
        k["metadata"] = dict(k["metadata"], name="%s-r%d" % (k["metadata"]["name"], i // len(constraints)))
        out.append(k)
    return out


def main():
    out = {}
    with_oracle = os.environ.get("GK_JIT_COLD_ARGS") != "0" and os.environ.get("GK_FUSED_TOTALS") != "0"   # (the variant's results; the switch-off run is compared with them bit for bit)
    c = U.client("configs2")
    for n in REVIEWS:
        t = U.native_table(c, n)
        try:
            out["reviews_%d" % n] = U.summary(c, t)
        finally:
            t.free()
        if with_oracle:
            out["reviews_%d" % n]["oracle"] = oracle_parity(c, *U.policy("configs2"), n, 100 + n)
    for k in CONSTRAINTS:
        ck = client_with(k)
        t = U.native_table(ck, 257)
        try:
            out["constraints_%d" % k] = U.summary(ck, t)
        finally:
            t.free()
        if with_oracle:
            templates, constraints = U.policy("configs2")
            out["constraints_%d" % k]["oracle"] = oracle_parity(ck, templates, repeated(constraints, k), 65, 200 + k)
    # match words off, on, off on one table: null and non-null `match`, the cached launch dropped in between
    t = U.native_table(c, 257)
    try:
        seq = []
        for wm in (False, False, True, False, False):
            ev = t.eval(want_match=wm, download=True)
            seq.append({"plain": plain_words(ev), "match": hashlib.sha256(ev.match.tobytes()).hexdigest() if wm else None, "hash": "%016x" % ev.kernel_text_hash,
                        "verified": verified(c, t, wm)})
        out["want_match_sequence"] = seq
        # 1, 64 and 65 launches before one collecting call
        for k in (1, 64, 65):
            for _ in range(k):
                t.launch()
            ev = t.eval(download=True, collect_only=True)
            out["launches_%d" % k] = {"plain": plain_words(ev), "hash": "%016x" % ev.kernel_text_hash, "n_launches": int(ev.n_launches), "verified": verified(c, t, False)}
        # the pair list: (constraint, review) entries allocated through the returning atomic, against the bits of the violation words
        ev = t.eval(want_list=True, download=True)
        pairs = sorted((int(a), int(b)) for a, b in ev.list)
        bits = sorted((ci, w * 64 + b) for ci in range(ev.viol.shape[0]) for w in range(ev.viol.shape[1]) for b in range(64) if (int(ev.viol[ci, w]) >> b) & 1)
        out["pair_list"] = {"pairs": hashlib.sha256(json.dumps(pairs).encode()).hexdigest(), "n": len(pairs), "list_total": int(ev.list_total), "equals_bitmap": pairs == bits,
                            "plain": plain_words(ev), "hash": "%016x" % ev.kernel_text_hash, "verified": verified(c, t, False)}
    finally:
        t.free()
    # two tables on one engine
    a, b = U.native_table(c, 513), U.native_table(c, 65, seed=synth.SEED + 1)
    try:
        out["two_tables_a"], out["two_tables_b"] = U.summary(c, a), U.summary(c, b)
        out["two_tables_a_again"] = U.summary(c, a)
    finally:
        a.free()
        b.free()
    # squeezed element capacities: overflow, too_big, list_count[1]
    cs = U.client("configs2", elem_cap=(2, 4, 2))
    t = U.native_table(cs, 600, resident=False)
    try:
        out["overflowed"] = U.summary(cs, t)
    finally:
        t.free()
    if with_oracle:
        out["overflowed"]["oracle"] = oracle_parity(cs, *U.policy("configs2"), 257, 301)
    # a plan without hoisted review-word classes
    cn = U.client("none")
    t = U.native_table(cn, 257)
    try:
        out["no_hoisted_class"] = U.summary(cn, t)
    finally:
        t.free()
    if with_oracle:
        out["no_hoisted_class"]["oracle"] = oracle_parity(cn, *U.policy("none"), 257, 302)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
