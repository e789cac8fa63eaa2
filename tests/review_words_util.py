"""Helper of test_review_words.py, run as a script in a process of its own on the GPU (the review-words switches are read once per
process: GK_REVIEW_WORDS, GK_REVIEW_WORDS_MIN; GK_RPT / GK_FORCE_RPP set the geometry).  Prints one JSON line per case.
usage: review_words_util.py table POLICY N [A,B,C]  one resident table: result words (SHA-256), rows the sweep streams, kernel text hash,
                                                   gk_table_verify (the bytecode kernel keeps the full lists)
       review_words_util.py oracle POLICY N        parity_util.assert_parity of N objects against the Python oracle
       review_words_util.py warm                   policy change under a warm table, two tables on one engine, a sharded sweep between plain ones
       review_words_util.py fuzz SEED...           test_template_fuzz.run_batched("gpu", seed, ..) per seed"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

from gatekeeper_amd import driver as D  # noqa: E402
from gatekeeper_amd import synth  # noqa: E402

POD_KINDS = [{"apiGroups": [""], "kinds": ["Pod"]}]


def policy(name):
    fx = synth.load_fixtures()
    if name == "configs2":
        return synth.psp_templates(fx), synth.audit_constraints()
    if name == "corpus":
        return synth.corpus(fx, 200)
    if name == "labels":   # review-level tests only: required labels, one constraint per label
        t = fx["yaml"]["demo/basic/templates/k8srequiredlabels_template.yaml"]["docs"][0] if "demo/basic/templates/k8srequiredlabels_template.yaml" in fx["yaml"] else None
        if t is None:
            t = next(fx["yaml"][p]["docs"][0] for p in sorted(fx["yaml"]) if p.endswith("k8srequiredlabels_template.yaml"))
        kind = t["spec"]["crd"]["spec"]["names"]["kind"]
        params = [{"labels": ["owner"]}, {"labels": ["team", "env"]}, {"labels": ["app"]}]
        if "allowedRegex" in json.dumps(t):
            params = [{"labels": [{"key": "owner"}]}, {"labels": [{"key": "team"}, {"key": "env"}]}, {"labels": [{"key": "app"}]}]
        return [t], [{"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": kind, "metadata": {"name": "labels-%d" % i},
                      "spec": {"match": {"kinds": POD_KINDS}, "parameters": p}} for i, p in enumerate(params)]
    if name == "none":     # element tests only and no match block: nothing for the binding pass to evaluate
        t = next(t_ for t_ in synth.psp_templates(fx) if t_["spec"]["crd"]["spec"]["names"]["kind"] == "K8sPSPPrivilegedContainer")
        return [t], [{"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": "K8sPSPPrivilegedContainer", "metadata": {"name": "priv"}, "spec": {}}]
    raise SystemExit("unknown policy " + name)


def client(name, elem_cap=None):
    drv = D.Driver(device=0, hostemu=False, elem_cap=elem_cap)
    c = D.Client(drv)
    templates, constraints = policy(name)
    for t in templates:
        c.AddTemplate(t)
    for k in constraints:
        c.AddConstraint(k)
    return c


def native_table(c, n, seed=synth.SEED, resident=True):
    eng = c.driver.engine
    batch = synth.NativeBatch(eng.lib, n, seed=seed, mixed=True, start=0, namespaces=synth.gen_namespaces())
    table = eng.create_table_native(batch.reviews, n, keep_docs=False, resident=resident)
    table._batch = batch
    return table


def words(ev):
    h = hashlib.sha256()
    for a in (ev.viol, ev.err, ev.match, ev.too_big, ev.counts):
        h.update(a.tobytes())
    return h.hexdigest()


def summary(c, table):
    ev = table.eval(want_match=True, download=True)
    v = c.driver.VerifyTable(table, want_match=True)
    again = table.eval(want_match=True, download=True)
    return {"words": words(ev), "again": words(again), "pairs": int(ev.counts.sum()), "n_rows_read": int(ev.n_rows_read), "algo_bytes": int(ev.algo_bytes),
            "hash": "%016x" % ev.kernel_text_hash, "overflow": int(ev.n_overflow), "verify_ok": bool(v.ok), "specialised_groups": int(v.specialised_groups),
            "n_plan_groups": int(v.n_plan_groups), "diff_total": int(v.diff_total), "diff_too_big": int(v.diff_too_big)}


def case_table(name, n, cap=None):
    c = client(name, elem_cap=cap)
    table = native_table(c, n, resident=cap is None)   # (a resident table's plan takes its capacities from the table: squeezed ones need a plain table)
    try:
        print(json.dumps(summary(c, table)))
    finally:
        table.free()


def case_oracle(name, n):
    from oracle import client as OC
    from parity_util import assert_parity
    c, oc = client(name), OC.Client()
    templates, constraints = policy(name)
    for t in templates:
        oc.add_template(t)
    for k in constraints:
        oc.add_constraint(k)
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(n, seed=7, mixed=True)
    rv = [D.AugmentedUnstructured(D.Unstructured(o), synth.namespace_for(o, nss), "Original") for o in objs]
    refused = []
    total = assert_parity(c, oc, rv, refused=refused)
    # which kernel evaluated such a table: one more, created as assert_parity creates its own
    table = c.driver.engine.create_table([D.to_review_in(r, None) for r in rv], keep_docs=False)
    try:
        ev = table.eval()
        print(json.dumps({"results": total, "refused": len(refused), "hash": "%016x" % ev.kernel_text_hash, "n_rows_read": int(ev.n_rows_read), "pairs": int(ev.counts.sum())}))
    finally:
        table.free()


def case_warm(n):
    c = client("configs2")
    a, b = native_table(c, n), native_table(c, n // 2 + 37, seed=synth.SEED + 1)
    try:
        out = {"a0": summary(c, a), "b0": summary(c, b)}
        # a constraint more under the warm tables: a new plan, a new binding, rebuilt words
        extra = dict(json.loads(json.dumps(synth.audit_constraints()[3])))
        extra["metadata"] = {"name": "one-more"}
        c.AddConstraint(extra)
        out["a1"], out["b1"] = summary(c, a), summary(c, b)
        c.RemoveConstraint(extra)
        out["a2"] = summary(c, a)
        # a sharded sweep at world size 1 between plain sweeps: the same words (last: a table set up as a shard is not verified any more)
        plain = a.eval(want_match=False, download=True)
        import ctypes as C
        import numpy as np
        from gatekeeper_amd import _lib as L
        from gatekeeper_amd.sweep import ShardedResult
        eng = c.driver.engine
        ident = C.create_string_buffer(L.GK_COMM_ID_BYTES)
        eng._check(eng.lib.gk_comm_unique_id(ident))
        eng._check(eng.lib.gk_comm_init(eng.handle, ident.raw, 0, 1))
        eng._check(eng.lib.gk_table_sweep_sharded(eng.handle, a.handle, L.GK_SHARD_ENQUEUE, None))
        so = C.POINTER(L.gk_shard_out)()
        eng._check(eng.lib.gk_table_sweep_sharded(eng.handle, a.handle, L.GK_SHARD_DOWNLOAD, C.byref(so)))
        res = ShardedResult(eng.lib, so)
        out["sharded_totals_equal"] = bool((res.totals == plain.counts.astype(np.int64)).all() and res.beyond_limits == 0)
        after = a.eval(want_match=False, download=True)
        out["plain_equal_after_shard"] = bool((plain.viol == after.viol).all() and (plain.err == after.err).all() and (plain.counts == after.counts).all())
        out["words_after_shard"] = hashlib.sha256(after.viol.tobytes() + after.err.tobytes() + after.counts.tobytes()).hexdigest()
        print(json.dumps(out))
    finally:
        a.free()
        b.free()


def case_fuzz(seeds):
    import test_template_fuzz as F
    loaded = compared = 0
    for s in seeds:
        mode = int(s) % 4
        lo, co = F.run_batched("gpu", int(s), 20, 14, envelope=mode == 1, numeric=mode >= 2, v1=mode == 3)
        loaded += lo
        compared += co
    print(json.dumps({"seeds": [int(s) for s in seeds], "loaded": loaded, "compared": compared}))


if __name__ == "__main__":
    what = sys.argv[1]
    if what == "table":
        case_table(sys.argv[2], int(sys.argv[3]), tuple(int(x) for x in sys.argv[4].split(",")) if len(sys.argv) > 4 else None)
    elif what == "oracle":
        case_oracle(sys.argv[2], int(sys.argv[3]))
    elif what == "warm":
        case_warm(600)
    elif what == "fuzz":
        case_fuzz(sys.argv[2:])
