"""Helper of test_dnf_form.py, run as a script in a process of its own (the generator reads its A/B switches once per process).
usage: dnf_form_util.py sha <config>                 SHA-256 of the plan-specialised text of a benchmark policy set (test_self_join_plan_text's procedure)
       dnf_form_util.py text <dir>                   the configs[2] text, written to <dir>
       dnf_form_util.py oracle <backend> <policy> <n>   product against the Python oracle for n synthetic objects: rendered results and the raw
                                                     violation / autoreject bitmaps against the oracle's pairs (parity_util.assert_parity)
       dnf_form_util.py words <backend>              SHA-256 of the violation / autoreject / match words of configs[2] (1 500) and the corpus (512)
       dnf_form_util.py fuzz <backend> <first> <last>   test_template_fuzz.run_batched over the seeds, each plan against the oracle
at the geometry (GK_RPT) and with the switches the environment sets.  backend: hostemu (with GK_HOSTEMU_KERNEL=jit: the emulated
plan-specialised kernel) or gpu."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]


def _policy(policy, fx):
    from gatekeeper_amd import synth
    if policy == "configs2":
        return synth.psp_templates(fx), synth.audit_constraints()
    return synth.corpus(fx, 200)


def oracle(backend, policy, n):
    import parity_util as P
    from gatekeeper_amd import driver as D
    from gatekeeper_amd import synth
    templates, constraints = _policy(policy, synth.load_fixtures())
    c, oc = P.load_both(backend, templates, constraints)
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(n, seed=synth.SEED, mixed=True)
    reviews = [D.AugmentedUnstructured(D.Unstructured(o), synth.namespace_for(o, nss), "Original") for o in objs]
    refused = []
    total = P.assert_parity(c, oc, reviews, D.AUDIT_EP, refused=refused)
    assert total > 0 and len(refused) < n // 2, (total, len(refused))
    return total


def words(backend, policy, n):
    from gatekeeper_amd import driver as D
    from gatekeeper_amd import synth
    if backend == "gpu":
        os.environ["GK_JIT_STRICT"] = "1"   # (a hiprtc failure fails the run instead of falling to the bytecode kernel)
    templates, constraints = _policy(policy, synth.load_fixtures())
    drv = D.Driver(device=0, hostemu=backend != "gpu")
    client = D.Client(drv)
    for t in templates:
        client.AddTemplate(t)
    for k in constraints:
        client.AddConstraint(k)
    batch = synth.NativeBatch(drv.engine.lib, n, seed=synth.SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
    table = drv.engine.create_table_native(batch.reviews, n, keep_docs=False, resident=True)
    ev = table.eval(want_match=True, download=True)
    assert int(ev.counts.sum()) > 0 and ev.viol is not None and ev.match is not None
    h = hashlib.sha256()
    for a in (ev.viol, ev.err, ev.match, ev.too_big, ev.counts):
        h.update(a.tobytes())
    return h.hexdigest()


if __name__ == "__main__":
    assert os.environ.get("GK_RPT") in ("128", "256")
    what = sys.argv[1]
    if what == "sha":
        import tempfile
        import test_self_join_plan_text as T
        with tempfile.TemporaryDirectory() as d:
            print("sha", T.plan_text_sha256(int(sys.argv[2]), d))
    elif what == "text":
        import test_self_join_plan_text as T
        print("sha", T.plan_text_sha256(2, sys.argv[2], n=1200))
    elif what == "oracle":
        print("oracle", sys.argv[3], oracle(sys.argv[2], sys.argv[3], int(sys.argv[4])))
    elif what == "words":
        print("configs2", words(sys.argv[2], "configs2", 1500))
        print("corpus", words(sys.argv[2], "corpus", 512))
    else:
        import test_template_fuzz as F
        loaded = compared = 0
        for seed in range(int(sys.argv[3]), int(sys.argv[4]) + 1):
            mode = seed % 4
            l, c = F.run_batched(sys.argv[2], seed, 60, 14, envelope=mode == 1, numeric=mode >= 2, v1=mode == 3)
            loaded += l
            compared += c
        print("fuzz", loaded, compared)
