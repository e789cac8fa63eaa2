"""Helper of test_join_form.py, run as a script in a process of its own (the generator reads its A/B switches once per process):
evaluates the benchmark's policy sets and the policy compiler's pattern / self-join plans on the emulated plan-specialised kernel at the
geometry and with the switches the environment sets, and prints one line per table with the SHA-256 of its result words.  The emulator
itself compares every bitmap word with the per-review evaluation and raises on a difference.
usage: join_form_util.py tables | patterns"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

from gatekeeper_amd import driver as D  # noqa: E402
from gatekeeper_amd import synth  # noqa: E402


def table_words(policy, n):
    fx = synth.load_fixtures()
    if policy == "configs2":
        templates, constraints = synth.psp_templates(fx), synth.audit_constraints()
    else:
        templates, constraints = synth.corpus(fx, 200)
    drv = D.Driver(device=0, hostemu=True)
    client = D.Client(drv)
    for t in templates:
        client.AddTemplate(t)
    for k in constraints:
        client.AddConstraint(k)
    batch = synth.NativeBatch(drv.engine.lib, n, seed=synth.SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
    table = drv.engine.create_table_native(batch.reviews, n, keep_docs=False, resident=True)
    ev = table.eval(want_match=True, download=True)   # violation, autoreject (error) and match words of every constraint
    assert int(ev.counts.sum()) > 0 and ev.viol is not None and ev.match is not None
    h = hashlib.sha256()
    for a in (ev.viol, ev.err, ev.match, ev.too_big, ev.counts):
        h.update(a.tobytes())
    return h.hexdigest()


def patterns():
    import test_library_patterns as L
    import test_pe_builtins as P
    import test_root_scope as R
    import test_self_join as S
    L.test_library_patterns_one_plan("hostemu")
    L.test_library_patterns_second_batch("hostemu")
    L.test_library_patterns_third_batch("hostemu")
    R.test_values_compared_outside_iterations("hostemu")
    P.test_string_tests_on_iterated_keys("hostemu")
    S.test_each_pair_once("hostemu")
    S.test_with_match_block("hostemu")
    S.test_edges("hostemu")


if __name__ == "__main__":
    assert os.environ.get("GK_HOSTEMU_KERNEL") == "jit" and os.environ.get("GK_RPT") in ("128", "256")
    if sys.argv[1] == "tables":
        print("configs2", table_words("configs2", 1500))
        print("corpus", table_words("corpus", 512))
    else:
        patterns()
        print("patterns ok")
