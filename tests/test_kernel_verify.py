"""gk_table_verify / gk_resident_verify: the plan-specialised kernel checked against the bytecode kernel ON the device (DESIGN.md
sections 5 and 11).  The two evaluations of every plan group are compared where they lie (gk_verify_diff; tests/native/hostemu_verify.cpp
on the CPU backends, where the generated plan source stands in for the specialised kernel and the interpreter for the bytecode kernel);
only counts and the first differences come back.  No oracle is involved: equal kernels give zero differences, and differences are
injected into the bytecode side with gk_debug_set("verify_flip", ...) -- one bit or one 64-bit word per call.

Policies: the PSP templates with the audit constraint set (50 constraints), as tests/test_resident_audit.py; objects from synth.
  shape A: 200 objects -- 4 bitmap words, the last with 8 valid bits; 64-review row groups (an admission-sized table, on which a plain
           evaluation would not wait for hiprtc)
  shape B: 8 200 objects -- 129 words: two full waves of columns plus one lane, the last word with 8 valid bits; 256-review sweep geometry.
           Runs on every backend (the CPU stand-ins take about a second for it)."""
import ctypes as C
import json

import numpy as np
import pytest

from gatekeeper_amd import _lib as L
from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from parity_util import BACKENDS, make_client, plan_group_max

SPECIALISED = [b for b in BACKENDS if b.id in ("hostemu-gen", "gpu")]
PLAIN = [b for b in BACKENDS if b.id in ("hostemu", "gpu-interp")]
ALL = SPECIALISED + PLAIN
VIOL, ERR, MATCH, TOO_BIG = 0, 1, 2, 3
KINDS = ("viol", "err", "match", "too_big")
N_A, N_B = 200, 8200


def load(backend, fixtures, constraints=None):
    c = make_client(backend)
    for t in synth.psp_templates(fixtures):
        c.AddTemplate(t)
    for k in (synth.audit_constraints() if constraints is None else constraints):
        c.AddConstraint(k)
    return c


def native_table(c, n, seed=23, resident=False):
    eng = c.driver.engine
    batch = synth.NativeBatch(eng.lib, n, seed=seed, mixed=True, start=0, namespaces=synth.gen_namespaces())
    table = eng.create_table_native(batch.reviews, n, resident=resident)
    table._batch = batch   # (the reviews' text lives as long as the table)
    return table


class flipped:
    """gk_debug_set("verify_flip", kind << 56 | whole_word << 55 | row << 32 | review) for the verifications inside the block"""

    def __init__(self, lib, kind, row, review, whole=False):
        self.lib, self.v = lib, kind << 56 | int(whole) << 55 | row << 32 | review

    def __enter__(self):
        assert self.lib.gk_debug_set(b"verify_flip", self.v) == 0

    def __exit__(self, *a):
        assert self.lib.gk_debug_set(b"verify_flip", -1) == 0


def bit(bitmap, row, review):
    return int(bitmap[row][review // 64] >> np.uint64(review % 64)) & 1


def assert_equal_kernels(backend, v, ev, want_match=False):
    assert v.specialised_groups == v.n_plan_groups == ev.n_plan_groups and v.ok
    assert (v.kernel_text_hash != 0) == (backend == "gpu")
    assert v.diff_total == 0 and v.diff_too_big == 0 and v.entries_total == 0 and v.entries == []
    assert not any(v.diff_viol.values()) and not any(v.diff_err.values())
    assert (v.diff_match is None) if not want_match else not any(v.diff_match.values())
    assert v.constraint_ids == [int(x) for x in ev.constraint_ids] and v.n_reviews == ev.n_reviews
    assert v.quarantined_groups == 0


def assert_untouched(table, ev, want_match=False):
    """a gk_table_eval behind the verification returns the bitmaps it returned before"""
    again = table.eval(want_match=want_match)
    assert (again.viol == ev.viol).all() and (again.err == ev.err).all() and (again.too_big == ev.too_big).all() and (again.counts == ev.counts).all()
    if want_match:
        assert (again.match == ev.match).all()
    assert [int(x) for x in again.constraint_ids] == [int(x) for x in ev.constraint_ids]
    return again


# ------------------------------------------------------------------------------------------------ equal kernels
@pytest.mark.parametrize("n", [N_A, N_B], ids=["A", "B"])
@pytest.mark.parametrize("backend", SPECIALISED)
def test_equal_kernels(backend, n, fixtures):
    c = load(backend, fixtures)
    table = native_table(c, n)
    try:
        ev = table.eval(want_match=True)
        assert ev.n_tiles == (n + 63) // 64 and n % 64 == 8 and ev.viol.any() and ev.n_plan_groups == 1
        assert_equal_kernels(backend, c.driver.VerifyTable(table), ev)
        assert_equal_kernels(backend, c.driver.VerifyTable(table, want_match=True), ev, want_match=True)
        again = assert_untouched(table, ev, want_match=True)
        assert (again.kernel_text_hash != 0) == (backend == "gpu")
    finally:
        table.free()


@pytest.mark.parametrize("backend", PLAIN)
def test_nothing_to_compare_without_a_specialised_kernel(backend, fixtures):
    """plain hostemu, and the device with GK_NO_JIT=1: zero differences, and the answer says that nothing was compared"""
    c = load(backend, fixtures)
    table = native_table(c, N_A)
    try:
        ev = table.eval()
        with flipped(c.driver.engine.lib, VIOL, 0, 0):   # (even a difference that is there is not looked for: there is no specialised side)
            v = c.driver.VerifyTable(table)
        assert v.specialised_groups == 0 and v.n_plan_groups == 1 and not v.ok and v.diff_total == 0 and v.kernel_text_hash == 0
        assert v.constraint_ids == [int(x) for x in ev.constraint_ids]
        assert_untouched(table, ev)
    finally:
        table.free()


# ------------------------------------------------------------------------------------------------ several plan groups
@pytest.mark.parametrize("backend", SPECIALISED)
def test_several_plan_groups(backend, fixtures):
    lib = make_client(backend).driver.engine.lib
    with plan_group_max(lib, 8):
        c = load(backend, fixtures)
        table = native_table(c, N_A)
        try:
            ev = table.eval(want_match=True)
            assert ev.n_plan_groups > 1
            assert_equal_kernels(backend, c.driver.VerifyTable(table, want_match=True), ev, want_match=True)
            row = 8 + 3   # a row of the second group, reported under its merged number
            with flipped(lib, VIOL, row, 77):
                v = c.driver.VerifyTable(table)
            assert v.diff_total == 1 and v.diff_viol[int(ev.constraint_ids[row])] == 1 and sum(v.diff_viol.values()) == 1 and not v.ok
            assert [(e.kind, e.constraint_id, e.review, e.specialised_bit) for e in v.entries] == [("viol", int(ev.constraint_ids[row]), 77, bit(ev.viol, row, 77))]
            assert v.specialised_groups == v.n_plan_groups == ev.n_plan_groups
            assert_untouched(table, ev, want_match=True)
        finally:
            table.free()


# ------------------------------------------------------------------------------------------------ injected differences
@pytest.mark.parametrize("backend", SPECIALISED)
def test_injected_differences(backend, fixtures):
    c = load(backend, fixtures)
    lib = c.driver.engine.lib
    table = native_table(c, N_A)
    try:
        ev = table.eval(want_match=True)
        nc = ev.n_constraints
        names = {cid: key for key, cid in c.driver._ids.items()}
        for kind, row, review in ((VIOL, 0, 0), (VIOL, nc - 1, 199), (ERR, 17, 64), (MATCH, 5, 130)):
            want_match = kind == MATCH
            with flipped(lib, kind, row, review):
                v = c.driver.VerifyTable(table, want_match=want_match)
            cid = int(ev.constraint_ids[row])
            counts = {"viol": v.diff_viol, "err": v.diff_err, "match": v.diff_match if want_match else {}}
            assert v.diff_total == 1 and v.entries_total == 1 and v.diff_too_big == 0 and not v.ok
            assert {(k, i): n for k, d in counts.items() for i, n in d.items() if n} == {(KINDS[kind], cid): 1}
            (e,) = v.entries
            assert (e.kind, e.constraint_id, e.review) == (KINDS[kind], cid, review) and (e.constraint_kind, e.constraint_name) == names[cid]
            assert e.specialised_bit == bit(getattr(ev, KINDS[kind]), row, review)
            assert v.specialised_groups == v.n_plan_groups == 1 and v.quarantined_groups == 0
        # a match flip is not looked at without the flag
        with flipped(lib, MATCH, 5, 130):
            assert c.driver.VerifyTable(table, want_match=True).diff_total == 1
        assert c.driver.VerifyTable(table).ok
        assert_untouched(table, ev, want_match=True)
    finally:
        table.free()


@pytest.mark.parametrize("backend", SPECIALISED)
def test_whole_word_flips(backend, fixtures):
    c = load(backend, fixtures)
    lib = c.driver.engine.lib
    table = native_table(c, N_A)
    try:
        ev = table.eval()
        row, cid = 7, int(ev.constraint_ids[7])
        with flipped(lib, VIOL, row, 3 * 64 + 2, whole=True):   # word 3 holds 8 reviews: the tail mask is real
            v = c.driver.VerifyTable(table)
        assert v.diff_total == 8 and v.diff_viol[cid] == 8 and v.entries_total == 8
        assert [(e.kind, e.constraint_id, e.review) for e in v.entries] == [("viol", cid, 192 + i) for i in range(8)]
        assert [e.specialised_bit for e in v.entries] == [bit(ev.viol, row, 192 + i) for i in range(8)]
        with flipped(lib, VIOL, row, 5, whole=True):   # word 0, more differences than the caller has room for
            v = c.driver.VerifyTable(table, max_entries=16)
        assert v.diff_total == 64 and v.entries_total == 64 and v.diff_viol[cid] == 64 and len(v.entries) == 16
        reviews = [e.review for e in v.entries]
        assert all((e.kind, e.constraint_id) == ("viol", cid) for e in v.entries) and all(0 <= r < 64 for r in reviews)
        assert reviews == sorted(set(reviews))
        assert all(e.specialised_bit == bit(ev.viol, row, e.review) for e in v.entries)
        with flipped(lib, VIOL, row, 5, whole=True):   # no room at all: the counts alone
            v = c.driver.VerifyTable(table, max_entries=0)
        assert v.diff_total == 64 and v.entries_total == 64 and v.entries == []
        assert_untouched(table, ev)
    finally:
        table.free()


@pytest.mark.parametrize("backend", SPECIALISED)
def test_two_waves_of_columns(backend, fixtures):
    """shape B: a difference in the last column (the one lane of the third wave) and one in the middle of the second wave"""
    c = load(backend, fixtures)
    lib = c.driver.engine.lib
    table = native_table(c, N_B)
    try:
        ev = table.eval()
        for row, review in ((49, N_B - 1), (2, 100 * 64 + 63)):
            with flipped(lib, ERR, row, review):
                v = c.driver.VerifyTable(table)
            assert v.diff_total == 1 and v.diff_err[int(ev.constraint_ids[row])] == 1
            assert [(e.kind, e.constraint_id, e.review, e.specialised_bit) for e in v.entries] == [("err", int(ev.constraint_ids[row]), review, bit(ev.err, row, review))]
        with flipped(lib, VIOL, 0, N_B - 1, whole=True):
            v = c.driver.VerifyTable(table)
        assert v.diff_total == 8 and [e.review for e in v.entries] == list(range(N_B - 8, N_B))
    finally:
        table.free()


# ------------------------------------------------------------------------------------------------ beyond the limits
@pytest.mark.parametrize("backend", SPECIALISED)
def test_review_beyond_the_limits_is_masked(backend, fixtures):
    c = load(backend, fixtures)
    lib = c.driver.engine.lib
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(70, seed=23, mixed=True)
    huge = {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "huge", "namespace": "prod-01"},
            "spec": {"containers": [{"name": "c%d" % i, "image": "x", "securityContext": {"privileged": i == 299}} for i in range(300)]}}
    at = 66
    objs.insert(at, huge)
    rins = [D.to_review_in(D.AugmentedUnstructured(D.Unstructured(o), synth.namespace_for(o, nss), "Original")) for o in objs]
    table = c.driver.engine.create_table(rins, keep_docs=False)
    try:
        ev = table.eval(host_eval=False)
        assert ev.too_big_reviews() == [at]
        v = c.driver.VerifyTable(table)
        assert v.ok and v.diff_too_big == 0 and v.specialised_groups == 1
        with flipped(lib, VIOL, 0, at):   # its bits are unspecified on either side: not compared
            v = c.driver.VerifyTable(table)
        assert v.ok and v.diff_total == 0 and v.entries == []
        with flipped(lib, VIOL, 0, at, whole=True):   # ... the other reviews of its word are
            v = c.driver.VerifyTable(table)
        assert v.diff_total == len(objs) - 64 - 1 and at not in [e.review for e in v.entries]
        with flipped(lib, TOO_BIG, 0, at):
            v = c.driver.VerifyTable(table)
        assert not v.ok and v.diff_too_big == 1 and v.diff_total == 1 and not any(v.diff_viol.values())
        assert [(e.kind, e.constraint_id, e.review, e.specialised_bit) for e in v.entries] == [("too_big", -1, at, 1)]
        with flipped(lib, TOO_BIG, 0, 3):   # a review the bytecode side alone declares beyond the limits: counted, and its column masked
            v = c.driver.VerifyTable(table)
        assert v.diff_too_big == 1 and v.diff_total == 1 and [(e.kind, e.review, e.specialised_bit) for e in v.entries] == [("too_big", 3, 0)]
        again = table.eval(host_eval=False)
        assert (again.viol == ev.viol).all() and (again.too_big == ev.too_big).all()
    finally:
        lib.gk_debug_set(b"verify_flip", -1)
        table.free()


# ------------------------------------------------------------------------------------------------ quarantine
@pytest.mark.parametrize("backend", SPECIALISED)
def test_quarantine(backend, fixtures, capfd):
    cons = synth.audit_constraints()
    c = load(backend, fixtures, cons[:-1])
    lib = c.driver.engine.lib
    table = native_table(c, N_A)
    try:
        ev = table.eval()
        with flipped(lib, VIOL, 2, 9):   # without the flag a difference changes nothing
            v = c.driver.VerifyTable(table)
        assert v.diff_total == 1 and v.quarantined_groups == 0
        again = assert_untouched(table, ev)
        assert (again.kernel_text_hash != 0) == (backend == "gpu")
        assert c.driver.VerifyTable(table).ok
        capfd.readouterr()
        with flipped(lib, VIOL, 2, 9):
            v = c.driver.VerifyTable(table, quarantine=True)
        assert v.diff_total == 1 and v.quarantined_groups == 1 and v.specialised_groups == 1
        assert "using the bytecode kernel for this plan" in capfd.readouterr().err
        # the plan is served by the bytecode kernel from now on: same answers, no specialised text, nothing to compare
        again = assert_untouched(table, ev)
        assert again.kernel_text_hash == 0
        v = c.driver.VerifyTable(table, quarantine=True)
        assert v.specialised_groups == 0 and not v.ok and v.diff_total == 0 and v.quarantined_groups == 0 and v.kernel_text_hash == 0
        other = native_table(c, 130, seed=5)   # ... for every table that evaluates the plan
        try:
            assert other.eval().kernel_text_hash == 0 and c.driver.VerifyTable(other).specialised_groups == 0
        finally:
            other.free()
        # a policy change builds new plans: specialised again, verified again
        c.AddConstraint(cons[-1])
        fresh = native_table(c, N_A)
        try:
            ev2 = fresh.eval()
            assert ev2.n_constraints == ev.n_constraints + 1 and (ev2.kernel_text_hash != 0) == (backend == "gpu")
            assert_equal_kernels(backend, c.driver.VerifyTable(fresh), ev2)
        finally:
            fresh.free()
    finally:
        table.free()


@pytest.mark.parametrize("backend", SPECIALISED)
def test_pending_launches_are_collected(backend, fixtures):
    """enqueue-only launches (GK_EVAL_ASYNC) that nobody collected yet: the verification's own evaluation collects them"""
    c = load(backend, fixtures)
    table = native_table(c, N_A)
    try:
        ev = table.eval()
        table.launch()
        table.launch()
        assert_equal_kernels(backend, c.driver.VerifyTable(table), ev)
        with flipped(c.driver.engine.lib, VIOL, 0, 1):
            table.launch()
            assert c.driver.VerifyTable(table).diff_total == 1
        assert_untouched(table, ev)
    finally:
        table.free()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("backend", [b for b in ALL if b.id in ("hostemu", "gpu")])
def test_refusals(backend, fixtures):
    c = make_client(backend)
    fx = fixtures
    t_priv = next(t for t in synth.psp_templates(fx) if t["spec"]["crd"]["spec"]["names"]["kind"] == "K8sPSPPrivilegedContainer")
    t_host = next(t for t in synth.psp_templates(fx) if t["spec"]["crd"]["spec"]["names"]["kind"] == "K8sPSPHostNamespace")
    c.AddTemplate(t_priv)
    c.AddTemplate(t_host)
    c.AddConstraint({"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": "K8sPSPPrivilegedContainer", "metadata": {"name": "p"}, "spec": {}})
    eng = c.driver.engine
    lib = eng.lib
    table = native_table(c, N_A)
    try:
        out = C.POINTER(L.gk_verify_out)()
        assert lib.gk_table_verify(None, table.handle, 0, 8, C.byref(out)) == L.GK_ERR_INVALID
        assert lib.gk_table_verify(eng.handle, None, 0, 8, C.byref(out)) == L.GK_ERR_INVALID
        assert lib.gk_table_verify(eng.handle, table.handle, 0, 8, None) == L.GK_ERR_INVALID
        assert lib.gk_resident_verify(None, 0, 8, C.byref(out), None) == L.GK_ERR_INVALID
        assert lib.gk_resident_verify(eng.handle, 0, 8, None, None) == L.GK_ERR_INVALID
        lib.gk_verify_free(None)
        c.driver.VerifyTable(table)
        if backend == "hostemu":   # a table set up as a shard: its bitmaps live in the exchange buffer (a communicator of one rank, CPU stand-in)
            gather, reduce_ = L.HE_ALLGATHER(lambda ctx, buf, n: None), L.HE_ALLREDUCE(lambda ctx, buf, n: None)
            assert lib.gk_comm_init_host(eng.handle, 0, 1, gather, reduce_, None) == 0
            shard = native_table(c, 70)
            try:
                so = C.POINTER(L.gk_shard_out)()
                assert lib.gk_table_sweep_sharded(eng.handle, shard.handle, 0, C.byref(so)) == 0
                lib.gk_shard_free(so)
                with pytest.raises(D.EngineError, match="set up as a shard") as ei:
                    c.driver.VerifyTable(shard)
                assert ei.value.code == L.GK_ERR_INVALID
            finally:
                shard.free()
                lib.gk_comm_destroy(eng.handle)
        # a constraint that needs rows the table does not hold makes it stale, as for gk_table_eval
        c.AddConstraint({"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": "K8sPSPHostNamespace", "metadata": {"name": "h"}, "spec": {}})
        with pytest.raises(D.EngineError, match="create it again"):
            table.eval()
        with pytest.raises(D.EngineError, match="create it again") as ei:
            c.driver.VerifyTable(table)
        assert ei.value.code == L.GK_ERR_INVALID
        assert lib.gk_debug_set(b"verify_flip", -1) == 0
    finally:
        table.free()


# ------------------------------------------------------------------------------------------------ the resident set
@pytest.mark.parametrize("backend", SPECIALISED)
def test_resident(backend, fixtures):
    c = load(backend, fixtures)
    lib = c.driver.engine.lib
    nss = list(synth.gen_namespaces().values())
    objs = [o for o in synth.gen_objects(230, seed=23, mixed=True) if o.get("kind") != "Namespace"][:200]
    first, second = nss + objs[:100], objs[100:]
    for o in first:
        c.AddData(o)
    v = c.driver.VerifyResident()
    assert v.ok and v.n_reviews == len(first) and v.specialised_groups == v.n_plan_groups == 1
    for o in second:
        c.AddData(o)
    gone = first[len(nss) + 10]
    c.RemoveData(gone)
    sweep = c.driver.ResidentSweep()
    assert sweep["n_chunks"] == 2 and sweep["n_objects"] == len(first) + len(second) - 1
    v = c.driver.VerifyResident(want_match=True)
    assert v.ok and v.n_reviews == len(first) + len(second) and v.specialised_groups == v.n_plan_groups == 2 and v.entries == []
    assert sorted(v.constraint_ids) == sorted(sweep["pairs"])
    assert (v.kernel_text_hash != 0) == (backend == "gpu")
    # slots are handed out in the order the objects arrived; a flip names the object by its inventory path
    for slot, obj in ((len(nss) + 11, first[len(nss) + 11]), (len(first) + 42, second[42]), (3, nss[3])):
        with flipped(lib, VIOL, 1, slot):
            v = c.driver.VerifyResident()
        assert v.diff_total == 1 and not v.ok and v.diff_viol[v.constraint_ids[1]] == 1
        (e,) = v.entries
        assert (e.kind, e.constraint_id, e.review) == ("viol", v.constraint_ids[1], slot) and list(e.path) == D.process_data(obj)
    with flipped(lib, VIOL, 1, len(nss) + 10):   # the removed object's slot is dead: not compared
        v = c.driver.VerifyResident()
    assert v.ok and v.entries == []
    with flipped(lib, VIOL, 1, len(nss) + 10, whole=True):   # ... its neighbours in the word are
        v = c.driver.VerifyResident(max_entries=100)
    assert v.diff_total == 63 and len(v.entries) == 63 and tuple(D.process_data(gone)) not in [e.path for e in v.entries]
    assert c.driver.ResidentSweep()["pairs"] == sweep["pairs"]


@pytest.mark.parametrize("backend", SPECIALISED)
def test_verify_audit(backend, fixtures):
    """Client.VerifyAudit: the table the audit sweeps (resident: a table-sized plan variant, audit process)"""
    c = load(backend, fixtures)
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(N_A, seed=31, mixed=True)
    rv = [D.AugmentedUnstructured(D.Unstructured(o), synth.namespace_for(o, nss), "Original") for o in objs]
    v = c.VerifyAudit(rv)
    assert v.ok and v.n_reviews == N_A and v.specialised_groups == v.n_plan_groups == 1 and len(v.constraint_ids) == 50
    with flipped(c.driver.engine.lib, ERR, 49, 64):
        v = c.VerifyAudit(rv)
    assert v.diff_total == 1 and [(e.kind, e.review) for e in v.entries] == [("err", 64)]
    assert json.dumps(D.dataclasses.asdict(v))   # (plain data)
