"""gk_table_changes with GK_CHANGES_DEVICE_JOIN: the same stream, the two cycles' object keys joined on the device (gk_kjoin_build +
gk_kjoin_probe + gk_kjoin_finish; tests/native/hostemu_kjoin.cpp on the CPU build) instead of merged on the host.

Cycle, expected() and got_entries() are tests/test_table_changes.py's: the expected entries come from two complete gk_table_violations
streams joined by object name in Python, nothing of the new code.  Every case reads the device-join stream against a snapshot taken with
its device keys and again against one taken without them (their upload at the first device join), at three page sizes, compares it with
expected() and, entry by entry, with the host-join stream, and asks gk_table_changes_join how the stream was joined.  The join alone, at
the shapes where the kernels can go wrong: tests/test_table_join.py."""
import pytest

from gatekeeper_amd import _lib as L
from gatekeeper_amd import synth
from test_table_changes import (GONE, NEW, NONE, PAGES, TABLE_BACKENDS, VERSION, Cycle, big_pod, check_apply, deny_client, expected, got_entries, name_of, psp_client)
from parity_util import plan_group_max
from test_table_violations import NS_A, cm, delete_without_old_object, deny, kinds_client, rin, violated_rows
from gatekeeper_amd import driver as D


def check_device_join(then, now, use_versions=True, sizes=PAGES, resolved=None):
    """the device-join stream against both kinds of snapshot of `then` == expected() == the host-join stream -> the expected entries"""
    want = expected(then, now, use_versions)
    vers = now.versions if use_versions else None
    v_then = then.versions if use_versions else None
    snaps = [then.table.snapshot(v_then, device_keys=True), then.table.snapshot(v_then)]
    try:
        assert snaps[0].info()["host_bytes"] < snaps[1].info()["host_bytes"]      # (no key order was built)
        for snap in snaps:
            for size in sizes:
                got = got_entries(now.table.change_pages(snap, size, versions=vers, device_join=True))
                assert got == want, (size, [x for x in got if x not in want][:5], [x for x in want if x not in got][:5])
                st = now.table.changes_join()
                assert (st["device"], st["fallback"], st["n_now"], st["n_then"]) == (1, 0, now.n, then.n), st
                if resolved is not None:
                    assert (st["host_resolved_now"], st["host_resolved_then"]) == resolved
            host = got_entries(now.table.change_pages(snap, sizes[0], versions=vers))    # flags 0 -- against the first snapshot: its key order is built here
            assert host == want
            st = now.table.changes_join()
            assert (st["device"], st["fallback"], st["capacity"]) == (0, 0, 0)
        check_apply(then, now, want)
        return want
    finally:
        for s in snaps:
            s.free()


def listing(names, n, order, changed=(), removed=(), added=0):
    """n objects with the labels violated_rows gives them, in `order`; `changed` flip one label, `removed` are left out, `added` new ones"""
    nc = len(names)
    out = []
    for i in order:
        if i in removed:
            continue
        rows = set(violated_rows(i, n, nc))
        if i in changed:
            rows ^= {i % nc}
        out.append(cm(i, [names[j] for j in sorted(rows)]))
    return out + [cm(9000 + k, [names[k % nc]]) for k in range(added)]


def cycles_of(eng, objs_then, objs_now, **kw):
    return Cycle(eng, [rin(o) for o in objs_then], [name_of(o) for o in objs_then], **kw), Cycle(eng, [rin(o) for o in objs_now], [name_of(o) for o in objs_now], **kw)


CASES = {"changed-answers": dict(order=range(130), changed=set(range(0, 130, 3))),
         "shuffled": dict(order=[(i * 37) % 130 for i in range(130)], changed={5, 64, 65, 129}),
         "gone-and-new": dict(order=reversed(range(130)), changed={7}, removed={0, 5, 63, 64, 129}, added=4)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_the_stream_is_the_host_joins_stream(backend, case):
    names = ["l%03d" % j for j in range(5)]
    eng = deny_client(backend, names).driver.engine
    then, now = cycles_of(eng, listing(names, 130, range(130)), listing(names, 130, **CASES[case]))
    try:
        want = check_device_join(then, now, resolved=(0, 0))
        assert want
        if case == "gone-and-new":
            assert {e[6] for e in want} >= {GONE, NEW, 0}
    finally:
        then.free()
        now.free()


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_duplicated_rejected_and_excluded_reviews(backend):
    c = kinds_client(backend)
    eng = c.driver.engine
    dup_a, dup_b, dup_c = cm(7, ["l0"]), cm(7, ["l1"]), cm(7, ["l0", "l1"])
    then_r = [(rin(cm(0, ["l0"]), NS_A), "obj-0000"), (D.to_review_in(delete_without_old_object()), None), (rin(cm(4, []), NS_A), "obj-0004"),
              (rin(dup_a, NS_A), "obj-0007"), (rin(dup_b, NS_A), "obj-0007"), (rin(cm(8, ["l1"]), NS_A), "obj-0008")]
    now_r = [(rin(dup_b, NS_A), "obj-0007"), (D.to_review_in(delete_without_old_object()), None), (rin(cm(4, [])), "obj-0004"), (rin(dup_b, NS_A), "obj-0007"),
             (rin(dup_c, NS_A), "obj-0007"), (rin(cm(0, ["l0"]), NS_A), "obj-0000")]
    then = Cycle(eng, [r for r, _ in then_r], [k for _, k in then_r], process="audit")
    now = Cycle(eng, [r for r, _ in now_r], [k for _, k in now_r], process="audit")
    try:
        want = check_device_join(then, now, sizes=(64,), resolved=(3, 2))
        assert [(e[0], e[1], e[6]) for e in want] == [(0, 3, 0), (2, 2, 0), (4, NONE, NEW), (NONE, 5, GONE)]
    finally:
        then.free()
        now.free()


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_versions(backend):
    names = ["l0", "l1"]
    eng = deny_client(backend, names).driver.engine
    objs = [cm(i, [names[i % 2]] if i % 3 else []) for i in range(150)]
    v_then = [1000 + i for i in range(150)]
    v_now = [v + (1 if i % 4 == 0 else 0) for i, v in enumerate(v_then)]
    then = Cycle(eng, [rin(o) for o in objs], [name_of(o) for o in objs], versions=v_then)
    now = Cycle(eng, [rin(o) for o in reversed(objs)], [name_of(o) for o in reversed(objs)], versions=list(reversed(v_now)))
    try:
        want = check_device_join(then, now, sizes=(64, 1000000))
        assert sorted(e[1] for e in want) == [i for i in range(150) if i % 4 == 0 and i % 3] and all(e[6] == VERSION for e in want)
    finally:
        then.free()
        now.free()


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_a_review_the_host_evaluation_answered_on_either_side(backend):
    """now_of of the device join feeds delta_known_build: the host-known review keeps its masks of both sides"""
    c, _ = psp_client(backend)
    eng = c.driver.engine
    nss = synth.gen_namespaces()
    base = synth.gen_objects(70, seed=5, mixed=True)

    def cycle(pod, order):
        objs = list(base)
        objs[66] = pod
        return Cycle(eng, [rin(objs[i], synth.namespace_for(objs[i], nss), "Original") for i in order], ["pos-%d" % i for i in order])

    small, huge = big_pod("huge-66", False, 2), big_pod("huge-66", True)
    # (both listings are `base` in one order, so equal keys -- should the generator repeat a name -- pair up by position)
    for pod_then, pod_now in ((small, huge), (huge, small)):
        then, now = cycle(pod_then, range(70)), cycle(pod_now, range(70))
        try:
            want = check_device_join(then, now, sizes=(64,))
            assert [e[0] for e in want] == [66] and want[0][1] == 66 and (want[0][2] or want[0][4]) and want[0][2] != want[0][4]
        finally:
            then.free()
            now.free()


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_three_plan_groups(backend):
    names = ["l%03d" % j for j in range(130)]
    lib = L.load(hostemu=backend.startswith("hostemu"))
    with plan_group_max(lib, 50):
        eng = deny_client(backend, names).driver.engine
        then, now = cycles_of(eng, listing(names, 130, range(130)), listing(names, 130, reversed(range(130)), changed=set(range(0, 130, 2)), removed={3}, added=2))
        try:
            assert now.table.eval().n_plan_groups == 3
            want = check_device_join(then, now, sizes=(64, 1000000))
            assert len(want) > 64
        finally:
            then.free()
            now.free()


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_constraint_set_changed_between_the_cycles(backend):
    names = ["l0", "l1", "l2", "l3"]
    c = deny_client(backend, names[:3])
    eng = c.driver.engine
    objs = [cm(i, [names[j] for j in range(4) if (i >> j) & 1]) for i in range(80)]
    then = Cycle(eng, [rin(o) for o in objs], [name_of(o) for o in objs])
    snaps = [then.table.snapshot(device_keys=True), then.table.snapshot()]
    then.free()                                                                   # the snapshots, device keys included, outlive the table
    now = None
    try:
        c.RemoveConstraint(deny("l1"))
        c.AddConstraint(deny("l3"))
        now = Cycle(eng, [rin(o) for o in reversed(objs)], [name_of(o) for o in reversed(objs)])
        want = expected(then, now)
        assert want and all(e[6] == 0 for e in want)
        for snap in snaps:
            for size in PAGES:
                assert got_entries(now.table.change_pages(snap, size, device_join=True)) == want
                assert now.table.changes_join()["device"] == 1
            assert got_entries(now.table.change_pages(snap, 64)) == want
        check_apply(then, now, want)
    finally:
        for s in snaps:
            s.free()
        if now:
            now.free()


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_without_a_snapshot_nothing_is_joined(backend):
    names = ["l0", "l1", "l2"]
    eng = deny_client(backend, names).driver.engine
    objs = listing(names, 100, range(100))
    now = Cycle(eng, [rin(o) for o in objs], [name_of(o) for o in objs])
    try:
        with pytest.raises(D.EngineError):
            now.table.changes_join()                                              # no stream yet
        want = expected(None, now)
        for size in PAGES:
            assert got_entries(now.table.change_pages(None, size, device_join=True)) == want
        st = now.table.changes_join()
        assert (st["device"], st["fallback"], st["n_now"], st["n_then"], st["capacity"]) == (0, 0, 100, 0, 0)
        assert want and all(e[6] == NEW for e in want)
    finally:
        now.free()


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_a_snapshots_device_keys_count_in_its_device_bytes(backend):
    names = ["l0"]
    eng = deny_client(backend, names).driver.engine
    objs = listing(names, 100, range(100))
    one = Cycle(eng, [rin(o) for o in objs], [name_of(o) for o in objs])
    plain, keyed = one.table.snapshot(), one.table.snapshot(device_keys=True)
    try:
        # a ConfigMap's key: \0 v1 \0 ConfigMap \0 default \0 obj-NNNN = 30 bytes; its record, 4 + 30 rounded up to 16: 48; its offset: 4
        packed = 100 * (48 + 4)
        assert keyed.info()["device_bytes"] - plain.info()["device_bytes"] == packed
        got_entries(one.table.change_pages(plain, 64, device_join=True))           # the first device join uploads the plain snapshot's keys
        assert plain.info()["device_bytes"] == keyed.info()["device_bytes"]
        # ... and a host join against the keyed one builds its key order: the same stream (nothing changed), the order now counted
        before = keyed.info()["host_bytes"]
        assert got_entries(one.table.change_pages(keyed, 64)) == [] and keyed.info()["host_bytes"] == before + 100 * 4 == plain.info()["host_bytes"]
    finally:
        plain.free()
        keyed.free()
        one.free()
