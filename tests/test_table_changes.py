"""Row a11, the list-based audit from one cycle to the next: gk_table_snapshot keeps a table's answer, gk_table_changes of a LATER table
streams only what differs -- objects joined by key, bitmap rows by constraint id (gk_tchg_align + gk_tchg_index + gk_tchg_emit;
tests/native/hostemu_tchg.cpp on the CPU build).

Expected answers use nothing of the new code: two complete gk_table_violations streams of two separately built tables (checked against
numpy over the bitmaps of a downloading eval(): test_table_violations' reference), joined by object name in Python with the contract's
rules; where the construction says what must change, that as well.  Every case also checks the defining property: applying the entries
in order (state[key] := now, delete when now is empty) to the then-state gives the now-state, except for objects beyond the limits now.
The pure join / row map / cursor / index / merge logic and the stand-in's loops: tests/test_table_delta_native.py."""
import contextlib

import pytest

from gatekeeper_amd import _lib as L
from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from oracle import client as OC
from oracle import excluder as OX
from parity_util import BACKENDS, load_both, make_client, plan_group_max, to_oracle_review
from test_table_violations import (DENY_LABEL, MOVED, NS_A, NS_HIDDEN, cm, delete_without_old_object, deny, entries_of, kinds_client, reference, rin, tmpl,
                                   violated_rows)

TABLE_BACKENDS = [b for b in BACKENDS if b.id in ("hostemu", "gpu")]
C = L.C
PAGES = (64, 100, 1000000)
NONE = 0xFFFFFFFF
GONE, NEW, VERSION = L.GK_CHANGE_GONE, L.GK_CHANGE_NEW, L.GK_CHANGE_VERSION


class Cycle:
    """one built and evaluated table with what a complete gk_table_violations stream says of it, by constraint id"""

    def __init__(self, eng, rins, keys, versions=None, process=None, **eval_kw):
        self.table = eng.create_table(rins, process=process) if process else eng.create_table(rins)
        self.keys, self.versions, self.n = self.occurrences(keys), versions, len(rins)
        self.evaluate(**eval_kw)

    @staticmethod
    def occurrences(keys):
        """(name, i) for the i-th review of that name; None: a review without a key"""
        seen, out = {}, []
        for k in keys:
            if k is None:
                out.append(None)
                continue
            seen[k] = seen.get(k, -1) + 1
            out.append((k, seen[k]))
        return out

    def evaluate(self, **eval_kw):
        ev = self.table.eval(**eval_kw)
        self.ids = [int(x) for x in ev.constraint_ids]
        self.beyond = set(ev.too_big_reviews())
        want = reference(ev, skip=self.beyond)
        pages = list(self.table.violation_pages(1000000))
        assert entries_of(pages) == want and pages[0]["beyond_limits"] == len(self.beyond)   # the stream IS the reference
        self.res = {r: (frozenset(self.ids[j] for j in v), frozenset(self.ids[j] for j in e)) for r, (v, e) in want.items()}
        return ev

    def state(self):
        return {self.keys[r]: x for r, x in self.res.items()}

    def free(self):
        self.table.free()


EMPTY = (frozenset(), frozenset())


def expected(then, now, use_versions=True):
    """the entries the contract asks for, in stream order: (review, was_review, viol ids, err ids, was_viol ids, was_err ids, flags)"""
    live = set(now.ids)
    p_of = {k: p for p, k in enumerate(then.keys) if k is not None} if then else {}
    versions = use_versions and then is not None and then.versions is not None and now.versions is not None
    out, matched = [], set()
    for r, k in enumerate(now.keys):
        p = p_of.get(k) if k is not None else None
        if p is not None:
            matched.add(p)
        if r in now.beyond:
            continue
        cur = now.res.get(r, EMPTY)
        was = tuple(frozenset(x for x in s if x in live) for s in then.res.get(p, EMPTY)) if p is not None else EMPTY
        moved = versions and p is not None and then.versions[p] != now.versions[r]
        if cur != was or (moved and cur != EMPTY):
            out.append((r, NONE if p is None else p, sorted(cur[0]), sorted(cur[1]), sorted(was[0]), sorted(was[1]), (NEW if p is None else 0) | (VERSION if moved else 0)))
    for p in range(then.n if then else 0):
        if p in matched:
            continue
        was = tuple(frozenset(x for x in s if x in live) for s in then.res.get(p, EMPTY))
        if was != EMPTY:
            out.append((NONE, p, [], [], sorted(was[0]), sorted(was[1]), GONE))
    return out


def got_entries(pages):
    out = []
    for pg in pages:
        ids = pg["ids"]

        def named(mask_row):
            return sorted(ids[w * 64 + b] for w, m in enumerate(mask_row) for b in range(64) if (int(m) >> b) & 1)
        for i in range(len(pg["keys"])):
            out.append((int(pg["reviews"][i]), int(pg["was_reviews"][i]), named(pg["viol"][i]), named(pg["err"][i]), named(pg["was_viol"][i]), named(pg["was_err"][i]),
                        pg["flags"][i]))
    return out


def check_changes(then, now, snap, sizes=PAGES, use_versions=True, was_beyond=None):
    """the stream of every page size: exactly the expected entries in order, whole words of one side per page, the totals on every page,
    the keys name the objects, and applying the entries to the then-state gives the now-state"""
    want = expected(then, now, use_versions)
    vers = now.versions if use_versions else None
    for size in sizes:
        pages = list(now.table.change_pages(snap, size, versions=vers))
        got = got_entries(pages)
        assert got == want, (size, [x for x in got if x not in want][:5], [x for x in want if x not in got][:5])
        at = 0
        for k, p in enumerate(pages):
            n = len(p["keys"])
            assert p["total_entries"] == len(want) and p["beyond_limits"] == len(now.beyond) and p["n_reviews"] == now.n
            assert p["n_then"] == (then.n if then else 0) and p["reset"] == (0 if snap is not None else 1) and p["ids"] == now.ids
            assert p["was_beyond_limits"] == (was_beyond if was_beyond is not None else len(then.beyond) if then else 0)
            assert n <= max(size, 64) and (n or len(pages) == 1)                 # no empty page inside a stream
            assert (p["next_cursor"] != 0) == (k + 1 < len(pages))
            sides = {f & GONE for f in p["flags"]}
            assert len(sides) <= 1                                                # one side per page
            words = {(f & GONE, int(r if not f & GONE else q) // 64) for f, r, q in zip(p["flags"], p["reviews"], p["was_reviews"])}
            before = {(e[6] & GONE, (e[0] if not e[6] & GONE else e[1]) // 64) for e in want[:at]}
            assert not words & before                                             # whole words
            for i in range(n):                                                    # the key names the object
                e = want[at + i]
                name = now.keys[e[0]][0] if e[0] != NONE else then.keys[e[1]][0]
                assert p["keys"][i][4] == name and len(p["keys"][i]) == 5, (p["keys"][i], name)
            at += n
        if size == 64 and len(want) > 64:
            assert len(pages) > 1
    check_apply(then, now, want)
    return want


def check_apply(then, now, want):
    """the defining property: the entries applied in order to the then-state give the now-state, but for the objects beyond the limits now"""
    live = set(now.ids)
    state = {k: tuple(frozenset(x for x in s if x in live) for s in v) for k, v in (then.state() if then else {}).items()}
    state = {k: v for k, v in state.items() if v != EMPTY}
    for r, p, viol, err, _wv, _we, _f in want:
        key = now.keys[r] if r != NONE else then.keys[p]
        if viol or err:
            state[key] = (frozenset(viol), frozenset(err))
        else:
            state.pop(key, None)
    held = {now.keys[r] for r in now.beyond}
    assert {k: v for k, v in state.items() if k not in held} == {k: v for k, v in now.state().items() if k not in held}


def deny_client(backend, names):
    c = make_client(backend)
    c.AddTemplate(tmpl("K8sDenyLabel", DENY_LABEL))
    for x in names:
        c.AddConstraint(deny(x))
    return c


# ------------------------------------------------------------------------------------------------ 1. shapes
SHAPES = {(1, 1): ([], 0), (64, 65): ([5, 17, 40], 4), (65, 64): ([5, 17, 40], 2), (200, 197): ([5, 17, 40, 130, 131], 2),
          (4133, 4100): ([5, 17, 40] + list(range(128, 160)), 2)}


def changed_at(q, n):
    """whether the object at position q of an n-review second listing differs from the first: word 0 all, word 1 (of a table with one) none,
    the five last words of a large table none, elsewhere every third"""
    w = q // 64
    if w == 0:
        return True
    if (w == 1 and n >= 128) or (n > 1000 and w >= (n + 63) // 64 - 5):
        return False
    return q % 3 == 0


def two_listings(names, n_then, n_now):
    """-> (then objects, now objects).  The second listing is the first reversed -- every gather crosses words -- without the objects
    removed (from full words of the first) and with new ones in its last, partial word"""
    nc = len(names)
    removed, added = SHAPES[(n_then, n_now)]
    then = [cm(i, [names[j] for j in violated_rows(i, n_then, nc)]) for i in range(n_then)]
    now = []
    for q, i in enumerate(i for i in reversed(range(n_then)) if i not in removed):
        rows = set(violated_rows(i, n_then, nc))
        if changed_at(q, n_now):
            rows ^= {q % nc}
        now.append(cm(i, [names[j] for j in sorted(rows)]))
    for k in range(added):
        q = len(now)
        now.append(cm(9000 + k, [names[q % nc]] if n_now <= 1000 else []))
    assert len(now) == n_now
    return then, now


def name_of(o):
    return o["metadata"]["name"]


@pytest.mark.parametrize("nc", [1, 65, 130])
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_shapes_where_the_kernels_can_go_wrong(backend, nc):
    names = ["l%03d" % j for j in range(nc)]
    c = deny_client(backend, names)
    eng = c.driver.engine
    for n_then, n_now in SHAPES:
        objs_then, objs_now = two_listings(names, n_then, n_now)
        then = Cycle(eng, [rin(o) for o in objs_then], [name_of(o) for o in objs_then])
        snap = then.table.snapshot()
        now = None
        try:
            info = snap.info()
            assert info["n_reviews"] == n_then and info["constraint_ids"] == then.ids and info["beyond_limits"] == 0 and info["device_bytes"] > 0
            then.free()                                                           # the snapshot outlives its table
            now = Cycle(eng, [rin(o) for o in objs_now], [name_of(o) for o in objs_now])
            want = check_changes(then, now, snap)
            now_side = {e[0] for e in want if e[0] != NONE}
            if n_now >= 64:
                assert all(q in now_side for q in range(64))                      # a now-word with 64 entries
            if n_now >= 197:
                assert not any(64 <= q < 128 for q in now_side)                   # a now-word with none
            if n_now == 4100:
                assert max(now_side) // 64 <= 59 and max(e[1] for e in want if e[6] & GONE) // 64 <= 2   # empty words at the end of both sides
            assert {e[1] for e in want if e[6] & GONE} == {p for p in SHAPES[(n_then, n_now)][0] if violated_rows(p, n_then, nc)}
            now.table.eval(download=False)                                        # the same stream from bitmaps that never came back
            assert got_entries(now.table.change_pages(snap, 100)) == want
        finally:
            snap.free()
            then.free()
            if now:
                now.free()


# ------------------------------------------------------------------------------------------------ 2. / 3. no snapshot, nothing in between
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_without_a_snapshot_the_stream_is_the_whole_state(backend):
    names = ["l%03d" % j for j in range(65)]
    c = deny_client(backend, names)
    objs = [cm(i, [names[j] for j in violated_rows(i, 200, 65)]) for i in range(200)]
    now = Cycle(c.driver.engine, [rin(o) for o in objs], [name_of(o) for o in objs])
    try:
        want = check_changes(None, now, None)
        viol = list(now.table.violation_pages(1000000))
        assert [(e[0], e[2], e[3]) for e in want] == [(r, sorted(now.ids[j] for j in v), sorted(now.ids[j] for j in e)) for r, (v, e) in sorted(entries_of(viol).items())]
        assert want and all(e[6] == NEW and e[1] == NONE and not e[4] and not e[5] for e in want)
    finally:
        now.free()


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_a_snapshot_and_changes_with_nothing_in_between(backend):
    names = ["l%03d" % j for j in range(3)]
    c = deny_client(backend, names)
    eng = c.driver.engine
    objs = [cm(i, [names[j] for j in violated_rows(i, 200, 3)]) for i in range(200)]
    one = Cycle(eng, [rin(o) for o in objs], [name_of(o) for o in objs])
    snap = one.table.snapshot()
    two = None
    try:
        pages = list(one.table.change_pages(snap, 64))
        assert len(pages) == 1 and pages[0]["total_entries"] == 0 and not pages[0]["keys"] and pages[0]["reset"] == 0 and pages[0]["next_cursor"] == 0
        one.free()
        two = Cycle(eng, [rin(o) for o in objs], [name_of(o) for o in objs])        # the same listing in a new table, after the first is gone
        assert check_changes(one, two, snap) == []
        assert snap.info()["n_constraints"] == 3 and snap.info()["host_bytes"] > 0
    finally:
        snap.free()
        one.free()
        if two:
            two.free()


# ------------------------------------------------------------------------------------------------ 4. plan groups
def group_changes(backend, nc, max_then, max_now):
    """the changes between two listings of 200 / 197 objects, the snapshot taken under one split into plan groups, the table evaluated
    under another -> (entries by constraint NAME, groups then, groups now)"""
    names = ["l%03d" % j for j in range(nc)]
    objs_then, objs_now = two_listings(names, 200, 197)
    lib = L.load(hostemu=backend.startswith("hostemu"))
    c = None
    with (plan_group_max(lib, max_then) if max_then else contextlib.nullcontext()):
        c = deny_client(backend, names)
        eng = c.driver.engine
        then = Cycle(eng, [rin(o) for o in objs_then], [name_of(o) for o in objs_then])
        g_then = then.table.eval().n_plan_groups
        snap = then.table.snapshot()
        then.free()
    label = {c.driver.constraint_id(deny(x)): x for x in names}
    now = None
    try:
        with (plan_group_max(lib, max_now) if max_now else contextlib.nullcontext()):
            if max_now != max_then:
                c.AddConstraint(deny("zz-extra"))                                 # a policy change: the plans are cut again, under the other limit
                c.RemoveConstraint(deny("zz-extra"))
            now = Cycle(eng, [rin(o) for o in objs_now], [name_of(o) for o in objs_now])
            g_now = now.table.eval().n_plan_groups
            want = check_changes(then, now, snap, sizes=(64, 1000000))
        return [(e[0], e[1]) + tuple([label[x] for x in s] for s in e[2:6]) + (e[6],) for e in want], g_then, g_now
    finally:
        snap.free()
        if now:
            now.free()


@pytest.mark.parametrize("nc,group_max,groups", [(130, 50, 3), (50, 5, 10)], ids=["130-by-50", "50-by-5"])
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_plan_groups_stream_what_one_plan_streams(backend, nc, group_max, groups):
    """row0 = 0, 50, 100: the middle group's rows straddle bit 64 of the masks; ten groups: the descriptors go through device memory"""
    one, a, b = group_changes(backend, nc, None, None)
    many, c, d = group_changes(backend, nc, group_max, group_max)
    assert (a, b, c, d) == (1, 1, groups, groups)
    assert sorted(many) == sorted(one) and [e[:2] for e in many] == [e[:2] for e in one] and len(one) > 64


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_a_snapshot_under_three_groups_against_a_one_plan_table(backend):
    one, _, _ = group_changes(backend, 130, None, None)
    mixed, g_then, g_now = group_changes(backend, 130, 50, None)
    assert (g_then, g_now) == (3, 1)
    assert sorted(mixed) == sorted(one) and [e[:2] for e in mixed] == [e[:2] for e in one]


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_more_mask_words_than_the_kernel_keeps_in_registers(backend):
    got, g_then, g_now = group_changes(backend, 260, None, None)
    assert g_then >= 2 and g_now >= 2
    assert any("l259" in e[2] or "l259" in e[4] for e in got) and len(got) > 64


# ------------------------------------------------------------------------------------------------ 5. another constraint set
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_constraint_set_changed_between_the_cycles(backend):
    names = ["l0", "l1", "l2", "l3", "l4", "l7"]
    c = deny_client(backend, names[:5])
    eng = c.driver.engine
    objs = [cm(i, [names[j] for j in range(6) if (i >> j) & 1]) for i in range(64)] + [cm(64 + i, []) for i in range(70)]
    then = Cycle(eng, [rin(o) for o in objs], [name_of(o) for o in objs])
    snap = then.table.snapshot()
    id_then = {x: c.driver.constraint_id(deny(x)) for x in names[:5]}
    then.free()
    now = None
    try:
        c.RemoveConstraint(deny("l1"))                                            # removed
        c.AddConstraint(deny("l7"))                                               # added
        c.RemoveConstraint(deny("l2"))
        c.AddConstraint(deny("l2"))                                               # replaced: the same kind and name, a new id
        id_now = {x: c.driver.constraint_id(deny(x)) for x in ("l0", "l2", "l3", "l4", "l7")}
        assert id_now["l2"] != id_then["l2"] and id_now["l0"] == id_then["l0"]
        now = Cycle(eng, [rin(o) for o in objs], [name_of(o) for o in objs])
        assert sorted(now.ids) == sorted(id_now.values())
        want = check_changes(then, now, snap)
        pages = list(now.table.change_pages(snap, 64))
        assert all(p["reset"] == 0 and p["ids"] == now.ids for p in pages)
        seen = {x for e in want for s in e[2:6] for x in s}
        assert id_then["l1"] not in seen and id_then["l2"] not in seen            # the removed one and the replaced one's old id: nowhere
        # exactly the objects that carry l2 or l7 have entries: l2 and l7 are entirely new, l0 / l3 / l4 did not change
        assert [e[0] for e in want] == [i for i in range(64) if (i >> 2) & 1 or (i >> 5) & 1]
        for e in want:
            i = e[0]
            assert id_now["l2"] not in e[4] and id_now["l7"] not in e[4] and e[6] == 0
            assert e[4] == sorted(id_now[x] for j, x in ((0, "l0"), (3, "l3"), (4, "l4")) if (i >> j) & 1)
    finally:
        snap.free()
        if now:
            now.free()


# ------------------------------------------------------------------------------------------------ 6. versions
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_versions(backend):
    names = ["l0", "l1"]
    c = deny_client(backend, names)
    eng = c.driver.engine
    objs = [cm(i, [names[i % 2]] if i % 3 else []) for i in range(150)]
    v_then = [1000 + i for i in range(150)]
    v_now = [v + (1 if i % 4 == 0 else 0) for i, v in enumerate(v_then)]
    v_now[149] = 2 ** 64 - 1
    then = Cycle(eng, [rin(o) for o in objs], [name_of(o) for o in objs], versions=v_then)
    now = Cycle(eng, [rin(o) for o in objs], [name_of(o) for o in objs], versions=v_now)
    snap, bare = then.table.snapshot(v_then), then.table.snapshot()
    try:
        want = check_changes(then, now, snap, sizes=(64, 1000000))
        # equal masks everywhere: an entry iff the version differs and the object has a result now
        assert [e[0] for e in want] == [i for i in range(150) if (i % 4 == 0 or i == 149) and i % 3]
        assert all(e[6] == VERSION and e[2:4] == e[4:6] and e[2] for e in want)
        assert got_entries(now.table.change_pages(bare, 64, versions=v_now)) == []      # no versions in the snapshot
        assert got_entries(now.table.change_pages(snap, 64)) == []                      # none given now
    finally:
        snap.free()
        bare.free()
        then.free()
        now.free()


# ------------------------------------------------------------------------------------------------ 7. the kinds of review
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_autoreject_excluded_rejected_and_duplicated_reviews(backend):
    c = kinds_client(backend)
    eng = c.driver.engine
    dup_a, dup_b, dup_c = cm(7, ["l0"]), cm(7, ["l1"]), cm(7, ["l0", "l1"])
    then_r = [(rin(cm(0, ["l0"]), NS_A), "obj-0000"),
              (rin(cm(1, [])), "obj-0001"),                            # its Namespace is not cached: the namespaceSelector constraint autorejects
              (rin(cm(2, ["l0"], "hidden"), NS_HIDDEN), "obj-0002"),   # excluded
              (D.to_review_in(delete_without_old_object()), None),     # rejected: no key
              (rin(cm(4, []), NS_A), "obj-0004"),
              (rin(dup_a, NS_A), "obj-0007"), (rin(dup_b, NS_A), "obj-0007"),
              (rin(cm(8, ["l1"]), NS_A), "obj-0008")]
    now_r = [(rin(dup_b, NS_A), "obj-0007"),                           # first occurrence: was dup_a
             (D.to_review_in(delete_without_old_object()), None),
             (rin(cm(4, [])), "obj-0004"),                             # autoreject appears
             (rin(cm(1, []), NS_A), "obj-0001"),                       # autoreject disappears
             (rin(dup_b, NS_A), "obj-0007"),                           # second occurrence: unchanged
             (rin(cm(2, ["l0", "l1"], "hidden"), NS_HIDDEN), "obj-0002"),
             (rin(dup_c, NS_A), "obj-0007"),                           # third occurrence: new
             (rin(cm(0, ["l0"]), NS_A), "obj-0000")]                   # unchanged; obj-0008 is gone
    then = Cycle(eng, [r for r, _ in then_r], [k for _, k in then_r], process="audit")
    now = Cycle(eng, [r for r, _ in now_r], [k for _, k in now_r], process="audit")
    snap = then.table.snapshot()
    try:
        want = check_changes(then, now, snap, sizes=(64,))
        ids = {x: c.driver.constraint_id(deny(x)) for x in ("l0", "l1", "l2")}
        assert want == [(0, 5, [ids["l1"]], [], [ids["l0"]], [], 0),
                        (2, 4, [], [ids["l2"]], [], [], 0),
                        (3, 1, [], [], [], [ids["l2"]], 0),
                        (6, NONE, sorted([ids["l0"], ids["l1"]]), [], [], [], NEW),
                        (NONE, 7, [], [], [ids["l1"]], [], GONE)]
        rendered = [pg for pg in now.table.change_pages(snap, 64, render=True)]
        rows = [r for pg in rendered for r in pg["rows"]]
        viol = {r: x for r, _v, _e, x in now.table.violations(64, render=True)}
        assert rows == [viol[0], viol[2], None, viol[6], None]                 # byte for byte gk_table_violations' rendering; none without a result now
    finally:
        snap.free()
        then.free()
        now.free()


def psp_client(backend):
    fx = synth.load_fixtures()
    c, oc = load_both(backend, synth.psp_templates(fx), synth.audit_constraints())
    return c, oc


def big_pod(name, privileged, containers=256):
    """256 containers where predicates iterate elements: beyond the device's limits, answered by the host evaluator"""
    return {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": name, "namespace": "prod-1", "labels": {}},
            "spec": {"containers": [{"name": "c%d" % i, "image": "x", "securityContext": {"privileged": privileged and i == containers - 1}} for i in range(containers)]}}


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_a_review_the_host_evaluation_answered_on_either_side(backend):
    c, _ = psp_client(backend)
    eng = c.driver.engine
    nss = synth.gen_namespaces()
    base = synth.gen_objects(70, seed=5, mixed=True)

    def cycle(pod, host_eval=True):
        objs = list(base)
        objs[66] = pod
        # (both listings are `base` in one order, so equal keys -- should the generator repeat a name -- pair up by position)
        return Cycle(eng, [rin(o, synth.namespace_for(o, nss), "Original") for o in objs], ["pos-%d" % i for i in range(len(objs))], host_eval=host_eval)

    small, huge, huge2 = big_pod("huge-66", False, 2), big_pod("huge-66", True), big_pod("huge-66", False)
    made, snaps = [], []
    try:
        def pair(pod_then, pod_now, then_host=True, now_host=True):
            then = cycle(pod_then, then_host)
            made.append(then)
            snap = then.table.snapshot()
            snaps.append(snap)
            now = cycle(pod_now, now_host)
            made.append(now)
            want = expected(then, now)
            got = got_entries(now.table.change_pages(snap, 64))
            assert got == want
            check_apply(then, now, want)
            pg = next(iter(now.table.change_pages(snap, 64)))
            assert pg["beyond_limits"] == len(now.beyond) and pg["was_beyond_limits"] == len(then.beyond)
            return want, then, now

        want, then, now = pair(small, huge)                               # answered on the host now
        assert not now.beyond and [e[0] for e in want] == [66] and want[0][2] and want[0][2] != want[0][4]
        want, then, now = pair(huge, small)                               # ... then
        assert [e[0] for e in want] == [66] and want[0][4]
        want, then, now = pair(huge, huge2)                               # ... on both sides
        assert [e[0] for e in want] == [66] and want[0][2] != want[0][4] and want[0][4]
        want, then, now = pair(huge, huge)
        assert want == []
        want, then, now = pair(huge, huge2, now_host=False)               # beyond the limits now and unanswered: no entry, the consumer keeps what it holds
        assert want == [] and now.beyond == {66} and then.res[66] != EMPTY
        want, then, now = pair(huge2, huge, then_host=False)              # unanswered then: reads as zero then
        assert then.beyond == {66} and [e[0] for e in want] == [66] and not want[0][4] and not want[0][5] and want[0][6] == 0
    finally:
        for s in snaps:
            s.free()
        for cy in made:
            cy.free()


# ------------------------------------------------------------------------------------------------ 8. refusals
def raw(table, snap, cursor, max_entries=64, flags=0):
    """one raw gk_table_changes -> (status, error text, next cursor)"""
    eng = table.engine
    out = C.POINTER(L.gk_table_changes_out)()
    rc = eng.lib.gk_table_changes(eng.handle, table.handle, snap.handle if snap else None, None, cursor, max_entries, flags, C.byref(out))
    if rc != L.GK_OK:
        try:
            eng._check(rc)
        except D.EngineError as e:
            return rc, str(e), None
    nxt = int(out.contents.next_cursor)
    eng.lib.gk_table_changes_free(out)
    return rc, "", nxt


def raw_snapshot(table):
    eng = table.engine
    h = C.c_void_p()
    rc = eng.lib.gk_table_snapshot(eng.handle, table.handle, None, C.byref(h))
    if rc != L.GK_OK:
        try:
            eng._check(rc)
        except D.EngineError as e:
            return rc, str(e)
    eng.lib.gk_snapshot_free(h)
    return rc, ""


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_what_the_calls_refuse(backend):
    c = kinds_client(backend)
    eng = c.driver.engine
    rins = [rin(cm(i, ["l0"]), NS_A) for i in range(130)]
    table, bare, snap, other, other_snap, again = eng.create_table(rins), None, None, None, None, None
    try:
        for rc, err in (raw(table, None, 0)[:2], raw_snapshot(table)):
            assert rc == L.GK_ERR_INVALID and "evaluate the table first" in err                      # never evaluated
        assert raw(table, None, 0xDEADBEEF)[0] == L.GK_ERR_INVALID
        table.launch()
        for rc, err in (raw(table, None, 0)[:2], raw_snapshot(table)):
            assert rc == L.GK_ERR_INVALID and "still to be collected" in err                         # pending launches
        table.eval(collect_only=True)
        snap = table.snapshot()
        empty = eng.create_table([rin(cm(i, []), NS_A) for i in range(130, 260)])
        try:
            empty.eval()
            zero = empty.snapshot()                                                                  # a snapshot all of whose objects are gone now
        finally:
            empty.free()

        def page_one(then):
            rc, err, nxt = raw(table, then, 0)
            assert rc == L.GK_OK and nxt, err
            assert raw(table, then, nxt)[0] == L.GK_OK and raw(table, then, nxt)[0] == L.GK_OK        # while nothing moves the cursor works, again and again
            return nxt

        def refused(then, cursor):
            rc, err, _ = raw(table, then, cursor)
            assert rc == L.GK_ERR_INVALID and MOVED in err, (rc, err)

        saved = page_one(None)
        refused(None, 0xDEADBEEF), refused(None, saved ^ 1 << 63), refused(None, saved ^ 1 << 40), refused(None, saved + 1000)
        rc, err, _ = raw(table, zero, saved)                                                         # a later page with another `then`
        assert rc == L.GK_ERR_INVALID and "the snapshot the stream began with" in err
        assert raw(table, snap, 0) == (L.GK_OK, "", 0)                                               # against its own snapshot: nothing
        saved = page_one(zero)                                                                       # 130 new objects
        rc, err, _ = raw(table, None, saved)
        assert rc == L.GK_ERR_INVALID and "the snapshot the stream began with" in err
        table.eval()                                                                                 # a second evaluation
        refused(zero, saved)
        saved = page_one(zero)
        table.launch()                                                                               # launches alone move it as well
        table.eval(collect_only=True)
        refused(zero, saved)
        saved = page_one(zero)
        # a snapshot of another engine
        other = make_client(backend)
        other.AddTemplate(tmpl("K8sDenyLabel", DENY_LABEL))
        other.AddConstraint(deny("l0"))
        ot = other.driver.engine.create_table(rins[:3])
        try:
            ot.eval()
            other_snap = ot.snapshot()
        finally:
            ot.free()
        rc, err, _ = raw(table, other_snap, 0)
        assert rc == L.GK_ERR_INVALID and "another engine" in err
        # rendering needs the documents
        bare = eng.create_table(rins[:3], keep_docs=False)
        bare.eval()
        assert raw(bare, None, 0)[0] == L.GK_OK
        rc, err, _ = raw(bare, None, 0, flags=L.GK_CHANGES_RENDER)
        assert rc == L.GK_ERR_INVALID and "GK_TABLE_KEEP_DOCS" in err
        if backend == "hostemu":   # a table set up as a shard: its bitmaps live in the exchange buffer (a communicator of one rank, CPU stand-in)
            gather, reduce_ = L.HE_ALLGATHER(lambda ctx, buf, n: None), L.HE_ALLREDUCE(lambda ctx, buf, n: None)
            assert eng.lib.gk_comm_init_host(eng.handle, 0, 1, gather, reduce_, None) == 0
            shard = eng.create_table(rins[:70])
            try:
                so = C.POINTER(L.gk_shard_out)()
                assert eng.lib.gk_table_sweep_sharded(eng.handle, shard.handle, 0, C.byref(so)) == 0
                eng.lib.gk_shard_free(so)
                rc, err, _ = raw(shard, None, 0)
                assert rc == L.GK_ERR_INVALID and "set up as a shard" in err
                rc, err, _ = raw(shard, snap, 0)
                assert rc == L.GK_ERR_INVALID and "set up as a shard" in err
                rc, err = raw_snapshot(shard)
                assert rc == L.GK_ERR_INVALID and "set up as a shard" in err
            finally:
                shard.free()
                eng.lib.gk_comm_destroy(eng.handle)
        c.AddConstraint(deny("l9"))                                                                  # the policies change
        refused(zero, saved)
        for rc, err in (raw(table, zero, 0)[:2], raw_snapshot(table)):
            assert rc == L.GK_ERR_INVALID and "create it again" in err                               # a new label value: the table itself is stale
        again = eng.create_table(rins)
        assert again.eval().n_constraints == 4
        assert raw(again, snap, 0)[0] == L.GK_OK                                                     # the snapshot survives the policy change
        c.RemoveConstraint(deny("l9"))                                                               # a policy change that leaves the table's rows valid
        for rc, err in (raw(again, snap, 0)[:2], raw_snapshot(again)):
            assert rc == L.GK_ERR_INVALID and "evaluate it again" in err
        assert again.eval().n_constraints == 3 and raw(again, snap, 0) == (L.GK_OK, "", 0)
        zero.free()
    finally:
        for x in (table, bare, again):
            if x:
                x.free()
        for s in (snap, other_snap):
            if s:
                s.free()


# ------------------------------------------------------------------------------------------------ 9. the audit, cycle after cycle
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_audit_cycles_mirror_the_audit_stream_and_the_oracles_loop(backend):
    c, oc = psp_client(backend)
    nss = synth.gen_namespaces()
    objs = synth.gen_objects(120, seed=5, mixed=True)
    objs[7] = big_pod("huge-7", True)
    excl = [{"excludedNamespaces": [objs[30]["metadata"].get("namespace") or objs[31]["metadata"]["namespace"]], "processes": ["audit"]}]
    c.SetExcluder(excl)
    ox = OX.Excluder(excl)

    def key_of(o):
        g, ver, kind = D.obj_gvk(o)
        return (g, ver, kind, o["metadata"].get("namespace", "") or "", o["metadata"]["name"])

    def listing(objs, rejected):
        rv = [D.AugmentedUnstructured(D.Unstructured(o), synth.namespace_for(o, nss), "Original") for o in objs]
        if rejected is not None:
            rv[rejected] = delete_without_old_object()
        return rv

    def result_key(r):
        return (r.constraint["metadata"]["name"], r.msg, r.enforcement_action)

    cycles = c.AuditCycles(page=64)
    mirror = {}

    def run(objs, rejected, removed=()):
        rv = listing(objs, rejected)
        failures = {}
        for key, *rest in cycles.run(rv):
            if isinstance(rest[0], D.ReviewFailure):
                failures[key] = rest[0]
                continue
            appeared, resolved, flags = rest
            if appeared and not flags & GONE:
                mirror[key] = sorted(result_key(r) for r in appeared)
            else:
                mirror.pop(key, None)
        for k in list(mirror):                                                # the consumer drops what it holds of constraints that are gone
            mirror[k] = [x for x in mirror[k] if x[0] not in removed]
            if not mirror[k]:
                del mirror[k]
        stream = {}
        for i, res in c.AuditStream(rv, page=64):
            if isinstance(res, D.ReviewFailure):
                assert isinstance(failures.get(i), D.ReviewFailure) and str(failures[i]) == str(res)
            else:
                stream[key_of(objs[i])] = sorted(result_key(r) for r in res)
        assert mirror == stream and (rejected is None) == (not failures)
        n = 0
        for i, o in enumerate(objs):                                          # the oracle client's serial loop (manager.go:667-776)
            if i == rejected or ox.is_namespace_excluded("audit", o):
                assert i == rejected or key_of(o) not in mirror
                continue
            want = sorted(result_key(r) for r in oc.review(to_oracle_review(rv[i]), OC.AUDIT_EP))
            assert mirror.get(key_of(o), []) == want, i
            n += len(want)
        return n

    try:
        assert run(objs, 20) > 50 and cycles.snapshot is not None
        second = [o for i, o in enumerate(reversed(objs)) if i % 9]            # another order, objects gone ...
        second += synth.gen_objects(15, seed=11, mixed=True)[10:]              # ... and new ones
        assert run(second, None) > 40
        kept = cycles.snapshot
        it = cycles.run(listing(objs, None))
        next(it)
        it.close()                                                            # an abandoned run leaves the previous snapshot in place
        assert cycles.snapshot is kept and kept.handle
        victim = synth.audit_constraints()[0]
        c.RemoveConstraint(victim)
        oc.remove_constraint(victim)
        assert run(objs, None, removed=(victim["metadata"]["name"],)) > 30
    finally:
        cycles.close()
    assert cycles.snapshot is None
