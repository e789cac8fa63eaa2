"""Row a11, the list-based audit: gk_table_topk (Table.topk) at the edges of its device kernel.  gk_topk_rows walks a bitmap row 64
key-order positions per step, one wave per row: ballots, a lane shuffle for the k-th key's rank, state carried from step to step, a stop
ballot and a per-lane cap guard.  Here: the k-th at the last lane of a step and at the first lane of the next, key ties that run over one
and over two step boundaries and up to the table's end in a partial last step, rows with fewer than k violators and with none, lists
exactly `cap` long and one over, and the callers' bitmap-walk fallback (Client.AuditAggregate, ShardedSweep.audit_lists) that an
overflowing list sets off.

Expected answers: tests/topk_ref.py -- plain Python over the bitmaps a downloading Table.eval() returns and the objects' keys, nothing of
the selection code; where the construction says what must violate, that as well.  The callers are compared with the oracle client's
reviews fed to oracle.audit.add_audit_responses / LimitQueue, as tests/test_parity.py::test_audit_aggregation does.

Policy: the label template of tests/test_resident_audit.py, one constraint (= one bitmap row) per violation pattern.  Objects: ConfigMaps
in namespace `default`; equal keys are equal metadata.name (the duplicates differ in a `data` member).  Patterns are sets of POSITIONS in
key order; the slot order -- the review index, which decides the order inside a tie -- is varied separately (reversed, shuffled), so that
order[] is a real gather.

Host-evaluated pairs, which gk_table_topk appends behind the device's lists, are not produced here (test_parity covers their effect).

This is where the device's tie and overflow branches of gk_topk_rows are tested: the table path is the only one on which keys can tie.
gk_audit_select restates the rule for the resident set, whose keys are unique: its copies of these branches stay unreachable through the
product (tests/test_audit_merge.py drives their CPU stand-in, tests/test_resident_audit.py the kernels without ties)."""
import contextlib

import pytest

import topk_ref as TR
from gatekeeper_amd import _lib as L
from gatekeeper_amd import driver as D
from gatekeeper_amd import sweep as S
from gatekeeper_amd import synth
from oracle import audit as OA
from parity_util import load_both, plan_group_max
from test_parity import _random_match_world as random_match_world   # (the neighbours' helpers, as they are)
from test_resident_audit import NEED_LABEL, STAMP, ckey, label_sig, labelled, need_label, serial_loop, shuffled, tmpl
from test_table_violations import TABLE_BACKENDS

STEP = 64   # positions one step of gk_topk_rows covers

# ---- layout T: singles 0-59 | 70 equal keys 60-129 (over the 63/64 and 127/128 boundaries) | singles 130-169 | 66 equal keys 170-235,
# up to the end of the table, 236 % 64 == 44
N_T, TIE_A, TIE_B = 236, range(60, 130), range(170, 236)
ROWS_T = {"all": set(range(N_T)), "none": set(), "tie70": set(TIE_A), "k-at-63": set(range(59, 66)), "tail66": set(TIE_B),
          "tail66-and-first": {0} | set(TIE_B), "odd": set(range(1, N_T, 2))}
KS_T = (1, 2, 5, 6, 20, 61, 64, 65, 70, N_T + 5)
# worked out by hand from the layout and the rule, cap = k + 64: the lists longer than cap ...
OVERFLOWING_T = {("all", 61), ("all", 64), ("all", 65), ("tie70", 1), ("tie70", 2), ("tie70", 5), ("tail66", 1), ("tail66-and-first", 2)}
EXACTLY_FULL_T = {("tie70", 6), ("tail66", 2)}   # ... and the ones exactly cap long


def name_t(p):
    """metadata.name of the object at key position p of layout T"""
    return "obj-%03d" % (TIE_A[0] if p in TIE_A else TIE_B[0] if p in TIE_B else p)


def rows_small(n):
    return {"all": set(range(n)), "none": set(), "first": {0}, "last": {n - 1}, "p63-p64": {p for p in (63, 64) if p < n}}


def slot_orders(n, ties=()):
    """{id: key position of every slot}.  Equal keys stay in slot order (a stable sort), so inside each range of `ties` the positions
    ascend with the slots the range got: a position below is the place in the walk, also inside a tie."""
    orders = {"reversed": list(reversed(range(n))), "shuffled": shuffled(range(n), 11)}
    for positions in orders.values():
        for tie in ties:
            for s, p in zip(sorted(s for s, p in enumerate(positions) if p in tie), tie):
                positions[s] = p
    return orders


def objects(rows, positions, name_of):
    """the ConfigMaps in slot order: slot s holds the object at key position positions[s]"""
    objs = []
    for p in positions:
        o = labelled(name_of(p), "default", {x for x, pos in rows.items() if p in pos}, list(rows))
        o["data"] = {"position": str(p)}
        objs.append(o)
    return objs


def clients(backend, rows):
    return load_both(backend, [tmpl("K8sNeedLabel", NEED_LABEL)], [need_label(x) for x in rows])


def rin(o):
    return D.to_review_in(D.AugmentedUnstructured(D.Unstructured(o), None, ""))


class Evaluated:
    """a table of `objs`, evaluated; the reference's view of it: the keys, per row name the violators' bits by slot"""

    def __init__(self, c, rows, positions, objs, resident):
        self.table = c.driver.engine.create_table([rin(o) for o in objs], resident=resident)
        self.ev = ev = self.table.eval()
        assert ev.n_reviews == len(objs) and ev.n_constraints == len(rows) and not ev.too_big_reviews() and not ev.host_evaluated
        self.keys = [TR.object_key(o) for o in objs]
        assert [positions[r] for r in sorted(range(len(objs)), key=self.keys.__getitem__)] == list(range(len(objs)))   # positions: the walk's
        self.cid = {x: c.driver.constraint_id(need_label(x)) for x in rows}
        row_of = {int(cid): i for i, cid in enumerate(ev.constraint_ids)}
        bits = TR.violators(ev)
        self.bits = {x: bits[row_of[self.cid[x]]] for x in rows}
        # the reference's view of the bitmaps is what the construction says: a wrong bitmap is not top-k's fault
        for x, pos in rows.items():
            assert [bool(b) for b in self.bits[x]] == [p in pos for p in positions], x

    def check(self, k, cap):
        """Table.topk(k) == the reference, exactly and in order, flag included, for every row -> {row name: (reviews, overflow)}"""
        got = self.table.topk(k)
        assert sorted(got) == sorted(self.cid.values())
        want = {x: TR.expected(self.bits[x], self.keys, k, cap) for x in self.cid}
        for x in self.cid:
            assert got[self.cid[x]] == want[x], (x, k)
        return want

    def steps_of_the_tie(self, x, k, positions):
        """how many steps of the walk hold the k-th violator of row x and the further ones that tie with it (0: none tie)"""
        walked = TR.walk(self.bits[x], self.keys, k)
        return len({positions[r] // STEP for r in walked[k - 1:]}) if len(walked) > k else 0


# ------------------------------------------------------------------------------------------------ 1. layout T
@pytest.mark.parametrize("resident", [False, True], ids=["plain", "resident"])
@pytest.mark.parametrize("order", ["reversed", "shuffled"])
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_step_edges_ties_and_overflow(backend, order, resident):
    positions = slot_orders(N_T, (TIE_A, TIE_B))[order]
    c, _ = clients(backend, ROWS_T)
    t = Evaluated(c, ROWS_T, positions, objects(ROWS_T, positions, name_t), resident)
    try:
        assert t.ev.n_plan_groups == 1
        overflowing, full, tie_steps = set(), set(), {}
        for k in KS_T:
            cap = TR.stride(t.table, k)
            assert cap == k + 64          # the product's capacity (engine.cpp), read from the product
            for x, (reviews, overflow) in t.check(k, cap).items():
                assert len(reviews) <= cap and (not overflow or len(reviews) == cap)
                if overflow:
                    overflowing.add((x, k))
                elif len(reviews) == cap:
                    full.add((x, k))
                tie_steps[x, k] = t.steps_of_the_tie(x, k, positions)
        # the reference itself reaches the branches this test is about: lists over cap and exactly cap long; ties that end in the k-th's
        # own step, in the next one and two steps on; the k-th at lane 63 and at lane 0
        assert overflowing == OVERFLOWING_T and full == EXACTLY_FULL_T
        assert tie_steps["k-at-63", 6] == 1 and tie_steps["k-at-63", 5] == 2 and tie_steps["tail66", 2] == 2 and tie_steps["all", 70] == 2
        assert tie_steps["tie70", 1] == 3 and tie_steps["all", 64] == 3 and tie_steps["all", 65] == 2 and tie_steps["all", 1] == 0
        assert sum(1 for v in tie_steps.values() if v >= 2) >= 20
        want = t.check(1, 65)
        assert want["all"] == ([positions.index(0)], False) and want["none"] == ([], False)
        # ties come out in review-index order, whatever the slot order
        assert want["tail66"][0] == sorted(s for s, p in enumerate(positions) if p in TIE_B)[:65] and want["tail66"][1]
    finally:
        t.table.free()


# ------------------------------------------------------------------------------------------------ 2. small tables
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_small_tables_of_distinct_keys(backend, n):
    rows = rows_small(n)
    c, _ = clients(backend, rows)
    for order, positions in slot_orders(n).items():
        objs = objects(rows, positions, lambda p: "obj-%03d" % p)
        for resident in (False, True):
            t = Evaluated(c, rows, positions, objs, resident)
            try:
                for k in (1, 20, n + 5):
                    want = t.check(k, k + 64)
                    for x, pos in rows.items():   # distinct keys: the k smallest positions, ascending, never a flag
                        assert want[x] == ([positions.index(p) for p in sorted(pos)[:k]], False), (order, resident, x, k)
            finally:
                t.table.free()


# ------------------------------------------------------------------------------------------------ 3. plan groups, many rows
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_three_plan_groups_answer_like_one(backend):
    """seven rows in groups of 3 / 3 / 1: a launch per group, the groups' lists appended"""
    positions = slot_orders(N_T, (TIE_A, TIE_B))["shuffled"]
    objs = objects(ROWS_T, positions, name_t)
    answers = []
    lib = L.load(hostemu=backend.startswith("hostemu"))
    for group_max, groups in ((None, 1), (3, 3)):
        with (plan_group_max(lib, group_max) if group_max else contextlib.nullcontext()):
            c, _ = clients(backend, ROWS_T)
            t = Evaluated(c, ROWS_T, positions, objs, True)
            try:
                assert t.ev.n_plan_groups == groups
                answers.append({k: t.check(k, k + 64) for k in KS_T})
            finally:
                t.table.free()
    assert answers[0] == answers[1] and {(x, k) for k in KS_T for x in ROWS_T if answers[1][k][x][1]} == OVERFLOWING_T


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_random_objects_that_share_names_under_180_constraints(backend, fixtures):
    """the table of tests/test_parity.py::test_many_constraints_split_into_plan_groups -- 150 random match blocks and the PSP constraints
    over 130 random objects of five names, seven namespaces and five kinds, so keys tie by chance; that test asserts of Table.topk(5)
    no more than "at least min(5, count) entries, all of them violators".  Here: exactly the reference's list and flag for every row."""
    tmpl_ = fixtures["go_consts"]["pkg/target/target_integration_test.go"]["testTemplate"]["docs"][0]
    cons, reviews = random_match_world(77, 150, 130)
    c, _ = load_both(backend, [tmpl_] + synth.psp_templates(fixtures), cons + synth.psp_constraints(), validate=False)
    revs = [r for r, _ in reviews]
    table = c.driver.engine.create_table([D.to_review_in(r) for r in revs], keep_docs=False)
    try:
        ev = table.eval()
        assert ev.n_constraints == len(cons) + 30 and not ev.host_evaluated and not ev.too_big_reviews()
        keys, bits, cap = [TR.object_key(D.review_object(r)) for r in revs], TR.violators(ev), TR.stride(table, 5)
        top = table.topk(5)
        assert len(top) == ev.n_constraints and len(set(keys)) < len(keys)
        for i, cid in enumerate(ev.constraint_ids):
            assert top[int(cid)] == TR.expected(bits[i], keys, 5, cap), i
        assert any(len(got) > 5 for got, _ in top.values())   # ties on the fifth key occur
    finally:
        table.free()


# ------------------------------------------------------------------------------------------------ 4. edge calls
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_edge_calls(backend):
    positions = slot_orders(N_T, (TIE_A, TIE_B))["reversed"]
    c, _ = clients(backend, ROWS_T)
    objs = objects(ROWS_T, positions, name_t)
    bare = c.driver.engine.create_table([rin(o) for o in objs[:70]])
    try:
        with pytest.raises(D.EngineError, match="evaluate the table first"):   # never evaluated
            bare.topk(5)
    finally:
        bare.free()
    t = Evaluated(c, ROWS_T, positions, objs, False)
    try:
        assert t.table.topk(0) == {cid: ([], False) for cid in t.cid.values()} and TR.stride(t.table, 0) == 64   # k == 0: nothing, no flag
        totals = t.table.totals()
        for x, pos in ROWS_T.items():   # pairs: the row's popcount; one message per pair for this template
            assert totals[t.cid[x]] == (len(pos), len(pos)) and int(t.bits[x].sum()) == len(pos), x
    finally:
        t.table.free()


# ------------------------------------------------------------------------------------------------ 5. the callers' fallback
def oracle_lists(want, limit):
    lists, totals, per_action = {}, {}, {}
    OA.add_audit_responses(lists, totals, per_action, want[0], limit=limit)
    return lists, totals, per_action


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_callers_walk_the_bitmap_row_where_a_list_overflows(backend):
    """Client.AuditAggregate and ShardedSweep.audit_lists against the oracle fed with EVERY result.  Limit 1: `tie70` and `tail66`
    overflow (66 and 70 equal keys against cap = 65), limit 2: `tie70` and `tail66-and-first` -- the callers walk those rows' bitmaps;
    limit 20: no list overflows.  (`all` does not overflow at limit 1: its smallest key is a single one.)"""
    positions = slot_orders(N_T, (TIE_A, TIE_B))["shuffled"]
    c, oc = clients(backend, ROWS_T)
    objs = objects(ROWS_T, positions, name_t)
    # one oracle review per distinct label set: the template reads nothing but the labels
    want = serial_loop(oc, dict(enumerate(objs)), memo={}, sig=label_sig)
    assert {k[2]: v for k, v in want[1].items()} == {x: len(pos) for x, pos in ROWS_T.items() if pos}
    reviews = [D.AugmentedUnstructured(D.Unstructured(o), None, "") for o in objs]
    t = Evaluated(c, ROWS_T, positions, objs, True)   # the table AuditAggregate builds
    try:
        flagged = {limit: {x for x, cid in t.cid.items() if t.table.topk(limit)[cid][1]} for limit in (1, 2, 20)}
    finally:
        t.table.free()
    assert flagged == {1: {"tie70", "tail66"}, 2: {"tie70", "tail66-and-first"}, 20: set()}
    shard = S.ShardedSweep(c, objs, {}, keep_docs=True)
    try:
        for limit in (1, 2, 20):
            lists, totals, per_action = oracle_lists(want, limit)
            got = c.AuditAggregate(reviews, limit=limit)
            assert {k: v["total_pairs"] for k, v in got.items() if v["total_pairs"]} == want[1]
            assert {k: v["total"] for k, v in got.items() if v["total"]} == totals
            assert got.totals_per_action == per_action and not got.errors
            assert set(got) == {ckey(k) for k in c.constraints.values()} and len(lists) == len(ROWS_T) - 1
            for k, v in got.items():
                q = lists.get(k) or OA.LimitQueue(limit)
                assert v["violations"] == q.sorted() and len(v["violations"]) == min(limit, len(ROWS_T[k[2]])), (k, limit)
                st = got.constraint_status(k, STAMP, violations_limit=limit)
                assert st == OA.constraint_status(q, totals.get(k, 0), STAMP, violations_limit=limit), (k, limit)
            assert shard.audit_lists(limit) == {k: (lists[k].sorted() if k in lists else []) for k in got}, limit
    finally:
        shard.table.free()
