"""Rows a11 + f2: gk_resident_changes -- what differs in gk_resident_violations' answer since the last changes stream that was read to
its end.  The device compares the sweep's bitmaps with a copy kept at the baseline (gk_delta_index + gk_delta_emit); autoreject pairs
and host-completed pairs are compared on the host.

The yardstick is independent of the code under test: S(state) = {path: (violated constraints, autoreject constraints)} comes from the
oracle client's serial loop over the cached objects (serial_loop + expected_sets of tests/test_resident_violations.py, memoised by
signature), before and after every step.  A second leg takes S from the product's own complete gk_resident_violations stream.  The
entries, folded per path in stream order (OR of was, OR of now), must equal the difference of the two maps.  The CPU stand-in's loops
and the host-side diff of sparse pairs are covered on their own by tests/test_delta_stream_native.py."""
import contextlib
import json

import pytest

from gatekeeper_amd import _lib as L
from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from oracle import excluder as OX
from parity_util import load_both, plan_group_max
import test_resident_violations as RV

RESIDENT_BACKENDS = RV.RESIDENT_BACKENDS
C = L.C
PAGES = (64, 100, 1000000)
NONE = (frozenset(), frozenset())


def call(c, cursor, max_objects, flags=L.GK_CHANGES_RENDER):
    """one raw gk_resident_changes -> (status, error text, page dict or None); an entry is (path, viol, err, was_viol, was_err, gone, text)"""
    eng = c.driver.engine
    out = C.POINTER(L.gk_changes_out)()
    rc = eng.lib.gk_resident_changes(eng.handle, cursor, max_objects, flags, C.byref(out))
    if rc != L.GK_OK:
        try:
            eng._check(rc)
        except D.EngineError as e:
            return rc, str(e), None
    o = out.contents
    ids, mw = [int(o.constraint_ids[i]) for i in range(o.n_constraints)], int(o.mask_words)
    assert mw == (len(ids) + 63) // 64

    def bits(arr, i):
        m = 0
        for w in range(mw):
            m |= int(arr[i * mw + w]) << (64 * w)
        assert m >> len(ids) == 0
        return frozenset(ids[r] for r in range(len(ids)) if (m >> r) & 1)

    render = bool(flags & L.GK_CHANGES_RENDER)
    assert render or not o.results_json
    page = {"reset": int(o.reset), "total": int(o.total_entries), "next": int(o.next_cursor), "beyond": int(o.beyond_limits), "n_objects": int(o.n_objects),
            "n_chunks": int(o.n_chunks), "ids": ids, "device_ms": float(o.device_ms), "baseline_bytes": int(o.baseline_bytes),
            "entries": [(tuple(json.loads(o.paths[i].decode())), bits(o.viol, i), bits(o.err, i), bits(o.was_viol, i), bits(o.was_err, i),
                         bool(o.entry_flags[i] & L.GK_CHANGE_GONE), o.results_json[i] if render and o.results_json else None) for i in range(o.n_entries)]}
    eng.lib.gk_changes_free(out)
    return rc, "", page


def stream(c, max_objects, flags=L.GK_CHANGES_RENDER):
    """the whole stream from cursor 0 -> [page dict]; reading it to the end advances the baseline"""
    pages, cursor = [], 0
    while True:
        rc, err, page = call(c, cursor, max_objects, flags)
        assert rc == L.GK_OK, err
        pages.append(page)
        cursor, flags = page["next"], flags & ~L.GK_CHANGES_RESTART
        if not cursor:
            return pages
        assert len(pages) < 100000


def product_sets(c):
    """S(state) as the product's own complete gk_resident_violations stream says it, in constraint ids"""
    return {e[0]: (frozenset(e[1]), frozenset(e[2])) for p in RV.stream(c, 1000000, 0) for e in p["entries"]}


class World:
    """a product client and the oracle side by side, the slot order the resident set must have (every sweep flattens what was put since
    the last one, in put order, into a new chunk), and S at the baseline as both legs see it"""

    def __init__(self, c, oc, size, memo=None, sig=None, track=True):
        self.c, self.oc, self.size, self.memo, self.sig = c, oc, size, memo, sig
        self.hidden = None
        self.pending, self.chunks, self.track = [], [], track
        self.base_oracle, self.base_product = {}, {}
        self.touched = set()

    # ---- the set
    def _queue(self, path):
        if path not in self.pending:
            self.pending.append(path)
        self.touched.add(path)

    def _dependants(self, path):
        if path[:3] == ("cluster", "v1", "Namespace"):
            for p in self.c.cached:
                if len(p) == 5 and p[0] == "namespace" and p[1] == path[3]:
                    self._queue(p)

    def put(self, o):
        path = tuple(D.process_data(o))
        if self.c.cached.get(path) != o:
            self._queue(path)
            self._dependants(path)
        self.c.AddData(o), self.oc.add_data(o)

    def remove(self, o):
        path = tuple(D.process_data(o))
        if path in self.pending:
            self.pending.remove(path)
        self.touched.add(path)
        self.c.RemoveData(o), self.oc.remove_data(o)
        self._dependants(path)

    def swept(self):
        """call before anything that brings the set up to date"""
        live = [p for p in self.pending if p in self.c.cached]
        if live:
            self.chunks.append(live)
        self.pending = []

    # ---- the yardsticks
    def oracle_sets(self):
        want = RV.serial_loop(self.oc, self.c.cached, hidden=self.hidden, memo=self.memo, sig=self.sig)
        return {p: (frozenset(v), frozenset(e)) for p, (v, e) in RV.expected_sets(want).items()}

    def key_of(self):
        return {self.c.driver.constraint_id(k): RV.ckey(k) for k in self.c.constraints.values()}

    def check_pages(self, pages, reset):
        entries = [e for p in pages for e in p["entries"]]
        for p in pages:
            assert p["reset"] == int(reset) and p["total"] == len(entries) and p["ids"] == pages[0]["ids"] and p["n_objects"] == len(self.c.cached)
            assert len(p["entries"]) <= max(self.size, 64) and (p["entries"] or len(pages) == 1)
            if self.track:   # ascending slot order of ONE chunk
                paths = [e[0] for e in p["entries"]]
                assert any(all(x in pos for x in paths) and [pos[x] for x in paths] == sorted(pos[x] for x in paths) and len(set(paths)) == len(paths)
                           for pos in ({x: i for i, x in enumerate(ch)} for ch in self.chunks)) or not paths, paths
        for path, viol, err, was_viol, was_err, gone, _ in entries:
            assert (viol, err) != (was_viol, was_err) or (viol | err and path in self.touched), path   # a slot has an entry iff now != was (or it was flattened again)
            assert not gone or not (viol | err), path
        return entries

    @staticmethod
    def fold(entries, name=lambda i: i):
        out = {}
        for path, viol, err, was_viol, was_err, _, _ in entries:
            f = out.setdefault(path, [set(), set(), set(), set()])
            for k, ids in enumerate((was_viol, was_err, viol, err)):
                f[k] |= {name(i) for i in ids}
        return {p: ((frozenset(f[0]), frozenset(f[1])), (frozenset(f[2]), frozenset(f[3]))) for p, f in out.items()}

    def check_difference(self, entries, before, after, name=lambda i: i):
        folded = self.fold(entries, name)
        for path in set(before) | set(after):
            if before.get(path, NONE) != after.get(path, NONE):
                assert path in folded, ("missing", path)
        for path, (was, now) in folded.items():
            assert (was, now) == (before.get(path, NONE), after.get(path, NONE)), path
            assert was != now or (now != NONE and path in self.touched), ("unchanged", path)

    def changes(self, reset=False, flags=L.GK_CHANGES_RENDER):
        """one complete changes stream, checked against both legs; -> its entries"""
        after_oracle = self.oracle_sets()
        self.swept()
        after_product = product_sets(self.c)                                      # (a complete violation stream in between alters nothing)
        pages = stream(self.c, self.size, flags)
        if reset is None:                                                         # (the caller looks at last_reset)
            reset = bool(pages[0]["reset"])
        self.last_reset, self.last_pages = reset, pages
        entries = self.check_pages(pages, reset)
        key_of = self.key_of()
        self.check_difference(entries, {} if reset else self.base_oracle, after_oracle, lambda i: key_of[i])
        self.check_difference(entries, {} if reset else self.base_product, after_product)
        for path, viol, err, _, _, gone, text in entries:                         # rendered: gk_resident_review's bytes where there is a result now
            if flags & L.GK_CHANGES_RENDER:
                assert (text == RV.review_bytes(self.c, path)) if viol | err else text is None, path
        self.base_oracle, self.base_product, self.touched = after_oracle, after_product, set()
        return entries


def psp_world(backend, fixtures, size):
    """100 pods, 30 of the namespaces they live in: 130 objects, three bitmap words, the last with two slots; the pods of the other
    namespaces have autoreject results under the namespaceSelector constraints"""
    c, oc = load_both(backend, synth.psp_templates(fixtures), synth.audit_constraints())
    w = World(c, oc, size, memo=RV.PSP_MEMO, sig=RV.text_sig)
    pods, nss = synth.gen_objects(100, seed=23), synth.gen_namespaces()
    used = []
    for o in pods:
        if o["metadata"]["namespace"] not in used:
            used.append(o["metadata"]["namespace"])
    assert len(used) > 40
    for o in RV.shuffled([nss[n] for n in used[:30]] + pods, 7):
        w.put(o)
    return w, pods, nss, used


def copy_of(o):
    return json.loads(json.dumps(o))


def run_psp_scenario(backend, fixtures, size):
    """steps 1-9 of the issue's list at one page size; -> per step the entries without the rendered text"""
    w, pods, nss, used = psp_world(backend, fixtures, size)
    c = w.c
    log = []

    def step(**kw):
        log.append([e[:6] for e in w.changes(**kw)])
        return log[-1]

    # 1. the first stream: the whole state, was = 0
    first = step(reset=True)
    assert len(first) > 64 and all(not e[3] and not e[4] and not e[5] for e in first)
    assert [(e[0], e[1], e[2]) for e in first] == [(e[0], frozenset(e[1]), frozenset(e[2])) for p in RV.stream(c, 1000000, 0) for e in p["entries"]]
    assert sum(1 for e in first if e[2]) > 5                                     # autoreject results among them
    # 2. nothing changed
    assert step() == []
    # 3. puts and removes
    S = w.base_oracle
    path_of = lambda o: tuple(D.process_data(o))   # noqa: E731
    bad = [o for o in pods if S.get(path_of(o), NONE)[0]]
    synced = [o for o in bad if o["metadata"]["namespace"] in used[:30] and not S[path_of(o)][1]]   # (violating, and no autoreject result whatever the spec)
    assert len(synced) > 8
    new_bad = copy_of(synced[0]); new_bad["metadata"]["name"] = "zz-new-bad"
    new_clean = {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "zz-new-clean", "namespace": synced[0]["metadata"]["namespace"]}, "spec": {"containers": []}}
    to_clean = copy_of(synced[1]); to_clean["spec"] = {"containers": []}; to_clean["metadata"].pop("labels", None)
    clean_then_bad = copy_of(new_bad); clean_then_bad["metadata"]["name"] = "zz-flip"
    other = copy_of(synced[2]); other["spec"]["hostNetwork"] = not other["spec"].get("hostNetwork", False); other["spec"]["hostPID"] = not other["spec"].get("hostPID", False)
    same = copy_of(synced[3]); same["metadata"].setdefault("annotations", {})["note"] = "changed text, same answers"
    flip0 = copy_of(new_clean); flip0["metadata"]["name"] = "zz-flip"
    w.put(flip0)
    step()
    assert path_of(flip0) not in w.base_oracle and path_of(new_clean) not in w.base_oracle
    for o in (new_bad, new_clean, to_clean, clean_then_bad, other, same):
        w.put(o)
    w.remove(synced[4])
    got = step()
    by_path = {}
    for e in got:
        by_path.setdefault(e[0], []).append(e)
    assert len(by_path[path_of(new_bad)]) == 1 and not by_path[path_of(new_bad)][0][3] and path_of(new_clean) not in by_path
    assert [e[5] for e in by_path[path_of(to_clean)]] == [True]                   # violating -> clean: one entry, GONE
    assert [e[5] for e in by_path[path_of(clean_then_bad)]] == [False]            # clean -> violating
    assert [e[5] for e in by_path[path_of(other)]] == [True, False] and by_path[path_of(other)][0][3] != by_path[path_of(other)][1][1]   # old first, other masks
    assert [e[5] for e in by_path[path_of(same)]] == [True, False] and by_path[path_of(same)][0][3] == by_path[path_of(same)][1][1]     # equal masks: appears
    assert [e[5] for e in by_path[path_of(synced[4])]] == [True]                  # removed
    w.remove(new_clean)                                                          # removing a clean object: nothing to say
    assert step() == []
    # 4. a Namespace's labels change: the namespaceSelector constraints flip for the objects living in it
    prod = next(n for n in used[:30] if n.startswith("prod") and any(o["metadata"]["namespace"] == n for o in bad))
    ns2 = copy_of(nss[prod]); ns2["metadata"]["labels"]["env"] = "dev"; ns2["metadata"]["labels"].pop("pci", None)
    w.put(ns2)
    got = step()
    assert any(e[0][1] == prod and e[5] for e in got if e[0][0] == "namespace") and any(e[0][1] == prod and not e[5] for e in got if e[0][0] == "namespace")
    # 5. autoreject: a Namespace that was not synced arrives
    late = next(n for n in used[30:] if any(S.get(path_of(o), NONE)[1] for o in pods if o["metadata"]["namespace"] == n))
    w.put(nss[late])
    got = step()
    olds = [e for e in got if e[0][0] == "namespace" and e[0][1] == late and e[5]]
    assert olds and all(e[4] and not e[2] for e in olds)                         # was_err set, err clear
    assert not any(e[2] for e in got if e[0][0] == "namespace" and e[0][1] == late)
    # 6. a process excluder, set and cleared
    hide = prod
    ex = [{"excludedNamespaces": [hide], "processes": ["audit"]}]
    c.SetExcluder(ex)
    ox = OX.Excluder(ex)
    w.hidden = lambda o: ox.is_namespace_excluded("audit", o)   # noqa: E731
    got = step()
    assert got and all(e[5] and e[0][1] == hide for e in got)
    c.SetExcluder([])
    w.hidden = None
    got = step()
    assert got and all(not e[5] and not e[3] and not e[4] and e[0][1] == hide for e in got)
    # 8. abandoned and refused streams
    for k, o in enumerate(bad[10:90]):
        o2 = copy_of(o); o2["spec"]["hostIPC"] = not o2["spec"].get("hostIPC", False)
        w.put(o2)
    w.swept()
    rc, err, page1 = call(c, 0, 64)
    assert rc == L.GK_OK and page1["next"] and not page1["reset"], err
    rc, err, again = call(c, 0, 64)                                              # page 1, then cursor 0 again: the same entries
    assert rc == L.GK_OK and again["entries"] == page1["entries"] and again["total"] == page1["total"]
    extra = copy_of(synced[5]); extra["spec"]["hostNetwork"] = not extra["spec"].get("hostNetwork", False)
    w.put(extra)                                                                 # a put between two pages
    rc, err, page = call(c, again["next"], 64)
    assert rc == L.GK_ERR_INVALID and RV.MOVED in err and page is None
    w.swept()
    assert c.driver.ResidentSweep()["n_objects"] == len(c.cached) and c.driver.ResidentAudit(3)["n_objects"] == len(c.cached)
    got = step()                                                                 # the old entries and the new one
    assert [e for e in got if e[0] == path_of(extra)] and {e[0] for e in page1["entries"]} <= {e[0] for e in got}
    assert step() == []
    # 9. policies: a constraint goes, one comes, an explicit restart
    k_ = synth.audit_constraints()[0]
    c.RemoveConstraint(k_), w.oc.remove_constraint(k_)
    w.memo = {}
    got = step(reset=True)
    assert got and len(w.c.driver.ResidentAudit(0)["pairs"]) == len(synth.audit_constraints()) - 1
    assert step() == []
    c.AddConstraint(k_), w.oc.add_constraint(k_)
    w.memo = {}
    assert step(reset=True)
    assert step() == []
    assert step(reset=True, flags=L.GK_CHANGES_RENDER | L.GK_CHANGES_RESTART) == log[-3]
    assert step() == []
    return log


# ------------------------------------------------------------------------------------------------ 1-6, 8, 9: the PSP set
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_first_stream_is_the_whole_state(backend, fixtures):
    w, _, _, _ = psp_world(backend, fixtures, 64)
    first = w.changes(reset=True)
    assert len(first) > 64 and all(not e[3] and not e[4] and not e[5] for e in first)
    assert w.changes() == []                                                     # a stream begun right after a completed one
    rc, err, page = call(w.c, 0, 64, 0)
    assert rc == L.GK_OK and page["total"] == 0 and page["reset"] == 0 and page["next"] == 0 and page["baseline_bytes"] > 0


@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_steps_of_a_long_running_audit_at_every_page_size(backend, fixtures):
    logs = [run_psp_scenario(backend, fixtures, size) for size in PAGES]
    assert logs[0] == logs[1] == logs[2]                                         # every page size gives the same entries
    assert sum(1 for step in logs[0] if step) >= 10                              # (the steps said something)


# ------------------------------------------------------------------------------------------------ 7. host-completed objects
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_host_completed_pairs_appear_and_resolve(backend):
    cons = [{"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": "NoPrivileged", "metadata": {"name": "np"}, "spec": {}}, RV.need_label("team")]
    c, oc = load_both(backend, [RV.tmpl("NoPrivileged", RV.PRIVILEGED), RV.tmpl("K8sNeedLabel", RV.NEED_LABEL)], cons)
    w = World(c, oc, 64)

    def pod(name, n, privileged=(), labels=None):
        return {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": name, "namespace": "default", "labels": labels if labels is not None else {"team": "x"}},
                "spec": {"containers": [dict({"name": "c%d" % i, "image": "x"}, **({"securityContext": {"privileged": True}} if i in privileged else {})) for i in range(n)]}}

    for i in range(70):
        w.put(pod("small-%02d" % i, 2, privileged=(1,) if i % 3 == 0 else ()))
    w.changes(reset=True)
    huge = pod("huge-priv", 300, privileged=(299,))                              # beyond the device's 255 elements: no device bit carries its pair
    w.put(huge)
    w.put(pod("huge-clean", 300))
    got = w.changes()
    name_of = {c.driver.constraint_id(k): k["metadata"]["name"] for k in c.constraints.values()}
    assert [(e[0][-1], {name_of[i] for i in e[1]}, e[5]) for e in got] == [("huge-priv", {"np"}, False)]
    assert w.changes() == []
    w.remove(huge)
    got = w.changes()
    assert [(e[0][-1], {name_of[i] for i in e[3]}, e[1], e[5]) for e in got] == [("huge-priv", {"np"}, frozenset(), True)]
    assert w.changes() == []


# ------------------------------------------------------------------------------------------------ shapes chosen for the kernels
STRICT_RULE = '''
violation[{"msg": msg}] {
  input.parameters.strict == true
  msg := sprintf("strict constraint %v", [input.parameters.label])
}
'''


def strict_label(name, strict):
    k = RV.need_label(name)
    k["spec"]["parameters"]["strict"] = strict
    return k


def label_world(backend, names, size, n_objects, violates, strict=(), ns_of=lambda i: "ns"):
    c, oc = load_both(backend, [RV.tmpl("K8sNeedLabel", RV.NEED_LABEL)], [strict_label(x, x in strict) for x in names])
    w = World(c, oc, size, memo={}, sig=RV.label_sig)
    for i in range(n_objects):
        w.put(RV.labelled("obj-%05d" % i, ns_of(i), violates.get(i, set()), names))
    return w


def recompile(w, rego):
    """the template is replaced: every constraint of the kind is compiled again under its id -- the rows stay where they are"""
    t = RV.tmpl("K8sNeedLabel", rego)
    w.c.AddTemplate(t), w.oc.add_template(t)
    w.memo = {}


@pytest.mark.parametrize("group_max", [None, 24], ids=["one-plan", "groups-of-24"])
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_seventy_rows_and_plan_groups(backend, group_max):
    """70 constraints of one template: two mask words, an unroll remainder of 2 in the index kernel, two row blocks in the transposes.
    With groups of 24: three groups at rows 0, 24 and 48 (row0 no multiple of 64).  A policy recompile that leaves the row layout as it
    is (the template gains a rule that fires for the constraints 0, 63, 64 and 69 -- the first and the last group) is no reset; every
    slot changes in two groups and counts once."""
    names = ["l%02d" % j for j in range(70)]
    strict = [names[r] for r in (0, 63, 64, 69)]
    violates = {i: {names[i % 70]} | {names[j] for j in range(70) if (i * 7 + j * 3) % 11 == 0} for i in range(0, 130, 2)}
    violates[129] = {names[69]}
    with (plan_group_max(L.load(hostemu=backend.startswith("hostemu")), group_max) if group_max else contextlib.nullcontext()):
        w = label_world(backend, names, 64, 130, violates, strict)
        c = w.c
        first = w.changes(reset=True)
        assert len(first) == len(violates)
        assert w.changes() == []
        ids_before = list(c.driver.ResidentAudit(0)["pairs"])
        recompile(w, RV.NEED_LABEL + STRICT_RULE)
        got = w.changes()                                                         # not a reset
        assert ids_before == list(c.driver.ResidentAudit(0)["pairs"])
        name_of = {c.driver.constraint_id(k): k["metadata"]["name"] for k in c.constraints.values()}
        assert len(got) >= 128 and not any(e[5] for e in got)                     # every object that did not violate all four already; each counts once
        for e in got:
            assert {name_of[i] for i in e[1] ^ e[3]} <= set(strict) and set(strict) <= {name_of[i] for i in e[1]} and e[3] <= e[1]
        assert w.changes() == []
        # objects change in the first and the last group at once
        for i in (1, 64, 129):
            w.put(RV.labelled("obj-%05d" % i, "ns", {names[1], names[68]} if i != 129 else set(), names))
        got = w.changes()
        assert [(e[0][-1], e[5]) for e in got] == [("obj-%05d" % i, gone) for gone in (True, False) for i in (1, 64, 129)]
        recompile(w, RV.NEED_LABEL)                                              # ... and the rule goes again: rows 0, 63, 64, 69 resolve
        got = w.changes()
        assert len(got) >= 128 and not w.last_reset
        if group_max:
            table = c.driver.engine.create_table([D.to_review_in(D.AugmentedUnstructured(D.Unstructured(next(iter(c.cached.values()))), None, ""))])
            try:
                assert table.eval().n_plan_groups == 3
            finally:
                table.free()


@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_one_chunk_of_16500_objects(backend):
    """one chunk of 258 bitmap words: the index kernel runs more than one block.  Every object of words 255, 256 and the last (partial)
    word 257 violates AT THE BASELINE.  They are hidden and shown again at page size 64 -- three pages, which begin at the words 255, 256
    (the index kernel's block boundary) and 257 (the tail word), with was != 0 --, then some are removed, replaced by clean versions and
    replaced by versions with other masks: GONE entries with was != 0 out of the second block, on a page that runs from word 0 to the tail.  Then 1100 violating objects of 18 consecutive words are hidden
    and shown again on pages of 1000 entries: more than one emit block."""
    names = ["team", "zone"]
    n = 16500
    busy = range(6410, 7510)
    edge = list(range(255 * 64, n))
    picks = [255 * 64, 255 * 64 + 63, 256 * 64, n - 1]
    violates = {i: {"team"} for i in busy}
    violates.update({i: {"team"} for i in [3, 5] + edge})
    violates[255 * 64 + 63] = {"team", "zone"}
    w = label_world(backend, names, 64, n, violates, ns_of=lambda i: "busy" if i in busy else "edge" if i in edge else "ns")
    c = w.c
    name_of = {c.driver.constraint_id(k): k["metadata"]["name"] for k in c.constraints.values()}
    named = lambda ids: {name_of[i] for i in ids}   # noqa: E731
    first = w.changes(reset=True)
    assert [e[0][-1] for e in first] == ["obj-%05d" % i for i in sorted(violates)]
    assert w.changes() == []

    def hide(ns):
        ex = [{"excludedNamespaces": [ns], "processes": ["audit"]}] if ns else []
        c.SetExcluder(ex)
        ox = OX.Excluder(ex)
        w.hidden = (lambda o: ox.is_namespace_excluded("audit", o)) if ns else None

    # hidden: every page begins at one of the words 255, 256, 257 and carries what the baseline held there
    hide("edge")
    got = w.changes()
    assert [(e[0][-1], e[5], named(e[3])) for e in got] == [("obj-%05d" % i, True, violates[i]) for i in edge]
    assert [[e[0][-1] for e in p["entries"]] for p in w.last_pages] == [["obj-%05d" % i for i in edge[k:k + 64]] for k in (0, 64, 128)]
    # shown again: a baseline that is there, under a baseline mask that is clear
    hide(None)
    got = w.changes()
    assert [(e[0][-1], e[5], named(e[1]), e[3]) for e in got] == [("obj-%05d" % i, False, violates[i], frozenset()) for i in edge]
    assert [len(p["entries"]) for p in w.last_pages] == [64, 64, n - 257 * 64]
    assert w.changes() == []
    # removed, replaced by a clean version, replaced by a version with other masks
    w.remove(RV.labelled("obj-%05d" % picks[0], "edge", set(), names))
    w.put(RV.labelled("obj-%05d" % picks[1], "edge", set(), names))              # team + zone -> clean
    w.put(RV.labelled("obj-%05d" % picks[2], "edge", {"zone"}, names))           # team -> zone
    w.put(RV.labelled("obj-%05d" % picks[3], "edge", {"team", "zone"}, names))   # team -> team + zone
    w.put(RV.labelled("obj-00003", "ns", {"zone"}, names))
    w.remove(RV.labelled("obj-00005", "ns", set(), names))
    got = w.changes()
    old = [(3, {"team"}), (5, {"team"}), (picks[0], {"team"}), (picks[1], {"team", "zone"}), (picks[2], {"team"}), (picks[3], {"team"})]
    new = [(picks[2], {"zone"}), (picks[3], {"team", "zone"}), (3, {"zone"})]    # (the second chunk, in put order; the clean version has no entry)
    assert [(e[0][-1], e[5], named(e[3]), named(e[1])) for e in got] == \
        [("obj-%05d" % i, True, m, set()) for i, m in old] + [("obj-%05d" % i, False, set(), m) for i, m in new]
    assert [len(p["entries"]) for p in w.last_pages] == [6, 3]                   # words 0, 255, 256, 257 of the first chunk on one page, then the second
    assert w.changes() == []
    for i in range(64 * 10, 64 * 16):                                            # six words of the first chunk lose their (clean) objects: nothing to say
        w.remove(RV.labelled("obj-%05d" % i, "ns", set(), names))
    assert w.changes() == []
    w.size = 1000
    hide("busy")
    got = w.changes()
    assert [(e[0][-1], e[5]) for e in got] == [("obj-%05d" % i, True) for i in busy] and len(w.last_pages) == 2   # (pages take whole words)
    hide(None)
    got = w.changes()
    assert [(e[0][-1], e[5], e[3]) for e in got] == [("obj-%05d" % i, False, frozenset()) for i in busy]
    assert w.changes() == []


# ------------------------------------------------------------------------------------------------ 10. compaction
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_a_compaction_resets_the_stream(backend):
    names = ["team"]
    w = label_world(backend, names, 64, 70, {i: {"team"} for i in range(0, 70, 3)})
    w.track = False
    assert w.changes(reset=True)
    resets = []
    for r in range(17):                                                          # one put and one stream per round: a chunk each, past the 16-chunk limit
        w.put(RV.labelled("late-%02d" % r, "ns", {"team"} if r % 2 == 0 else set(), names))
        got = w.changes(reset=None)
        resets.append(w.last_reset)
        if w.last_reset:                                                          # the whole state, from one chunk
            assert {e[0] for e in got} == set(w.base_oracle) and w.last_pages[0]["n_chunks"] == 1 and all(not e[3] and not e[5] for e in got)
        else:                                                                     # an ordinary delta
            assert [e[0][-1] for e in got] == (["late-%02d" % r] if r % 2 == 0 else [])
    assert sum(resets) == 1 and not resets[0] and not resets[-1], resets


# ------------------------------------------------------------------------------------------------ 11. render and the Python mirror
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_render_and_the_client_generator(backend, fixtures):
    w, pods, nss, used = psp_world(backend, fixtures, 100)
    c, oc = w.c, w.oc

    def oracle_results():
        out = {}
        for r, o in RV.serial_loop(oc, c.cached, memo=RV.PSP_MEMO, sig=RV.text_sig):
            out.setdefault(tuple(D.process_data(o)), []).append((RV.ckey(r.constraint), r.msg, r.enforcement_action))
        return {p: sorted(v) for p, v in out.items()}

    def fold_client(pages, state):
        resets = []
        for reset, entries in pages:
            resets.append(reset)
            if reset:
                state.clear()
            for path, appeared, resolved, gone in entries:
                assert not (gone and appeared)
                state[path] = sorted((RV.ckey(r.constraint), r.msg, r.enforcement_action) for r in appeared)
                if not state[path]:
                    del state[path]
        return resets

    state = {}
    assert all(fold_client(list(c.AuditChangesFromCache(page=100)), state))
    assert state == oracle_results()
    # unrendered pages carry no text; rendered ones only where there is a result now
    bad = [o for o in pods if tuple(D.process_data(o)) in state]
    o2 = copy_of(bad[0]); o2["spec"] = {"containers": []}; o2["metadata"].pop("labels", None)
    o3 = copy_of(bad[1]); o3["spec"]["hostNetwork"] = not o3["spec"].get("hostNetwork", False)
    w.put(o2), w.put(o3)
    rc, err, page = call(c, 0, 100, 0)
    assert rc == L.GK_OK and all(e[6] is None and e[5] for e in page["entries"]) and len(page["entries"]) == 2 and page["reset"] == 0 and page["next"]   # (the old slots; abandoned)
    before = dict(state)
    pages = list(c.AuditChangesFromCache(page=100))
    assert not any(fold_client(pages, state)) and state == oracle_results() and state != before
    resolved = {p: r for _, es in pages for p, _, r, gone in es if gone}
    assert resolved[tuple(D.process_data(o2))] and all(isinstance(k, tuple) for r in resolved.values() for k in r)
    pages = [pg for pg in c.driver.ResidentChanges(100, render=True, restart=True)]
    assert all(pg["reset"] for pg in pages)
    for pg in pages:
        for path, sets, gone, rows in pg["entries"]:
            assert not gone and rows == c.driver.ResidentReview(list(path)) and rows


# ------------------------------------------------------------------------------------------------ edge calls
@pytest.mark.parametrize("backend", RESIDENT_BACKENDS)
def test_edge_calls(backend):
    c, oc = load_both(backend, [RV.tmpl("K8sNeedLabel", RV.NEED_LABEL)], [RV.need_label("team")])
    eng = c.driver.engine
    eng.lib.gk_changes_free(None)
    out = C.POINTER(L.gk_changes_out)()
    assert eng.lib.gk_resident_changes(None, 0, 64, 0, C.byref(out)) == L.GK_ERR_INVALID and eng.lib.gk_resident_changes(eng.handle, 0, 64, 0, None) == L.GK_ERR_INVALID
    rc, err, _ = call(c, 0xDEADBEEF, 64)                                         # before any stream began
    assert rc == L.GK_ERR_INVALID and RV.MOVED in err
    rc, err, page = call(c, 0, 64)                                               # an empty resident set: one empty, last page
    assert rc == L.GK_OK and page["entries"] == [] and page["next"] == 0 and page["total"] == 0 and page["reset"] == 1 and page["baseline_bytes"] == 0
    assert list(c.AuditChangesFromCache()) == [(False, [])]                      # (that one page was the whole stream: an empty baseline)
    o = RV.labelled("obj-0", "default", {"team"}, ["team"])
    c.AddData(o), oc.add_data(o)
    rc, err, page = call(c, 0, 0)                                                # max_objects 0 counts as 64
    assert rc == L.GK_OK and [e[0][-1] for e in page["entries"]] == ["obj-0"] and page["reset"] == 0 and page["next"] == 0
    # the violation stream's cursors and this stream's do not invalidate each other
    for i in range(200):
        o = RV.labelled("more-%03d" % i, "default", {"team"}, ["team"])
        c.AddData(o), oc.add_data(o)
    rc, err, vpage = RV.call(c, 0, 64)
    rc2, err2, cpage = call(c, 0, 64)
    assert rc == L.GK_OK and rc2 == L.GK_OK and vpage["next"] and cpage["next"]
    assert RV.call(c, vpage["next"], 64)[0] == L.GK_OK and call(c, cpage["next"], 64)[0] == L.GK_OK
    assert RV.call(c, cpage["next"] ^ (1 << 40), 64)[0] == L.GK_ERR_INVALID
