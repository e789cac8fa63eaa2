"""What surrounds the dominant kernel in a sweep step: the per-launch counter slots (any number of launches between two collecting
calls, nothing on the stream between two sweeps), the collecting call (one enqueue, one wait, with or without download) and the cached
launch state of a (plan, table) pair.  None of it may change an answer: every case compares with a single launch followed by eval, with
a fresh engine, or with the Python oracle.

On the CPU build the launch path is the emulation's own (tests/native/hostemu.cpp): there the cases check the engine's entry points and
the collecting logic; the counter slots, the pinned counters and the cached launch are exercised by the `gpu` cases."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gatekeeper_amd import driver as D
from gatekeeper_amd import synth
from oracle import client as OC
from oracle import target as OT
from parity_util import BACKENDS, make_client

TWO = [b for b in BACKENDS if b.id in ("hostemu", "gpu")]
N_OBJECTS = 1500          # six 256-review groups, 24 bitmap words, the last one partly filled
SQUEEZED = (2, 4, 2)      # element capacities under which some synthetic pods overflow the LDS accumulators (tools/limits_probe.py)


def _fixtures():
    return synth.load_fixtures()


def _client(backend, constraints=None, **kw):
    c = make_client(backend, **kw)
    for t in synth.psp_templates(_fixtures()):
        c.AddTemplate(t)
    for k in synth.audit_constraints() if constraints is None else constraints:
        c.AddConstraint(k)
    return c


def _table(c, n=N_OBJECTS, seed=synth.SEED, resident=True):
    batch = synth.NativeBatch(c.driver.engine.lib, n, seed=seed, mixed=True, start=0, namespaces=synth.gen_namespaces())
    table = c.driver.engine.create_table_native(batch.reviews, n, keep_docs=False, resident=resident, keep_text=True)
    table._batch = batch   # (the table reads the batch's text)
    return table


def _sweeps(table, k, **kw):
    """k enqueue-only launches, then ONE collecting call -> the device's own answer"""
    for _ in range(k):
        table.launch(want_match=kw.get("want_match", False))
    return table.eval(collect_only=True, host_eval=False, **kw)


def _answer(ev):
    return (ev.viol.tobytes(), ev.err.tobytes(), ev.counts.tobytes(), ev.too_big.tobytes())


def _by_name(c, ev, which="viol"):
    """{(kind, name): bitmap row} -- constraint ids differ from engine to engine"""
    row = {int(cid): i for i, cid in enumerate(ev.constraint_ids)}
    bm = getattr(ev, which)
    return {key: bm[row[c.driver.constraint_id(cons)]].tobytes() for key, cons in c.constraints.items()}


# ---- more pending launches than one block of counter slots

@pytest.mark.parametrize("rpt", ["default", "256"])
@pytest.mark.parametrize("backend", TWO)
def test_any_number_of_launches_between_two_collecting_calls(backend, rpt, monkeypatch):
    """1, 64, 65 and 130 launches before one collecting eval (64 counter slots per block: the last slot of the first block, the first
    of the second, a third block): bitmaps, totals and too_big are those of a single launch followed by eval -- in the first batch of
    each length and in the next one, which reuses the slots the first left behind."""
    if rpt != "default":
        monkeypatch.setenv("GK_RPT", rpt)
    else:
        monkeypatch.delenv("GK_RPT", raising=False)
    c = _client(backend)
    table = _table(c)
    ref = table.eval(host_eval=False)
    assert ref.counts.sum() > 100 and ref.n_reviews == N_OBJECTS
    for k in (1, 64, 65, 130, 65, 1):
        ev = _sweeps(table, k)
        assert ev.n_launches == k
        assert _answer(ev) == _answer(ref), k
        assert ev.n_overflow == ref.n_overflow
    table.free()


# ---- overflow on the last of many launches

def _overflow_check(backend):
    """A non-resident table under squeezed element capacities: some pods overflow the dominant kernel's LDS accumulators and are
    answered by the large-capacity variant (or reported in too_big) -- after 1, 64 and 65 enqueue-only launches exactly as after a
    single evaluation, and as an engine with room for them answers."""
    roomy = _client(backend)
    t0 = _table(roomy, n=300, resident=False)
    want = t0.eval(host_eval=False)
    c = _client(backend, elem_cap=SQUEEZED)
    table = _table(c, n=300, resident=False)
    ref = table.eval(host_eval=False)
    assert ref.n_overflow > 0                       # or the case shows nothing
    refused = set(ref.too_big_reviews())
    # never silently clean: an overflowed review is answered as the roomy engine answers it, or it is in too_big
    keep = np.array([r not in refused for r in range(300)])
    for which in ("viol", "err"):
        a, b = _by_name(c, ref, which), _by_name(roomy, want, which)
        for key in b:
            ba = np.unpackbits(np.frombuffer(a[key], np.uint8), bitorder="little")[:300]
            bb = np.unpackbits(np.frombuffer(b[key], np.uint8), bitorder="little")[:300]
            assert (ba[keep] == bb[keep]).all(), (which, key)
    for k in (1, 64, 65, 1):
        ev = _sweeps(table, k, download=True)
        assert ev.n_overflow == ref.n_overflow, k
        assert _answer(ev) == _answer(ref), k
    # without download the totals on the device are still those of the re-run
    _sweeps(table, 65, download=False)
    assert {cid: p for cid, (_, p) in table.totals().items()} == {int(cid): int(ref.counts[i]) for i, cid in enumerate(ref.constraint_ids)}
    table.free()
    t0.free()


@pytest.mark.parametrize("backend", TWO)
def test_overflow_is_seen_on_the_last_of_many_launches(backend):
    _overflow_check(backend)


def _child(args, extra_env):
    """this file as a script in a fresh process"""
    env = dict(os.environ, **extra_env)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests")] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    return subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)] + args,
                          env=env, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_overflow_is_seen_with_the_counters_in_device_memory():
    """the same with GK_LC_PINNED=0 (read once per process: a child process), the counters in device memory and one small copy in
    front of the collecting wait -- what a device without native host atomics gets"""
    r = _child(["overflow", "gpu"], {"GK_LC_PINNED": "0"})
    assert r.returncode == 0 and "overflow ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the cached launch state of a (plan, table) pair

@pytest.mark.parametrize("backend", TWO)
def test_a_new_constraint_changes_the_plan_under_a_warm_table(backend):
    cons = synth.audit_constraints()
    more = json.loads(json.dumps(cons[0]))
    more["metadata"]["name"] = cons[0]["metadata"]["name"] + "-again"
    c = _client(backend)
    table = _table(c)
    first = _sweeps(table, 3)                      # the second and third launch repeat the first one's resolved state
    c.AddConstraint(more)                          # a new plan id; the table stays
    ev = _sweeps(table, 3)
    fresh = _client(backend, constraints=cons + [more])
    ftable = _table(fresh)
    want = ftable.eval(host_eval=False)
    assert ev.n_constraints == first.n_constraints + 1 == want.n_constraints
    for which in ("viol", "err"):
        assert _by_name(c, ev, which) == _by_name(fresh, want, which)
    got_counts = {key: int(ev.counts[list(ev.constraint_ids).index(c.driver.constraint_id(k))]) for key, k in c.constraints.items()}
    want_counts = {key: int(want.counts[list(want.constraint_ids).index(fresh.driver.constraint_id(k))]) for key, k in fresh.constraints.items()}
    assert got_counts == want_counts and sum(want_counts.values()) > 100
    table.free()
    ftable.free()


@pytest.mark.parametrize("backend", TWO)
def test_two_tables_on_one_engine_keep_their_own_launch_state(backend):
    c = _client(backend)
    a, b = _table(c, n=N_OBJECTS), _table(c, n=700, seed=synth.SEED + 5)
    fresh = _client(backend)
    fa, fb = _table(fresh, n=N_OBJECTS), _table(fresh, n=700, seed=synth.SEED + 5)
    want_a, want_b = fa.eval(host_eval=False), fb.eval(host_eval=False)
    assert _answer(want_a) != _answer(want_b)
    for _ in range(2):
        assert _answer(_sweeps(a, 2)) == _answer(want_a)
        assert _answer(_sweeps(b, 2)) == _answer(want_b)
    # launches of both pending at once, collected in the other order
    a.launch(); b.launch(); b.launch(); a.launch()
    eb, ea = b.eval(collect_only=True, host_eval=False), a.eval(collect_only=True, host_eval=False)
    assert _answer(ea) == _answer(want_a) and _answer(eb) == _answer(want_b)
    for t in (a, b, fa, fb):
        t.free()


@pytest.mark.parametrize("backend", TWO)
def test_want_match_toggled_between_sweeps(backend):
    c = _client(backend)
    table = _table(c)
    fresh = _client(backend)
    ftable = _table(fresh)
    want = ftable.eval(want_match=True, host_eval=False)
    assert want.match is not None and want.match.any()
    for want_match in (False, True, False, True, True, False):
        ev = _sweeps(table, 2, want_match=want_match)
        assert _answer(ev) == _answer(want), want_match
        if want_match:
            assert ev.match is not None and ev.match.tobytes() == want.match.tobytes()
    table.free()
    ftable.free()


@pytest.mark.parametrize("backend", TWO)
def test_an_evaluation_behind_enqueue_only_launches_is_still_timed(backend):
    """plain enqueue-only launches record no timing events; an eval() that launches and collects behind them times its own launch"""
    c = _client(backend)
    table = _table(c)
    ref = table.eval(host_eval=False)
    assert ref.kernel_ms > 0
    for _ in range(2):
        table.launch()
        table.launch()
        ev = table.eval(host_eval=False)
        assert ev.n_launches == 3 and ev.kernel_ms > 0 and ev.fast_kernel_ms > 0
        assert _answer(ev) == _answer(ref)
        if backend == "gpu":
            assert _sweeps(table, 2).kernel_ms == 0          # nothing but enqueue-only launches: no events, no figure
        table.launch(kernel_only=True)
        assert table.eval(collect_only=True, host_eval=False).fast_kernel_ms > 0
    table.free()


def _shard_pass_check(backend):
    """plain sweeps of a warm table, then the engine's sharded sweep of the same table at world size 1 -- detached enqueue-only passes
    and a collecting one, on the shard layout of the result buffers --, then plain sweeps again: each plain answer is a fresh
    engine's, the sharded totals are its counts"""
    import ctypes as C
    from gatekeeper_amd import _lib as L
    from gatekeeper_amd.sweep import ShardedResult
    c = _client(backend)
    eng = c.driver.engine
    table = _table(c)
    fresh = _client(backend)
    ftable = _table(fresh)
    want = ftable.eval(host_eval=False)
    assert _answer(_sweeps(table, 3)) == _answer(want)
    keep = None
    if backend == "hostemu":   # world size 1: the collectives have nothing to move
        keep = (L.HE_ALLGATHER(lambda ctx, buf, n: None), L.HE_ALLREDUCE(lambda ctx, buf, n: None))
        eng._check(eng.lib.gk_comm_init_host(eng.handle, 0, 1, keep[0], keep[1], None))
    else:
        ident = C.create_string_buffer(L.GK_COMM_ID_BYTES)
        eng._check(eng.lib.gk_comm_unique_id(ident))
        eng._check(eng.lib.gk_comm_init(eng.handle, ident.raw, 0, 1))
    for _ in range(2):
        for _ in range(2):
            eng._check(eng.lib.gk_table_sweep_sharded(eng.handle, table.handle, L.GK_SHARD_ENQUEUE, None))
        out = C.POINTER(L.gk_shard_out)()
        eng._check(eng.lib.gk_table_sweep_sharded(eng.handle, table.handle, L.GK_SHARD_DOWNLOAD, C.byref(out)))
        res = ShardedResult(eng.lib, out)
        assert (res.totals == want.counts.astype(np.int64)).all() and res.beyond_limits == 0
        assert _answer(_sweeps(table, 3)) == _answer(want)
        eng._check(eng.lib.gk_table_sweep_sharded(eng.handle, table.handle, L.GK_SHARD_ENQUEUE, None))   # a detached pass left uncollected
        assert _answer(_sweeps(table, 2)) == _answer(want)
    table.free()
    ftable.free()


def test_a_sharded_pass_between_plain_sweeps_on_the_cpu_build():
    _shard_pass_check("hostemu")


@pytest.mark.gpu
def test_a_sharded_pass_between_plain_sweeps_on_the_device():
    """(a child process: the engine's RCCL communicator stays out of the test process)"""
    r = _child(["shard", "gpu"], {})
    assert r.returncode == 0 and "shard ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the collecting call, with and without download, against the Python oracle

N_ORACLE = 384


@functools.lru_cache(maxsize=None)
def _oracle():
    """the pure-Python oracle over the first N_ORACLE synthetic objects -> ({(kind, name): set of violating reviews}, {(kind, name): results})"""
    oc = OC.Client()
    for t in synth.psp_templates(_fixtures()):
        oc.add_template(t)
    for k in synth.audit_constraints():
        oc.add_constraint(k)
    nss = synth.gen_namespaces()
    pairs, results = {}, {}
    for i, o in enumerate(synth.gen_objects(N_ORACLE, seed=synth.SEED, mixed=True)):
        for r in oc.review(OT.AugmentedUnstructured(OT.Unstructured(o), synth.namespace_for(o, nss), "Original"), OC.AUDIT_EP):
            key = (r.constraint["kind"], r.constraint["metadata"]["name"])
            pairs.setdefault(key, set()).add(i)
            results[key] = results.get(key, 0) + 1
    return pairs, results


@pytest.mark.parametrize("backend", TWO)
def test_collecting_with_and_without_download_agrees_with_the_oracle(backend):
    pairs, results = _oracle()
    assert sum(len(v) for v in pairs.values()) > 100
    c = _client(backend)
    table = _table(c, n=N_ORACLE)
    name_of = {c.driver.constraint_id(k): key for key, k in c.constraints.items()}

    def totals_ok():
        tot = table.totals()
        assert {name_of[cid]: v[1] for cid, v in tot.items() if v[1]} == {k: len(v) for k, v in pairs.items()}
        assert {name_of[cid]: v[0] for cid, v in tot.items() if v[0]} == results

    for k in (1, 3):
        table.launch() if k == 1 else [table.launch() for _ in range(k)]
        ev = table.eval(download=False, collect_only=True)
        assert ev.n_launches == k                          # (no bitmaps asked for: the totals below are the device's)
        totals_ok()
        for _ in range(k):
            table.launch()
        ev = table.eval(download=True, collect_only=True)
        got = {name_of[int(cid)]: set(int(r) for r in D.EvalResult.bits(ev.viol[i], ev.n_reviews)) for i, cid in enumerate(ev.constraint_ids)}
        assert {k_: v for k_, v in got.items() if v} == pairs
        assert {name_of[int(cid)]: int(ev.counts[i]) for i, cid in enumerate(ev.constraint_ids) if ev.counts[i]} == {k_: len(v) for k_, v in pairs.items()}
        assert not ev.too_big_reviews() and not ev.err.any()
        totals_ok()
    table.free()


if __name__ == "__main__":
    if sys.argv[1:2] == ["overflow"]:
        _overflow_check(sys.argv[2])
        print("overflow ok")
    if sys.argv[1:2] == ["shard"]:
        _shard_pass_check(sys.argv[2])
        print("shard ok")
