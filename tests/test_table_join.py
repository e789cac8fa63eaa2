"""gk_table_join: the objects of two listings lined up by key -- on the host (delta_join over the two key orders) and on the device
(GK_CHANGES_DEVICE_JOIN: gk_kjoin_build + gk_kjoin_probe + gk_kjoin_finish, an exact hash join keyed by the key bytes, with the host
settling the keys that occur more than once; tests/native/hostemu_kjoin.cpp on the CPU build).

The expected join is a Python dict over the key tuples (group, version, kind, namespace, name) with the contract's occurrence rule: the
i-th review of a key matches the i-th on the other side, a review without a key matches nothing.  Nothing of the new code computes it.
Every case checks the device join against it AND against the host join, array by array, calls the device join twice (identical arrays
and stats: atomics decide who owns a slot, never an answer), and checks the stats.  Shapes are the smallest at which the kernels can go
wrong: the word edges of `unmatched` and the wave edges (63 / 64 / 65), more than one block (257), records that end at a 16-byte unit's
edge, forced hash collisions.  The pure parts: tests/test_key_join_native.py."""
import random

import numpy as np
import pytest

from gatekeeper_amd import _lib as L
from gatekeeper_amd import driver as D
from parity_util import BACKENDS, make_client
from test_table_violations import DENY_LABEL, delete_without_old_object, deny, tmpl

TABLE_BACKENDS = [b for b in BACKENDS if b.id in ("hostemu", "gpu")]
NONE = 0xFFFFFFFF
SIZES = (0, 1, 63, 64, 65, 257)

_clients = {}


@pytest.fixture(scope="module", autouse=True)
def clients_of_this_module():
    """the clients engine() made live as long as this module's tests and are closed after the last of them"""
    yield
    for c in _clients.values():
        c.driver.engine.close()
    _clients.clear()


def engine(backend):
    """one client per backend for the whole module: a snapshot needs an evaluated table, so one constraint is loaded"""
    if backend not in _clients:
        c = make_client(backend)
        c.AddTemplate(tmpl("K8sDenyLabel", DENY_LABEL))
        c.AddConstraint(deny("l0"))
        _clients[backend] = c
    return _clients[backend].driver.engine


def obj(kind, ns, name, api="v1"):
    return {"apiVersion": api, "kind": kind, "metadata": {"name": name, "namespace": ns, "labels": {}}}


def key_of(o):
    if o is None:
        return None
    g, v, k = D.obj_gvk(o)
    return (g, v, k, o["metadata"]["namespace"], o["metadata"]["name"])


def review(o):
    return D.to_review_in(delete_without_old_object()) if o is None else D.to_review_in(D.AugmentedUnstructured(D.Unstructured(o), None, ""))


def occurrences(keys):
    seen, out = {}, []
    for k in keys:
        if k is None:
            out.append(None)
            continue
        seen[k] = seen.get(k, -1) + 1
        out.append((k, seen[k]))
    return out


def expected(now, then):
    """(then_of, now_of) by the contract's rules, and how many reviews of either side carry a key that occurs more than once on some
    side and is present then (what the device leaves to the host)"""
    kn, kt = [key_of(o) for o in now], [key_of(o) for o in then]
    p_of = {k: p for p, k in enumerate(occurrences(kt)) if k is not None}
    then_of = [NONE if k is None else p_of.get(k, NONE) for k in occurrences(kn)]
    now_of = [NONE] * len(then)
    for r, p in enumerate(then_of):
        if p != NONE:
            now_of[p] = r
    multi = {k for k in set(kt) if k is not None and (kt.count(k) > 1 or kn.count(k) > 1)}
    return then_of, now_of, sum(k in multi for k in kn), sum(k in multi for k in kt)


def check_join(backend, now, then, device_keys=True):
    """-> the device join's stats"""
    eng = engine(backend)
    t_then = eng.create_table([review(o) for o in then])
    t_now, snap = None, None
    try:
        t_then.eval()
        snap = t_then.snapshot(device_keys=device_keys)
        t_then.free()                                                            # the snapshot outlives its table
        t_now = eng.create_table([review(o) for o in now])                       # never evaluated: the join needs the keys only
        want_then_of, want_now_of, res_now, res_then = expected(now, then)
        h_then_of, h_now_of, h_st = t_now.join(snap, device=False)
        d_then_of, d_now_of, d_st = t_now.join(snap, device=True)
        again = t_now.join(snap, device=True)
        assert list(h_then_of) == want_then_of and list(h_now_of) == want_now_of
        assert list(d_then_of) == want_then_of and list(d_now_of) == want_now_of
        assert np.array_equal(again[0], d_then_of) and np.array_equal(again[1], d_now_of)
        d_st.pop("pack_ms"), again[2].pop("pack_ms"), d_st.pop("join_ms"), again[2].pop("join_ms")    # (times differ from call to call)
        assert again[2] == d_st
        assert d_st == {"n_now": len(now), "n_then": len(then), "capacity": d_st["capacity"], "host_resolved_now": res_now, "host_resolved_then": res_then,
                        "device": 1, "fallback": 0}
        cap = d_st["capacity"]
        assert cap >= 1 and cap & (cap - 1) == 0 and cap >= 2 * len(then) and (not then or cap < 4 * len(then))
        assert (h_st["device"], h_st["fallback"], h_st["capacity"], h_st["n_now"], h_st["n_then"], h_st["join_ms"]) == (0, 0, 0, len(now), len(then), 0.0)
        return d_st
    finally:
        for x in (t_now, snap, t_then):
            if x:
                x.free()


def two_listings(n_now, n_then, seed):
    """unique keys; the second listing shuffled, about a third of each side's keys on that side only"""
    rnd = random.Random(seed)
    both = max(0, min(n_now, n_then) - min(n_now, n_then) // 3)
    mk = lambda i: obj("ConfigMap", "ns-%d" % (i % 5), "o-%05d" % i)
    then = [mk(i) for i in range(both)] + [mk(1000 + i) for i in range(n_then - both)]
    now = [mk(i) for i in range(both)] + [mk(2000 + i) for i in range(n_now - both)]
    rnd.shuffle(then)
    rnd.shuffle(now)
    return now, then


SIZE_PAIRS = [(0, 0), (0, 65), (65, 0), (1, 1), (1, 64), (63, 65), (64, 64), (65, 63), (257, 64), (64, 257), (257, 257)]


# ------------------------------------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_sizes_at_the_word_wave_and_block_edges(backend):
    assert {n for pair in SIZE_PAIRS for n in pair} == set(SIZES)
    for k, (n_now, n_then) in enumerate(SIZE_PAIRS):
        now, then = two_listings(n_now, n_then, seed=k)
        st = check_join(backend, now, then, device_keys=k % 2 == 0)               # (odd cases: the snapshot's keys go up at the first join)
        assert st["host_resolved_now"] == 0 and st["host_resolved_then"] == 0


# ------------------------------------------------------------------------------------------------ 2. key bytes
def sized(total, tag):
    """an object of kind A whose key has `total` bytes: \\0 v1 \\0 A \\0 ns \\0 name = 7 + len(ns) + len(name)"""
    o = obj("A", "n", tag + "x" * (total - 8 - len(tag)))
    assert len("\0".join(key_of(o))) == total
    return o


@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_key_bytes_at_the_record_edges_and_near_misses(backend):
    # records end at 4 + length: 15, 16, 17 and 31, 32, 33 bytes
    edge = [sized(t, "e") for t in (11, 12, 13, 27, 28, 29)]
    last = [obj("A", "n", "same-prefix-and-length-a"), obj("A", "n", "same-prefix-and-length-b")]          # differ in the last byte only
    first = [obj("A", "n", "a-same-suffix-and-length"), obj("A", "n", "b-same-suffix-and-length")]        # ... in the first byte of the name
    group = [obj("A", "n", "g", api="x/v1"), obj("A", "n", "g", api="y/v1")]                              # ... in the first byte of the key
    prefix = [obj("A", "n", "pre"), obj("A", "n", "prefix"), obj("A", "n", "prefix-of-a-longer-name-than-one-unit")]
    sep = [obj("A", "ab", "c"), obj("A", "a", "bc")]                                                      # the same bytes but for the separator's place
    assert "\0".join(key_of(sep[0])).replace("\0", "") == "\0".join(key_of(sep[1])).replace("\0", "")
    everything = edge + last + first + group + prefix + sep
    # of every near-miss pair one side holds one key, the other side the other ...
    then = [edge[0], edge[2], edge[4], last[0], first[0], group[0], prefix[0], prefix[2], sep[0]] + [sized(t, "t") for t in (11, 12, 13, 27, 28, 29)]
    now = [sep[1], prefix[1], group[1], first[1], last[1], edge[5], edge[3], edge[1]] + [edge[0], edge[2], sep[0], last[0]]   # ... plus four on both
    st = check_join(backend, now, then)
    assert st["host_resolved_now"] == 0 and st["host_resolved_then"] == 0
    then_of, _, _, _ = expected(now, then)
    assert [p for p in then_of if p != NONE] == [0, 1, 8, 3]                      # edge[0], edge[2], sep[0], last[0]: nothing else pairs
    st = check_join(backend, everything, list(reversed(everything)))               # all of them on both sides: each finds exactly itself
    assert st["host_resolved_now"] == 0


# ------------------------------------------------------------------------------------------------ 3. no key
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_reviews_without_a_key_match_nothing(backend):
    a, b, c = obj("ConfigMap", "default", "a"), obj("ConfigMap", "default", "b"), obj("ConfigMap", "default", "c")
    then = [a, None, b, None, None]
    now = [None, b, None, c, a, None]
    st = check_join(backend, now, then)
    assert st["host_resolved_now"] == 0 and st["host_resolved_then"] == 0
    assert expected(now, then)[:2] == ([NONE, 2, NONE, NONE, 0, NONE], [4, NONE, 1, NONE, NONE])


# ------------------------------------------------------------------------------------------------ 4. duplicates
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_duplicates_pair_by_occurrence_on_the_host(backend):
    u = [obj("ConfigMap", "default", "u-%03d" % i) for i in range(70)]            # unique keys around them, across a word edge
    d21, d12, d32, only_now = obj("ConfigMap", "default", "two-one"), obj("Secret", "default", "one-two"), obj("ConfigMap", "kube", "three-two"), obj("ConfigMap", "x", "now-only")
    then = u[:30] + [d21, d32] + u[30:60] + [d21, d12, d32] + u[60:] + [d32]
    now = [d32, only_now] + u[69::-1] + [d12, d21, only_now, d12, d32]
    st = check_join(backend, now, then)
    assert (st["host_resolved_now"], st["host_resolved_then"]) == (1 + 2 + 2, 2 + 1 + 3)
    then_of, now_of, _, _ = expected(now, then)
    assert then_of[0] == 31 and then_of[-1] == 64 and then_of[1] == NONE and then_of[-3] == NONE          # occurrences in review order; a key duplicated now and absent then: all new
    assert now_of[len(then) - 1] == NONE                                                                  # the third of three-two is gone
    # a key duplicated now and absent then alone: nothing for the host
    st = check_join(backend, [only_now, u[0], only_now], [u[0], u[1]])
    assert (st["host_resolved_now"], st["host_resolved_then"]) == (0, 0)


# ------------------------------------------------------------------------------------------------ 5. forced collisions
@pytest.mark.parametrize("bits", [0, 3])
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_colliding_hashes_change_nothing(backend, bits):
    """every key one home and one tag (0 bits) / eight homes and one tag (3): the probes walk long runs and compare bytes everywhere; a
    collision is not a duplicate and never reaches the host"""
    lib = L.load(hostemu=backend.startswith("hostemu"))
    assert lib.gk_debug_set(b"kjoin_hash_bits", bits) == 0
    try:
        for n_now, n_then in ((65, 65), (257, 65), (65, 257), (257, 257)):
            now, then = two_listings(n_now, n_then, seed=bits)
            st = check_join(backend, now, then)
            assert (st["host_resolved_now"], st["host_resolved_then"], st["fallback"], st["device"]) == (0, 0, 0, 1)
    finally:
        assert lib.gk_debug_set(b"kjoin_hash_bits", 64) == 0


# ------------------------------------------------------------------------------------------------ 6. / 7. twice, stats, refusals
@pytest.mark.parametrize("backend", TABLE_BACKENDS)
def test_the_join_of_another_engines_snapshot_is_refused(backend):
    eng = engine(backend)
    t = eng.create_table([review(obj("ConfigMap", "default", "a"))])
    other = make_client(backend)
    other.AddTemplate(tmpl("K8sDenyLabel", DENY_LABEL))
    other.AddConstraint(deny("l0"))
    ot = other.driver.engine.create_table([review(obj("ConfigMap", "default", "a"))])
    snap = None
    try:
        ot.eval()
        snap = ot.snapshot()
        with pytest.raises(D.EngineError) as ei:
            t.join(snap, device=True)
        assert ei.value.code == L.GK_ERR_INVALID and "another engine" in str(ei.value)
        with pytest.raises(ValueError):
            t.join(None)
    finally:
        for x in (snap, ot, t):
            if x:
                x.free()
