"""What gk_table_changes costs against what the code before it offers for the same answer -- two complete gk_table_violations streams,
joined by object on the host -- between two list-based audit cycles (profiles/table_changes.md), on one GPU.

  python tools/table_changes_cost.py all --out DIR          every churn below as a child process of its own, each under its own time limit
  python tools/table_changes_cost.py pair --objects N --churn P [--shuffle] [--keep-keys]
                                                            cycle 1: N synthetic objects (seed 23) in one table, evaluated, snapshot taken;
                                                            cycle 2: the same objects with P % of them regenerated from another seed (a regenerated
                                                            object whose kind or namespace came out differently -- most of them -- is a gone
                                                            object plus a new one), in the same listing order or, with
                                                            --shuffle, in a random one.  --keep-keys regenerates only objects whose kind and
                                                            namespace come out the same under the other seed (up to P % of N, as many as there
                                                            are): same object, other content.  Timed per repeat, alternating:
                                                            (a) gk_table_changes against the snapshot, pages of 65 536, without rendering;
                                                            (b) gk_table_violations of cycle 2, whole stream, joined with cycle 1's kept stream by
                                                                the object's position in the first listing (numpy: sort + searchsorted + compare;
                                                                an integer stands in for the key, which favours (b)).
                                                            Both are checked to name the same changed objects before anything is timed.
                                                            --device-join adds, in the same process and on the same tables:
                                                            (c) gk_table_changes with GK_CHANGES_DEVICE_JOIN against a snapshot taken with
                                                                GK_SNAPSHOT_DEVICE_KEYS, checked to give (a)'s entries one by one; the first such
                                                                call packs and uploads the table's keys (pack_ms), the repeats find them there;
                                                            and, once, on the freshly built first table: gk_table_snapshot_ex with device keys
                                                            (no sort) against gk_table_snapshot (the key sort, table_key_order).

Workload: the configs[2] policy set.  Every wall time is a host clock around C calls that end in a stream synchronise; device_ms is the
HIP-event time of a call's kernels.  Reads nothing outside the tree."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = sorted(xs)
    return "%.3f / %.3f / %.3f ms" % (xs[0] * 1e3, xs[len(xs) // 2] * 1e3, xs[-1] * 1e3)


def step_pair(args):
    import numpy as np
    from gatekeeper_amd import _lib as L
    from gatekeeper_amd import driver as D
    from gatekeeper_amd import synth
    os.environ["GK_JIT_STRICT"] = "1"
    lib = L.load(hostemu=args.hostemu)
    c = D.Client(D.Driver(hostemu=True) if args.hostemu else D.Driver(device=0, hostemu=False))
    for t in synth.psp_templates(synth.load_fixtures()):
        c.AddTemplate(t)
    for k in synth.audit_constraints():   # configs[2]
        c.AddConstraint(k)
    eng = c.driver.engine
    n = args.objects
    nss = synth.gen_namespaces()
    rng = np.random.default_rng(7)
    t0 = time.perf_counter()
    first = synth.NativeBatch(lib, n, seed=23, mixed=True, namespaces=nss)
    other = synth.NativeBatch(lib, n, seed=29, mixed=True, namespaces=nss) if args.churn else None
    churned = np.zeros(n, bool)
    want = min(n, max(1, n * args.churn // 100)) if args.churn else 0
    if args.churn and args.keep_keys:
        # only objects that come out with the same kind and namespace under the other seed (the name follows from kind and position): their
        # KEY stays and their content changes -- "same object, other result"
        import re
        kind_re, ns_re = re.compile(rb'"kind":\s*"(\w+)"'), re.compile(rb'"namespace":\s*"([^"]*)"')

        def key(batch, i):
            text = batch.json_text(i)
            k, m = kind_re.search(text), ns_re.search(text)
            return (k.group(1) if k else None, m.group(1) if m else None)
        got = 0
        for i in rng.permutation(n):
            if got >= want:
                break
            if key(first, int(i)) == key(other, int(i)):
                churned[i] = True
                got += 1
    elif args.churn:
        churned[rng.choice(n, size=want, replace=False)] = True
    ident = rng.permutation(n) if args.shuffle else np.arange(n)      # position in the second listing -> position in the first
    a, b = first.reviews, other.reviews if other else None
    second = (L.gk_review_in * n)()
    for q in range(n):
        i = int(ident[q])
        second[q] = b[i] if churned[i] else a[i]
    then = eng.create_table_native(a, n, resident=True, pruned=True)
    now = eng.create_table_native(second, n, resident=True, pruned=True)
    print("two tables of %d objects, %d regenerated, %s order: %.1f s" % (n, int(churned.sum()), "shuffled" if args.shuffle else "the same", time.perf_counter() - t0), flush=True)

    def evaluate(table, flags):
        out = C.POINTER(L.gk_eval_out)()
        t0 = time.perf_counter()
        eng._check(eng.lib.gk_table_eval(eng.handle, table.handle, flags, C.byref(out)))
        dt = time.perf_counter() - t0
        eng.lib.gk_eval_free(out)
        return dt

    def violations(table):
        """the whole gk_table_violations stream -> (seconds, reviews, viol, err)"""
        t0, cursor, revs, vs, es = time.perf_counter(), 0, [], [], []
        while True:
            out = C.POINTER(L.gk_table_violations_out)()
            eng._check(eng.lib.gk_table_violations(eng.handle, table.handle, cursor, 65536, 0, C.byref(out)))
            o = out.contents
            if o.n_entries:
                shape = (o.n_entries, o.mask_words)
                revs.append(np.ctypeslib.as_array(o.reviews, (o.n_entries,)).copy())
                vs.append(np.ctypeslib.as_array(o.viol, shape).copy())
                es.append(np.ctypeslib.as_array(o.err, shape).copy())
            cursor, mw = int(o.next_cursor), int(o.mask_words)
            eng.lib.gk_table_violations_free(out)
            if not cursor:
                break
        cat = lambda xs, empty: np.concatenate(xs) if xs else empty   # noqa: E731
        return time.perf_counter() - t0, cat(revs, np.zeros(0, np.uint32)), cat(vs, np.zeros((0, mw), np.uint64)), cat(es, np.zeros((0, mw), np.uint64))

    def changes(snap, call_flags=0):
        """the whole gk_table_changes stream -> (seconds per call, device_ms per call, changed first-listing positions or -1, gone, new)"""
        times, dev, cursor, who, flags, revs = [], [], 0, [], [], []
        by_kernel = np.zeros(3)
        while True:
            out = C.POINTER(L.gk_table_changes_out)()
            t0 = time.perf_counter()
            rc = eng.lib.gk_table_changes(eng.handle, now.handle, snap.handle, None, cursor, 65536, call_flags, C.byref(out))
            times.append(time.perf_counter() - t0)
            eng._check(rc)
            o = out.contents
            dev.append(float(o.device_ms))
            by_kernel += (float(o.align_ms), float(o.index_ms), float(o.emit_ms))
            if o.n_entries:
                who.append(np.ctypeslib.as_array(o.was_reviews, (o.n_entries,)).copy())
                flags.append(np.ctypeslib.as_array(o.entry_flags, (o.n_entries,)).copy())
                revs.append(np.ctypeslib.as_array(o.reviews, (o.n_entries,)).copy())
            cursor, total = int(o.next_cursor), int(o.total_entries)
            eng.lib.gk_table_changes_free(out)
            if not cursor:
                break
        who = np.concatenate(who) if who else np.zeros(0, np.uint32)
        flags = np.concatenate(flags) if flags else np.zeros(0, np.uint32)
        revs = np.concatenate(revs) if revs else np.zeros(0, np.uint32)
        assert len(who) == total, (len(who), total)
        is_new = (flags & L.GK_CHANGE_NEW) != 0
        who = who.astype(np.int64)
        who[is_new] = ident[revs[is_new]]                             # a new object: where the first listing had its predecessor
        return times, dev, who, flags, by_kernel

    def host_join(kept, fresh):
        """(b)'s join: cycle 1's kept entries against cycle 2's by the object's position in the first listing -> (seconds, changed positions)"""
        t0 = time.perf_counter()
        r1, v1, e1 = kept
        r2, v2, e2 = fresh
        id2 = ident[r2]
        order = np.argsort(id2, kind="stable")
        id2s = id2[order]
        at = np.searchsorted(id2s, r1)
        hit = (at < len(id2s)) & (id2s[np.minimum(at, max(len(id2s) - 1, 0))] == r1) if len(id2s) else np.zeros(len(r1), bool)
        gone = r1[~hit]                                              # had results, has none now (or is not listed any more)
        j = order[at[hit]]
        differ = ((v1[hit] != v2[j]) | (e1[hit] != e2[j])).any(axis=1)
        seen = np.zeros(len(r2), bool)
        seen[j] = True
        appeared = id2[~seen]                                        # has results now, had none
        changed = np.concatenate([gone, r1[hit][differ], appeared])
        return time.perf_counter() - t0, np.sort(changed)

    evaluate(then, 0)
    snap_keys = None
    if args.device_join:   # on the fresh table, the one without a sort first: gk_table_snapshot sorts the table's keys once and the table keeps the order
        t0 = time.perf_counter()
        snap_keys = then.snapshot(device_keys=True)
        t_keys = time.perf_counter() - t0
    t0 = time.perf_counter()
    snap = then.snapshot()
    t_plain = time.perf_counter() - t0
    info = snap.info()
    if snap_keys:
        ik = snap_keys.info()
        print("on the freshly built table: gk_table_snapshot_ex(GK_SNAPSHOT_DEVICE_KEYS) %.1f ms (no sort; %d B on the device, %d B on the host) | gk_table_snapshot %.1f ms "
              "(table_key_order's sort; %d B on the device, %d B on the host)" % (t_keys * 1e3, ik["device_bytes"], ik["host_bytes"], t_plain * 1e3, info["device_bytes"], info["host_bytes"]),
              flush=True)
    _, *kept = violations(then)
    then.free()                                                      # cycle 1's table is gone, as in a real audit; its answer is the snapshot / the kept stream
    evaluate(now, 0)
    print("snapshot: %d B on the device, %d B on the host; cycle 1 has %d entries" % (info["device_bytes"], info["host_bytes"], len(kept[0])), flush=True)
    # ---- the same answer?  Compared by position in the first listing.  A regenerated object whose KEY changed is a gone and a new entry
    # in (a) even where its masks stayed, and one position in (b) only where they differ: (a) may name more, among the regenerated only.
    _, _, who, flags, _ = changes(snap)
    _, *fresh = violations(now)
    _, changed_b = host_join(kept, fresh)
    n_gone, n_new = int(((flags & L.GK_CHANGE_GONE) != 0).sum()), int(((flags & L.GK_CHANGE_NEW) != 0).sum())
    in_a, in_b = set(int(x) for x in who), set(int(x) for x in changed_b)
    same = in_b <= in_a and all(churned[i] for i in in_a - in_b)
    print("entries: gk_table_changes %d (%d matched and changed, %d gone, %d new) at %d positions; host join %d changed positions; consistent: %s"
          % (len(who), len(who) - n_gone - n_new, n_gone, n_new, len(in_a), len(in_b), same), flush=True)
    if not same or (args.keep_keys and (n_gone or n_new)):
        sys.exit(2)
    c_all, c_first, c_later, c_join, c_stats = [], [], [], [], None
    if snap_keys:   # (c) names what (a) names, entry by entry; this first call is the one that packs and uploads the table's keys
        evaluate(now, L.GK_EVAL_NO_DOWNLOAD)
        times, _, who_c, flags_c, _ = changes(snap_keys, L.GK_CHANGES_DEVICE_JOIN)
        first_stats = now.changes_join()
        if not (np.array_equal(who_c, who) and np.array_equal(flags_c, flags)) or first_stats["device"] != 1:
            print("the device-join stream differs from the host-join stream, or the device did not join: %r" % (first_stats,), flush=True)
            sys.exit(3)
        print("(c) first device-join call on this table: cursor-0 call %.3f ms, of which key pack + upload of the now side %.3f ms; join kernels %.3f ms"
              % (times[0] * 1e3, first_stats["pack_ms"], first_stats["join_ms"]), flush=True)
    a_all, a_first, a_later, a_dev, a_kern, b_all, b_stream, b_join = [], [], [], [], [], [], [], []
    for _ in range(args.repeat):
        if snap_keys:
            evaluate(now, L.GK_EVAL_NO_DOWNLOAD)
            times, _, _, _, _ = changes(snap_keys, L.GK_CHANGES_DEVICE_JOIN)
            c_stats = now.changes_join()
            c_all.append(sum(times)); c_first.append(times[0]); c_later += times[1:]; c_join.append(c_stats["join_ms"] / 1e3)
        evaluate(now, L.GK_EVAL_NO_DOWNLOAD)                         # a new evaluation: the stream's state is built again at cursor 0
        times, dev, _, _, kern = changes(snap)
        a_all.append(sum(times)); a_first.append(times[0]); a_later += times[1:]; a_dev.append(dev); a_kern.append(kern)
        evaluate(now, L.GK_EVAL_NO_DOWNLOAD)
        st, *fresh = violations(now)
        jt, _ = host_join(kept, fresh)
        b_all.append(st + jt); b_stream.append(st); b_join.append(jt)
    print("(min / median / max) (a) gk_table_changes, whole stream %s [cursor-0 call: join + align + index + first page %s | later pages %s]"
          % (stats(a_all), stats(a_first), stats(a_later) if a_later else "-"))
    print("(min / median / max) (b) gk_table_violations, whole stream + host join %s [stream %s | join %s]" % (stats(b_all), stats(b_stream), stats(b_join)))
    med = sorted(a_dev, key=sum)[len(a_dev) // 2]
    print("device_ms per call of the median changes stream (cursor-0 call: align + index [+ the gone side] + first page): %s" % " ".join("%.3f" % x for x in med))
    kern = sorted(a_kern, key=sum)[len(a_kern) // 2]
    print("device time per kernel over the median changes stream, all its calls and both sides: gk_tchg_align %.3f ms | gk_tchg_index %.3f ms | gk_tchg_emit %.3f ms"
          % tuple(kern), flush=True)
    if snap_keys:
        print("(min / median / max) (c) gk_table_changes with the device join, keys already on the device, whole stream %s [cursor-0 call %s | later pages %s]"
              % (stats(c_all), stats(c_first), stats(c_later) if c_later else "-"))
        print("(c) cursor-0 + pack: %.3f ms = the median cursor-0 call of the repeats %.3f ms + the first call's key pack + upload %.3f ms (a sum of two measured figures: what "
              "a cycle that builds a new table pays)" % (sorted(c_first)[len(c_first) // 2] * 1e3 + first_stats["pack_ms"], sorted(c_first)[len(c_first) // 2] * 1e3, first_stats["pack_ms"]))
        print("(c) join kernels (HIP events) %s; capacity %d; host_resolved_now %d, host_resolved_then %d; fallback %d"
              % (stats(c_join), c_stats["capacity"], c_stats["host_resolved_now"], c_stats["host_resolved_then"], c_stats["fallback"]), flush=True)
        snap_keys.free()
    snap.free()
    now.free()


def step_all(args):
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "pair", "--objects", str(args.objects), "--repeat", str(args.repeat)] + (["--device-join"] if args.device_join else [])
    steps = [(churn, shuffle, False) for churn in (0, 1, 100) for shuffle in (False, True)] + [(1, False, True), (1, True, True)]   # (fewer than 1 % of the objects keep their key under the other seed)
    for churn, shuffle, keep in steps:   # a fresh child per step, each under its own limit; a step that fails or runs out ends the run
        name = "churn%d_%s%s" % (churn, "shuffled" if shuffle else "same", "_keys_kept" if keep else "")
        with open(os.path.join(args.out, name + ".log"), "w") as log:
            rc = subprocess.run(me + ["--churn", str(churn)] + (["--shuffle"] if shuffle else []) + (["--keep-keys"] if keep else []), stdout=log, stderr=subprocess.STDOUT,
                                timeout=args.limit).returncode
        print("%s: exit status %d" % (name, rc), flush=True)
        if rc != 0:
            sys.exit(rc)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["all", "pair"])
    ap.add_argument("--objects", type=int, default=1000000)
    ap.add_argument("--churn", type=int, default=1)
    ap.add_argument("--shuffle", action="store_true")
    ap.add_argument("--keep-keys", action="store_true")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default="table_changes_out")
    ap.add_argument("--hostemu", action="store_true")
    ap.add_argument("--device-join", action="store_true")
    a = ap.parse_args()
    {"all": step_all, "pair": step_pair}[a.step](a)
