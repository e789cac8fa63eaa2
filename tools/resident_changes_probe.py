"""What gk_resident_changes costs beside gk_resident_violations at low churn (profiles/resident_changes.md), on one GPU.

  python tools/resident_changes_probe.py [--objects 1000000] [--churn 0.001] [--runs 5] [--page 65536] [--hostemu]

configs[2]'s shape: the 50 audit constraints over N mixed resident objects.  One changes stream is read to its end (the baseline); then,
per run, `churn` of the objects are replaced by a changed version, the set is swept (not timed: flattening and evaluating the new chunk
is the same work for both streams), and two complete unrendered streams over that one state are timed in the same process: the changes
stream (wall clock and its device_ms), then the full violation stream.  The first run warms up and is dropped; the medians of the others
are printed as one JSON line.  Every wall time is a host clock around C calls that end in a stream synchronise.  --hostemu rehearses the
script on the CPU stand-in; its times mean nothing.  Reads nothing outside the tree; objects come from the seeded synthetic stream."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def put_text(eng, path, text):
    arr = (C.c_char_p * len(path))(*[p.encode() for p in path])
    eng._check(eng.lib.gk_data_put(eng.handle, arr, len(path), text, len(text)))


def changes_stream(eng, L, page):
    """-> (wall seconds, device ms, entries, pages, reset, baseline bytes)"""
    cursor, n, pages, dev, t0 = 0, 0, 0, 0.0, time.perf_counter()
    while True:
        out = C.POINTER(L.gk_changes_out)()
        eng._check(eng.lib.gk_resident_changes(eng.handle, cursor, page, 0, C.byref(out)))
        o = out.contents
        n, pages, dev = n + o.n_entries, pages + 1, dev + o.device_ms
        cursor, total, reset, held = int(o.next_cursor), int(o.total_entries), int(o.reset), int(o.baseline_bytes)
        eng.lib.gk_changes_free(out)
        if not cursor:
            assert n == total, (n, total)
            return time.perf_counter() - t0, dev, n, pages, reset, held


def violations_stream(eng, L, page):
    """-> (wall seconds, entries, pages)"""
    cursor, n, pages, t0 = 0, 0, 0, time.perf_counter()
    while True:
        out = C.POINTER(L.gk_violations_out)()
        eng._check(eng.lib.gk_resident_violations(eng.handle, cursor, page, 0, C.byref(out)))
        o = out.contents
        n, pages = n + o.n_entries, pages + 1
        cursor, total = int(o.next_cursor), int(o.total_objects)
        eng.lib.gk_violations_free(out)
        if not cursor:
            assert n == total, (n, total)
            return time.perf_counter() - t0, n, pages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=1000000)
    ap.add_argument("--churn", type=float, default=0.001)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--page", type=int, default=65536)
    ap.add_argument("--hostemu", action="store_true")
    args = ap.parse_args()
    from gatekeeper_amd import _lib as L
    from gatekeeper_amd import driver as D
    from gatekeeper_amd import synth
    os.environ["GK_JIT_STRICT"] = "1"
    c = D.Client(D.Driver(hostemu=True) if args.hostemu else D.Driver(device=0, hostemu=False))
    for t in synth.psp_templates(synth.load_fixtures()):
        c.AddTemplate(t)
    for k in synth.audit_constraints():   # configs[2]
        c.AddConstraint(k)
    eng, n = c.driver.engine, args.objects
    nss = synth.gen_namespaces()
    t0 = time.perf_counter()
    batch = synth.NativeBatch(eng.lib, n, seed=23, mixed=True, namespaces=nss)
    texts, paths = [], []
    for i in range(n):
        text = C.string_at(batch.reviews[i].json, batch.reviews[i].json_len)
        texts.append(text)
        paths.append(D.process_data(json.loads(text)))
        put_text(eng, paths[-1], text)
    for ns in nss.values():
        c.driver.AddData(D.TARGET_NAME, D.process_data(ns), dict(ns))
    print("put %d objects + %d Namespaces: %.1f s" % (n, len(nss), time.perf_counter() - t0), flush=True)
    t0 = time.perf_counter()
    sweep = c.driver.ResidentSweep()
    print("first sweep: %.2f s, %d chunk(s), %d violating pairs" % (time.perf_counter() - t0, sweep["n_chunks"], sum(sweep["pairs"].values())), flush=True)
    wall, dev, entries, pages, reset, held = changes_stream(eng, L, args.page)
    print("baseline stream: %.3f ms wall, %.3f ms device, %d entries on %d pages, reset %d, baseline holds %d bytes" % (wall * 1e3, dev, entries, pages, reset, held), flush=True)
    every = max(1, int(round(1.0 / args.churn)))
    rows = []
    for run in range(args.runs + 1):   # (run 0 warms up)
        replaced = 0
        for i in range(run % every, n, every):
            o = json.loads(texts[i])
            md = o.setdefault("metadata", {})
            md.setdefault("labels", {})["probe-run"] = "r%d" % run
            if o.get("kind") == "Pod" and isinstance(o.get("spec"), dict):
                o["spec"]["hostNetwork"] = not o["spec"].get("hostNetwork", False)
            text = json.dumps(o).encode()
            texts[i] = text
            put_text(eng, paths[i], text)
            replaced += 1
        t0 = time.perf_counter()
        sweep = c.driver.ResidentSweep()
        sweep_s = time.perf_counter() - t0
        cw, cd, ce, cp, creset, held = changes_stream(eng, L, args.page)
        vw, ve, vp = violations_stream(eng, L, args.page)
        rows.append({"replaced": replaced, "sweep_ms": sweep_s * 1e3, "chunks": sweep["n_chunks"], "changes_wall_ms": cw * 1e3, "changes_device_ms": cd, "changes_entries": ce,
                     "changes_pages": cp, "reset": creset, "violations_wall_ms": vw * 1e3, "violations_entries": ve, "violations_pages": vp, "baseline_bytes": held})
        print("run %d%s: %s" % (run, " (warm-up)" if run == 0 else "", json.dumps(rows[-1])), flush=True)
    kept = rows[1:]
    print(json.dumps({"objects": n, "constraints": len(sweep["pairs"]), "churn": args.churn, "runs": len(kept), "page": args.page, "hostemu": args.hostemu,
                      "changes_wall_ms_median": median([r["changes_wall_ms"] for r in kept]), "changes_device_ms_median": median([r["changes_device_ms"] for r in kept]),
                      "violations_wall_ms_median": median([r["violations_wall_ms"] for r in kept]), "changes_entries": [r["changes_entries"] for r in kept],
                      "violations_entries": [r["violations_entries"] for r in kept], "resets": sum(r["reset"] for r in kept), "baseline_bytes": kept[-1]["baseline_bytes"]}))


if __name__ == "__main__":
    main()
