"""What gk_resident_violations costs (profiles/resident_violations.md), on one GPU.

  python tools/resident_violations_cost.py all --out DIR      every step below as a child process of its own, each under its own time limit
  python tools/resident_violations_cost.py stream --objects N (a) the whole stream without rendering, pages of 65 536, against the plain host loop
                                                              over downloaded bitmaps (tools/resident_violations_host.cpp, built here with g++)
  python tools/resident_violations_cost.py client --objects N (b) Client.AuditStreamFromCache against Client.AuditFromCache; rendering at 1..16 host threads
                                                              (`all` runs (a) once more under rocprofv3 --kernel-trace --stats: the kernels' device times)

Every wall time is a host clock around a C call that ends in a stream synchronise (or around a Python call made of such calls).  Every
comparison is taken twice in one process, alternating.  Reads nothing outside the tree; objects come from the seeded synthetic stream."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = sorted(xs)
    return "%.3f / %.3f / %.3f ms" % (xs[0] * 1e3, xs[len(xs) // 2] * 1e3, xs[-1] * 1e3)


HOSTEMU = False   # --hostemu: the CPU stand-in, to rehearse the script; its times mean nothing


def new_client():
    from gatekeeper_amd import driver as D
    from gatekeeper_amd import synth
    os.environ["GK_JIT_STRICT"] = "1"
    c = D.Client(D.Driver(hostemu=True) if HOSTEMU else D.Driver(device=0, hostemu=False))
    for t in synth.psp_templates(synth.load_fixtures()):
        c.AddTemplate(t)
    for k in synth.audit_constraints():   # configs[2]
        c.AddConstraint(k)
    return c


def raw_stream(eng, L, max_objects, flags, keep=False):
    """the whole stream through the C ABI -> (seconds per call, entries, pages, [(viol, err) arrays per page] when keep)"""
    import numpy as np
    times, n, kept, cursor = [], 0, [], 0
    while True:
        out = C.POINTER(L.gk_violations_out)()
        t0 = time.perf_counter()
        rc = eng.lib.gk_resident_violations(eng.handle, cursor, max_objects, flags, C.byref(out))
        times.append(time.perf_counter() - t0)
        eng._check(rc)
        o = out.contents
        n += o.n_entries
        if keep and o.n_entries:
            shape = (o.n_entries, o.mask_words)
            kept.append((np.ctypeslib.as_array(o.viol, shape).copy(), np.ctypeslib.as_array(o.err, shape).copy()))
        cursor, total = int(o.next_cursor), int(o.total_objects)
        eng.lib.gk_violations_free(out)
        if not cursor:
            assert n == total, (n, total)
            return times, n, len(times), kept


def build_host_loop():
    so = os.path.join(tempfile.mkdtemp(prefix="gkviol"), "host_loop.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "resident_violations_host.cpp")], check=True)
    lib = C.CDLL(so)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    lib.host_viol_entries.argtypes = [u64p, u64p, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u32p, u64p, u64p]
    lib.host_viol_entries.restype = C.c_uint64
    return lib


def step_stream(args):
    import numpy as np
    from gatekeeper_amd import _lib as L
    from gatekeeper_amd import driver as D
    from gatekeeper_amd import synth
    c = new_client()
    eng = c.driver.engine
    nss = synth.gen_namespaces()
    n = args.objects
    t0 = time.perf_counter()
    batch = synth.NativeBatch(eng.lib, n, seed=23, mixed=True, namespaces=nss)
    reviews = batch.reviews
    for i in range(n):   # slots 0 .. n-1: the stream's objects; the Namespaces follow (a review's Namespace is looked up at sweep time)
        text = C.string_at(reviews[i].json, reviews[i].json_len)
        put_text(eng, D.process_data(json.loads(text)), text)
    for ns in nss.values():
        c.driver.AddData(D.TARGET_NAME, D.process_data(ns), dict(ns))
    print("put %d objects + %d Namespaces: %.1f s" % (n, len(nss), time.perf_counter() - t0), flush=True)
    t0 = time.perf_counter()
    sweep = c.driver.ResidentSweep()
    print("first sweep: %.2f s, %d chunk(s), %d violating pairs, %d beyond the limits" % (time.perf_counter() - t0, sweep["n_chunks"], sum(sweep["pairs"].values()), sweep["beyond_limits"]), flush=True)
    # ---- the host alternative: a table of the same reviews (no Source, as the resident set reviews them), its downloaded bitmaps
    arr = (L.gk_review_in * n)()
    C.memmove(arr, reviews, C.sizeof(L.gk_review_in) * n)
    for i in range(n):
        arr[i].source = L.GK_SRC_EMPTY
    table = eng.create_table_native(arr, n, resident=True, pruned=True)
    ev = table.eval()
    nc, nt = ev.n_constraints, ev.n_tiles
    mw = (nc + 63) // 64
    viol, err = np.ascontiguousarray(ev.viol), np.ascontiguousarray(ev.err)
    shown = np.full(nt, 0xFFFFFFFFFFFFFFFF, np.uint64)
    host = build_host_loop()
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)

    def host_loop():
        cap = n
        rev, hv, he = np.zeros(cap, np.uint32), np.zeros((cap, mw), np.uint64), np.zeros((cap, mw), np.uint64)
        t0 = time.perf_counter()
        k = host.host_viol_entries(viol.ctypes.data_as(u64p), err.ctypes.data_as(u64p), shown.ctypes.data_as(u64p), nc, nt, n, cap,
                                   rev.ctypes.data_as(u32p), hv.ctypes.data_as(u64p), he.ctypes.data_as(u64p))
        return time.perf_counter() - t0, int(k), hv[:k], he[:k]

    # ---- first call (index build), then steady state; twice, alternating with the host loop
    first, n_entries, n_pages, _ = raw_stream(eng, L, 65536, 0)
    print("first stream: first call %.3f ms (index build), %d entries on %d pages, all calls %.3f ms" % (first[0] * 1e3, n_entries, n_pages, sum(first) * 1e3))
    for rnd in (1, 2):
        whole, first_call, later, hostt = [], [], [], []
        for _ in range(args.repeat):
            times, k, pages, _ = raw_stream(eng, L, 65536, 0)
            whole.append(sum(times)); first_call.append(times[0]); later += times[1:]
            ht, hk, _, _ = host_loop()
            hostt.append(ht)
        print("round %d: whole stream (%d pages, min / median / max) %s | cursor-0 call %s | later pages %s | host loop over downloaded bitmaps %s"
              % (rnd, pages, stats(whole), stats(first_call), stats(later) if later else "-", stats(hostt)))
    # ---- the same entries?  slots 0 .. n-1 are the table's reviews; the Namespaces' entries (if any) come last in the stream
    _, k, _, kept = raw_stream(eng, L, 65536, 0, keep=True)
    sv = np.concatenate([a for a, _ in kept]) if kept else np.zeros((0, mw), np.uint64)
    se = np.concatenate([b for _, b in kept]) if kept else np.zeros((0, mw), np.uint64)
    _, hk, hv, he = host_loop()
    same = hk <= k and bool((sv[:hk] == hv).all()) and bool((se[:hk] == he).all())
    print("entries: stream %d, host loop over the table of the %d objects %d (the stream's further %d are Namespaces); masks of the common prefix equal: %s" % (k, n, hk, k - hk, same))
    dev_entries = int((sv != 0).any(axis=1).sum())
    merged = bool((se != 0).any())
    pw = (n + len(nss) + 63) // 64
    print("bytes downloaded (computed from the shapes): index %d (cnt, 4 B x %d words%s); entries %d (%d device entries x (4 + 8 x %d) B + 8 B per page)"
          % (pw * 4 + (pw * 8 if merged else 0), pw, " + any, 8 B x words: autoreject bits present" if merged else "", dev_entries * (4 + 8 * mw) + 8 * n_pages, dev_entries, mw))
    print("the sweep's own download of the bitmaps: %d bytes per evaluation (viol + err, %d rows x %d words)" % (2 * nc * nt * 8, nc, nt))
    table.free()


def put_text(eng, path, text):
    arr = (C.c_char_p * len(path))(*[p.encode() for p in path])
    eng._check(eng.lib.gk_data_put(eng.handle, arr, len(path), text, len(text)))


def step_client(args):
    from gatekeeper_amd import _lib as L
    from gatekeeper_amd import synth
    c = new_client()
    eng = c.driver.engine
    t0 = time.perf_counter()
    for o in list(synth.gen_namespaces().values()) + synth.gen_objects(args.objects, seed=23, mixed=True):
        c.AddData(o)
    print("put %d objects: %.1f s" % (len(c.cached), time.perf_counter() - t0), flush=True)
    c.driver.ResidentSweep()
    for rnd in (1, 2):
        t0 = time.perf_counter()
        got = list(c.AuditStreamFromCache(page=4096))
        t1 = time.perf_counter()
        full, _ = c.AuditFromCache()
        t2 = time.perf_counter()
        print("round %d: AuditStreamFromCache %.3f s (%d objects rendered, %d results) | AuditFromCache %.3f s (%d gk_resident_review calls, %d results)"
              % (rnd, t1 - t0, len(got), sum(len(r) for _, r in got), t2 - t1, len(full), sum(len(r) for r in full.values() if isinstance(r, list))))
    # where the stream's time goes: the C calls with and without rendering, at 1 .. 16 host threads (twice, alternating)
    for rnd in (1, 2):
        line = []
        for threads in (1, 2, 4, 8, 16):
            os.environ["GK_HOST_THREADS"] = str(threads)
            tr, k, pages, _ = raw_stream(eng, L, 4096, L.GK_VIOLATIONS_RENDER)
            tn, _, _, _ = raw_stream(eng, L, 4096, 0)
            line.append("%d threads: render %.3f s, no render %.4f s" % (threads, sum(tr), sum(tn)))
        os.environ.pop("GK_HOST_THREADS", None)
        print("round %d: C calls only, %d entries on %d pages | %s" % (rnd, k, pages, " | ".join(line)))


def step_all(args):
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    steps = [("stream", me + ["stream", "--objects", str(args.objects)], 900),
             ("client", me + ["client", "--objects", str(args.client_objects)], 600),
             ("trace", ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(args.out, "trace"), "--"] + me + ["stream", "--objects", str(args.objects), "--repeat", "3"], 900)]
    for name, cmd, limit in steps:   # a fresh child per step, each under its own limit; a step that fails or runs out ends the run
        with open(os.path.join(args.out, name + ".log"), "w") as log:
            rc = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=limit).returncode
        print("%s: exit status %d" % (name, rc), flush=True)
        if rc != 0:
            sys.exit(rc)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["all", "stream", "client"])
    ap.add_argument("--objects", type=int, default=1000000)
    ap.add_argument("--client-objects", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default="resident_violations_out")
    ap.add_argument("--hostemu", action="store_true")
    a = ap.parse_args()
    HOSTEMU = a.hostemu
    {"all": step_all, "stream": step_stream, "client": step_client}[a.step](a)
