"""What gk_table_violations costs against walking downloaded bitmaps on the host (profiles/table_violations.md), on one GPU.

  python tools/table_violations_cost.py all --out DIR        every step below as a child process of its own, each under its own time limit
  python tools/table_violations_cost.py evals --objects N    gk_table_eval alone, with and without download, back to back and behind a pause
  python tools/table_violations_cost.py stream --objects N   (a) gk_table_eval(GK_EVAL_NO_DOWNLOAD) + the whole stream without rendering, pages of 65 536, against
                                                             (b) a downloading gk_table_eval + the plain host loop over viol and err
                                                             (tools/resident_violations_host.cpp, built here with g++); --group-max G: plan groups of at most G
                                                             (`all` runs the step at one plan, at three plan groups, and once more under rocprofv3
                                                             --kernel-trace --stats: the kernels' device times)

Workload: the configs[2] policy set, N synthetic objects (seed 23) in ONE table.  Every wall time is a host clock around C calls that end in a
stream synchronise.  The comparison is taken twice in one process, alternating.  Reads nothing outside the tree."""
import argparse
import ctypes as C
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


def build_host_loop():
    so = os.path.join(tempfile.mkdtemp(prefix="gktviol"), "host_loop.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "resident_violations_host.cpp")], check=True)
    lib = C.CDLL(so)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    lib.host_viol_entries.argtypes = [u64p, u64p, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u32p, u64p, u64p]
    lib.host_viol_entries.restype = C.c_uint64
    return lib


def open_table(args):
    """the workload: -> (L, engine, client, table)"""
    from gatekeeper_amd import _lib as L
    from gatekeeper_amd import driver as D
    from gatekeeper_amd import synth
    os.environ["GK_JIT_STRICT"] = "1"
    lib = L.load(hostemu=args.hostemu)
    if args.group_max:
        assert lib.gk_debug_set(b"group_max", args.group_max) == 0
    c = D.Client(D.Driver(hostemu=True) if args.hostemu else D.Driver(device=0, hostemu=False))
    for t in synth.psp_templates(synth.load_fixtures()):
        c.AddTemplate(t)
    for k in synth.audit_constraints():   # configs[2]
        c.AddConstraint(k)
    eng = c.driver.engine
    n = args.objects
    t0 = time.perf_counter()
    batch = synth.NativeBatch(eng.lib, n, seed=23, mixed=True, namespaces=synth.gen_namespaces())
    table = eng.create_table_native(batch.reviews, n, resident=True, pruned=True)
    print("table of %d objects: %.1f s" % (n, time.perf_counter() - t0), flush=True)
    return L, eng, c, table


def step_evals(args):
    """gk_table_eval alone, no stream between: back to back, and with a pause in front of each (the host loop's 30 ms)"""
    L, eng, _c, table = open_table(args)

    def evaluate(flags, pause):
        out = C.POINTER(L.gk_eval_out)()
        if pause:
            time.sleep(pause)
        t0 = time.perf_counter()
        rc = eng.lib.gk_table_eval(eng.handle, table.handle, flags, C.byref(out))
        dt = time.perf_counter() - t0
        eng._check(rc)
        eng.lib.gk_eval_free(out)
        return dt

    evaluate(0, 0)
    for rnd in (1, 2):
        for name, flags in (("without download", L.GK_EVAL_NO_DOWNLOAD), ("downloading", 0)):
            for pause in (0, 0.03):
                print("round %d: %s, %s (min / median / max): %s" % (rnd, name, "30 ms pause in front of each" if pause else "back to back",
                                                                     stats([evaluate(flags, pause) for _ in range(args.repeat)])), flush=True)
    table.free()


def step_stream(args):
    import numpy as np
    L, eng, _c, table = open_table(args)
    n = args.objects
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    host = build_host_loop()

    def evaluate(flags):
        """one raw gk_table_eval -> (seconds, the out pointer: the caller frees it)"""
        out = C.POINTER(L.gk_eval_out)()
        t0 = time.perf_counter()
        rc = eng.lib.gk_table_eval(eng.handle, table.handle, flags, C.byref(out))
        dt = time.perf_counter() - t0
        eng._check(rc)
        return dt, out

    def stream(keep=False):
        """the whole stream through the C ABI -> (seconds per call, device_ms per call, entries, beyond, kept arrays)"""
        times, dev, k, cursor, kept, beyond = [], [], 0, 0, [], 0
        while True:
            out = C.POINTER(L.gk_table_violations_out)()
            t0 = time.perf_counter()
            rc = eng.lib.gk_table_violations(eng.handle, table.handle, cursor, 65536, 0, C.byref(out))
            times.append(time.perf_counter() - t0)
            eng._check(rc)
            o = out.contents
            dev.append(float(o.device_ms))
            if keep and o.n_entries:
                shape = (o.n_entries, o.mask_words)
                kept.append((np.ctypeslib.as_array(o.reviews, (o.n_entries,)).copy(), np.ctypeslib.as_array(o.viol, shape).copy(), np.ctypeslib.as_array(o.err, shape).copy()))
            k += o.n_entries
            cursor, total, beyond = int(o.next_cursor), int(o.total_entries), int(o.beyond_limits)
            eng.lib.gk_table_violations_free(out)
            if not cursor:
                assert k == total, (k, total)
                return times, dev, k, beyond, kept

    def host_loop(out):
        """the plain loop over the bitmaps the evaluation downloaded -> (seconds, entries, reviews, viol masks, err masks)"""
        o = out.contents
        nc, nt = o.n_constraints, o.n_tiles
        mw = (nc + 63) // 64
        shown = np.full(nt, 0xFFFFFFFFFFFFFFFF, np.uint64)
        rev, hv, he = np.zeros(n, np.uint32), np.zeros((n, mw), np.uint64), np.zeros((n, mw), np.uint64)
        t0 = time.perf_counter()
        k = host.host_viol_entries(o.viol, o.err, shown.ctypes.data_as(u64p), nc, nt, n, n, rev.ctypes.data_as(u32p), hv.ctypes.data_as(u64p), he.ctypes.data_as(u64p))
        return time.perf_counter() - t0, int(k), rev[:k], hv[:k], he[:k]

    # warm-up: the plan-specialised build, the first download, the first index
    dt, out = evaluate(0)
    o = out.contents
    nc, nt, groups, n_host = o.n_constraints, o.n_tiles, o.n_plan_groups, o.n_host_evaluated
    host_done = set(int(o.host_evaluated[i]) for i in range(n_host))
    mw = (nc + 63) // 64
    print("first evaluation %.2f s: %d constraints, %d plan group(s), %d reviews completed on the host" % (dt, nc, groups, n_host), flush=True)
    # ---- the same entries?  after the downloading evaluation the stream must be the host loop's answer exactly
    _, k_h, rev_h, hv, he = host_loop(out)
    _, _, k_s, beyond, kept = stream(keep=True)
    cat = lambda i: np.concatenate([x[i] for x in kept]) if kept else np.zeros((0, mw) if i else 0, np.uint64 if i else np.uint32)   # noqa: E731
    same = k_s == k_h and bool((cat(0) == rev_h).all()) and bool((cat(1) == hv).all()) and bool((cat(2) == he).all())
    print("entries after a downloading evaluation: stream %d, host loop %d, beyond the limits %d; reviews and masks equal: %s" % (k_s, k_h, beyond, same), flush=True)
    eng.lib.gk_eval_free(out)
    _, out = evaluate(L.GK_EVAL_NO_DOWNLOAD)
    eng.lib.gk_eval_free(out)
    _, _, k_n, beyond_n, kept = stream(keep=True)
    keep_h = np.array([int(r) not in host_done for r in rev_h], bool) if host_done else np.ones(len(rev_h), bool)
    same_n = k_n == int(keep_h.sum()) and bool((cat(0) == rev_h[keep_h]).all()) and bool((cat(1) == hv[keep_h]).all()) and bool((cat(2) == he[keep_h]).all())
    print("entries after GK_EVAL_NO_DOWNLOAD: stream %d, beyond the limits %d (the %d host-completed reviews have no entry); the others equal the host loop's: %s"
          % (k_n, beyond_n, n_host, same_n), flush=True)
    if not (same and same_n):
        sys.exit(2)
    # ---- (a) against (b): twice, alternating
    for rnd in (1, 2):
        a_all, a_eval, a_first, a_later, a_dev, b_all, b_eval, b_loop = [], [], [], [], [], [], [], []
        for _ in range(args.repeat):
            dt, out = evaluate(L.GK_EVAL_NO_DOWNLOAD)
            eng.lib.gk_eval_free(out)
            times, dev, _, _, _ = stream()
            a_eval.append(dt); a_all.append(dt + sum(times)); a_first.append(times[0]); a_later += times[1:]; a_dev.append(dev)
            dt, out = evaluate(0)
            ht, _, _, _, _ = host_loop(out)
            eng.lib.gk_eval_free(out)
            b_eval.append(dt); b_loop.append(ht); b_all.append(dt + ht)
        print("round %d (min / median / max): (a) evaluation without download + stream %s [evaluation %s | cursor-0 call %s | later pages %s]"
              % (rnd, stats(a_all), stats(a_eval), stats(a_first), stats(a_later) if a_later else "-"))
        print("round %d (min / median / max): (b) downloading evaluation + host loop %s [evaluation %s | host loop %s]" % (rnd, stats(b_all), stats(b_eval), stats(b_loop)))
        med = sorted(a_dev, key=sum)[len(a_dev) // 2]
        print("round %d: device_ms per call of the median stream (cursor-0 call: index + first page): %s" % (rnd, " ".join("%.3f" % x for x in med)), flush=True)
    pw, pages = (n + 63) // 64, len(times)
    print("bytes brought back per audit (computed from the shapes): (a) index %d (cnt 4 B x %d words + the counter%s) + entries %d (%d x (4 + 16 x %d) B + 8 B per page, %d pages)"
          % (pw * 4 + 8 + (pw * 8 if n_host else 0), pw, "; any 8 B x words: host pairs present" if n_host else "", k_n * (4 + 16 * mw) + 8 * pages, k_n, mw, pages))
    print("                                                         (b) %d (viol + err, %d rows x %d words; + too_big and counts)" % (2 * nc * nt * 8, nc, nt))
    table.free()


def step_all(args):
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    base = ["stream", "--objects", str(args.objects)]
    steps = [("stream", me + base, 360),
             ("stream_groups", me + base + ["--group-max", "17"], 360),
             ("trace", ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(args.out, "trace"), "--"] + me + base + ["--repeat", "3"], 360)]
    for name, cmd, limit in steps:   # a fresh child per step, each under its own limit; a step that fails or runs out ends the run
        with open(os.path.join(args.out, name + ".log"), "w") as log:
            rc = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=limit).returncode
        print("%s: exit status %d" % (name, rc), flush=True)
        if rc != 0:
            sys.exit(rc)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["all", "stream", "evals"])
    ap.add_argument("--objects", type=int, default=1000000)
    ap.add_argument("--group-max", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default="table_violations_out")
    ap.add_argument("--hostemu", action="store_true")
    a = ap.parse_args()
    {"all": step_all, "stream": step_stream, "evals": step_evals}[a.step](a)
