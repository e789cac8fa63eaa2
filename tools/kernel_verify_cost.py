"""What gk_table_verify costs (profiles/kernel_verify.md), on one GPU: configs[2]'s policy set (50 audit constraints) over N synthetic objects.

  python tools/kernel_verify_cost.py --objects 1000000 [--host-alternative] [--repeat 5] [--out FILE]

Measured, each `--repeat` times after one warm-up call (the warm-up pays hiprtc and the chunk lists):
  * a plain gk_table_eval without download: wall clock and the device time it reports (kernel_ms);
  * gk_table_verify: wall clock, and specialised_ms / bytecode_ms / diff_ms as the call reports them (HIP events);
  * with --host-alternative, what a caller had to do before: a second engine under GK_NO_JIT=1 with a second table of the same objects,
    both evaluations downloaded ([C][N/64] words each, viol and err), XOR and popcount on the host (numpy).  The flattening of the second
    table is reported once; it is the larger part of the price and is not repeated.
Every wall time is a host clock around a C call that ends in a stream synchronise.  Reads nothing outside the tree; objects come from the
seeded synthetic stream.  --hostemu rehearses the script on the CPU stand-in; its times mean nothing."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def new_client(hostemu, interp=False):
    from gatekeeper_amd import driver as D
    from gatekeeper_amd import synth
    for k in ("GK_NO_JIT", "GK_JIT_STRICT", "GK_HOSTEMU_JIT"):
        os.environ.pop(k, None)
    if interp:
        os.environ["GK_NO_JIT"] = "1"        # (read when a plan is uploaded: the table below is evaluated once before the variable goes)
    elif hostemu:
        os.environ["GK_HOSTEMU_JIT"] = "1"
    else:
        os.environ["GK_JIT_STRICT"] = "1"
    c = D.Client(D.Driver(hostemu=True) if hostemu else D.Driver(device=0, hostemu=False))
    for t in synth.psp_templates(synth.load_fixtures()):
        c.AddTemplate(t)
    for k in synth.audit_constraints():   # configs[2]
        c.AddConstraint(k)
    return c


def make_table(c, n):
    from gatekeeper_amd import synth
    t0 = time.perf_counter()
    batch = synth.NativeBatch(c.driver.engine.lib, n, seed=synth.SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
    t1 = time.perf_counter()
    table = c.driver.engine.create_table_native(batch.reviews, n, resident=True)
    return table, batch, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-alternative", action="store_true")
    ap.add_argument("--hostemu", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    res = {"objects": args.objects, "constraints": 50, "repeat": args.repeat}

    c = new_client(args.hostemu)
    table, batch, gen_s, flatten_s = make_table(c, args.objects)
    res["generate_s"], res["flatten_upload_s"] = round(gen_s, 3), round(flatten_s, 3)
    ev = table.eval(download=False)   # warm-up: the specialised build
    res["kernel_text_hash"] = "%016x" % ev.kernel_text_hash
    wall, dev = [], []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        ev = table.eval(download=False)
        wall.append(time.perf_counter() - t0)
        dev.append(ev.kernel_ms)
    res["eval_wall_ms"], res["eval_kernel_ms"] = round(med(wall) * 1e3, 4), round(med(dev), 4)

    v = c.driver.VerifyTable(table)   # warm-up: the verification view, the bytecode kernel's chunk lists
    res["verify_first_call"] = {"ok": v.ok, "specialised_groups": v.specialised_groups, "n_plan_groups": v.n_plan_groups, "diff_total": v.diff_total,
                                "entries": [[e.kind, e.constraint_kind, e.constraint_name, e.review, e.specialised_bit] for e in v.entries]}
    wall, a_ms, b_ms, d_ms = [], [], [], []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        v = c.driver.VerifyTable(table)
        wall.append(time.perf_counter() - t0)
        a_ms.append(v.specialised_ms), b_ms.append(v.bytecode_ms), d_ms.append(v.diff_ms)
    res["verify_wall_ms"] = round(med(wall) * 1e3, 4)
    res["specialised_ms"], res["bytecode_ms"], res["diff_ms"] = round(med(a_ms), 4), round(med(b_ms), 4), round(med(d_ms), 4)
    res["verify_ok"], res["diff_total"] = v.ok, v.diff_total
    res["verify_costs_sweeps"] = round((med(a_ms) + med(b_ms) + med(d_ms)) / max(res["eval_kernel_ms"], 1e-9), 2)
    vm = c.driver.VerifyTable(table, want_match=True)
    res["with_match"] = {"ok": vm.ok, "specialised_ms": round(vm.specialised_ms, 4), "bytecode_ms": round(vm.bytecode_ms, 4), "diff_ms": round(vm.diff_ms, 4)}

    if args.host_alternative:
        c2 = new_client(args.hostemu, interp=True)
        table2, batch2, gen2_s, flatten2_s = make_table(c2, args.objects)
        e2 = table2.eval(host_eval=False)   # (uploads the plan under GK_NO_JIT)
        os.environ.pop("GK_NO_JIT", None)
        assert e2.kernel_text_hash == 0
        res["host_second_table_s"] = round(gen2_s + flatten2_s, 3)
        dl, xor = [], []
        diff = -1
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            e1 = table.eval(host_eval=False)
            e2 = table2.eval(host_eval=False)
            t1 = time.perf_counter()
            care = ~(e1.too_big | e2.too_big)
            x = ((e1.viol ^ e2.viol) & care, (e1.err ^ e2.err) & care)
            diff = sum(int(np.unpackbits(a.view(np.uint8)).sum()) for a in x)   # (bits beyond n are zero on both sides of a download)
            xor.append(time.perf_counter() - t1)
            dl.append(t1 - t0)
        res["host_two_evals_downloaded_ms"], res["host_xor_popcount_ms"], res["host_diff_total"] = round(med(dl) * 1e3, 3), round(med(xor) * 1e3, 3), diff
        res["host_bitmap_bytes_downloaded"] = int(2 * 2 * e1.viol.nbytes)
        table2.free()
    table.free()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
