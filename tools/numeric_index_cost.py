#!/usr/bin/env python3
"""Cost of an indexed access on the device (profiles/numeric_index.md): configs[2]'s policy set plus ONE template that tests a member of
`containers[0]` (--form indexed) or of `containers[_]` (--form iterated; --form none: configs[2] alone), over a resident table of
configs[2]'s synthetic stream -- the resident-sweep recipe of profiles/self_join_cost.md: 3 warm-up sweeps, then 50 timed sweeps between
two synchronisations.  Prints one JSON line.  One process per run: alternate the forms from the shell.

--root DIR imports the package from another checkout's tree (a build of the parent commit, for the baseline)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--form", choices=["indexed", "iterated", "none"], required=True)
ap.add_argument("--reviews", type=int, default=1 << 20)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--hostemu", action="store_true", help="the GPU-less test build (to try the script; not a measurement)")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

from gatekeeper_amd import driver as D   # noqa: E402
from gatekeeper_amd import synth         # noqa: E402

REGO = '''package k8sfirstimage
violation[{"msg": msg}] {
  c := input.review.object.spec.containers[%s]
  endswith(c.image, ":latest")
  msg := sprintf("container %%v runs a floating tag", [c.name])
}
'''


def main():
    fx = synth.load_fixtures()
    drv = D.Driver(device=0, hostemu=args.hostemu)
    client = D.Client(drv)
    for t in synth.psp_templates(fx):
        client.AddTemplate(t)
    for k in synth.audit_constraints():
        client.AddConstraint(k)
    if args.form != "none":
        client.AddTemplate({"apiVersion": "templates.gatekeeper.sh/v1", "kind": "ConstraintTemplate", "metadata": {"name": "k8sfirstimage"},
                            "spec": {"crd": {"spec": {"names": {"kind": "K8sFirstImage"}}},
                                     "targets": [{"target": "admission.k8s.gatekeeper.sh", "rego": REGO % ("0" if args.form == "indexed" else "_")}]}})
        client.AddConstraint({"apiVersion": "constraints.gatekeeper.sh/v1beta1", "kind": "K8sFirstImage", "metadata": {"name": "first-image"}, "spec": {}})
    n = args.reviews
    batch = synth.NativeBatch(drv.engine.lib, n, seed=synth.SEED, mixed=True, start=0, namespaces=synth.gen_namespaces())
    table = drv.engine.create_table_native(batch.reviews, n, keep_docs=False, resident=True, pruned=True)

    def sync():
        if not args.hostemu:
            import torch
            torch.cuda.synchronize()

    def sweeps(k, **kw):
        for _ in range(k):
            table.launch(**kw)
        return table.eval(download=False, collect_only=True)
    sweeps(args.warmup)
    sync()
    t0 = time.perf_counter()
    sweeps(args.steps)
    sync()
    dt = time.perf_counter() - t0
    kern = sweeps(min(args.steps, 20), kernel_only=True)
    table.launch()
    final = table.eval(download=True, collect_only=True)
    pairs = sum(1 for _ in final.pairs("viol"))
    print(json.dumps({"form": args.form, "root": os.path.abspath(args.root), "reviews": n, "steps": args.steps, "ms_per_sweep": dt / args.steps * 1e3,
                      "kernel_ms": kern.fast_kernel_ms, "plan_groups": int(final.n_plan_groups), "violating_pairs": pairs}))
    table.free()


if __name__ == "__main__":
    main()
