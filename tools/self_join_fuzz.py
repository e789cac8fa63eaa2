#!/usr/bin/env python3
"""Differential campaign of self-join bodies: tests/test_self_join_fuzz.py's generator over a range of seeds (product through the
C ABI vs the oracle, rendered results and raw device bitmaps).  Prints only what is not clean, then one summary line.

  python tools/self_join_fuzz.py FIRST LAST [--templates 6] [--objects 24] [--backend hostemu|hostemu-gen|gpu|gpu-interp]

A failing seed is reproduced by `run(backend, seed, templates, objects)` of the test module."""
import argparse
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("first", type=int)
    ap.add_argument("last", type=int)
    ap.add_argument("--templates", type=int, default=6)
    ap.add_argument("--objects", type=int, default=24)
    ap.add_argument("--backend", default="hostemu-gen", choices=["hostemu", "hostemu-gen", "gpu", "gpu-interp"])
    a = ap.parse_args()
    import test_self_join_fuzz as F
    t0 = time.time()
    bad, templates, violations = [], 0, 0
    for seed in range(a.first, a.last + 1):
        try:
            n, v = F.run(a.backend, seed, a.templates, a.objects)
            templates += n
            violations += v
        except Exception:   # (a difference, a refusal or an engine error: all count as a failing seed)
            bad.append(seed)
            print("=== seed %d\n%s" % (seed, traceback.format_exc(limit=3)))
    print("self-join fuzz %s seeds %d..%d: %d templates, %d violations compared, %d failing seeds %s (%.0f s)"
          % (a.backend, a.first, a.last, templates, violations, len(bad), bad, time.time() - t0))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
