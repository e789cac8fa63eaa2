"""Plain reference of gk_table_topk (Table.topk), for tests/test_table_topk.py.  It reads the bitmaps a downloading
Table.eval() returned and the objects' keys, and shares nothing with the selection code (gk_topk_rows on the device, dev_topk in the CPU
stand-in, table_key_order on the host).

The rule, per bitmap row: the reviews in object-key order -- (group, version, kind, namespace, name) compared field by field as bytes,
equal keys in review-index order --, of these the violators; the list ends in front of the first violator at rank k or beyond whose key
differs from the key of the violator at rank k - 1; the product returns the first `cap` entries of that list and flags a longer one."""
import ctypes as C

import numpy as np

from gatekeeper_amd import _lib as L


def object_key(obj):
    """the audit sort key of an object (pkg/audit/manager.go:118-138 without message and action), as bytes"""
    api = obj.get("apiVersion") if isinstance(obj.get("apiVersion"), str) else ""
    group, _, version = api.rpartition("/")
    md = obj.get("metadata") if isinstance(obj.get("metadata"), dict) else {}
    fields = (group, version, obj.get("kind"), md.get("namespace"), md.get("name"))
    return tuple((f if isinstance(f, str) else "").encode("utf-8") for f in fields)


def violators(ev):
    """[bitmap row][review] -> bool, from the downloaded violation bitmaps of `ev`"""
    n = ev.n_reviews
    if ev.viol is None or ev.viol.size == 0:
        return np.zeros((ev.n_constraints, n), bool)
    return np.unpackbits(np.ascontiguousarray(ev.viol).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def walk(row_bits, keys, k):
    """the whole list of one bitmap row, before the capacity cuts it: row_bits[r] says whether review r violates, keys[r] is its key"""
    walked = []
    for r in sorted(range(len(keys)), key=keys.__getitem__):   # (stable: equal keys stay in review-index order)
        if k == 0:
            break
        if not row_bits[r]:
            continue
        if len(walked) >= k and keys[r] != keys[walked[k - 1]]:
            break
        walked.append(r)
    return walked


def expected(row_bits, keys, k, cap):
    """-> (reviews, overflow) of one bitmap row, as Table.topk(k) returns them"""
    walked = walk(row_bits, keys, k)
    return walked[:cap], len(walked) > cap


def stride(table, k):
    """the list capacity the product itself reports for `k`: gk_topk_out.stride of a raw gk_table_topk"""
    eng = table.engine
    out = C.POINTER(L.gk_topk_out)()
    eng._check(eng.lib.gk_table_topk(eng.handle, table.handle, k, C.byref(out)))
    try:
        return int(out.contents.stride)
    finally:
        eng.lib.gk_topk_free(out)
