"""The cold-arguments text on the device (csrc/cold_args.hip): the per-item tail and the epilogue of the plan-specialised
sweep kernel read their launch arguments from the kernel-argument segment.  tests/cold_args_util.py runs every case in one process per
setting (the switches are read once per process) with GK_JIT_COLD_ARGS_MIN=1 and 256-review groups: the variant, GK_JIT_COLD_ARGS=0 -- the
parent's text -- and the variant with GK_FUSED_TOTALS=0.  Every result is compared bit for bit with the switch off, verified against the
bytecode kernel on the device (gk_table_verify inside the helper), and every shape is checked against the Python oracle (parity_util.assert_parity
in the variant's process)."""
import functools
import json
import os
import subprocess
import sys

import pytest

import cold_args_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run(env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("GK_JIT_COLD_ARGS", "GK_REVIEW_WORDS", "GK_RPT", "GK_FORCE_RPP", "GK_NO_JIT", "GK_JIT_REVIEW_WORDS", "GK_FUSED_TOTALS"))}
    e.update({"GK_JIT_COLD_ARGS_MIN": "1", "GK_REVIEW_WORDS_MIN": "0", "GK_RPT": "256", "GK_JIT_STRICT": "1"})
    e.update(dict(env))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cold_args_util.py")], capture_output=True, text=True, env=e, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().split("\n")[-1])


def on():
    return run(())


def off():
    return run((("GK_JIT_COLD_ARGS", "0"),))


def assert_verified(r):
    assert r["verify_ok"] and r["specialised_groups"] > 0 and r["specialised_groups"] == r["n_plan_groups"] and r["diff_total"] == 0 and r["diff_too_big"] == 0
    assert r["again"] == r["words"]


def same_words_other_text(name):
    a, b = on()[name], off()[name]
    assert a["hash"] != b["hash"], "the variant was not on: the same kernel text ran"
    assert a["words"] == b["words"] and a["pairs"] == b["pairs"] and a["overflow"] == b["overflow"]
    assert_verified(a)
    assert_verified(b)
    # the Python oracle on the shape (parity_util.assert_parity in the variant's process: rendered results and raw bitmaps), by the variant text
    if "oracle" in a:   # (every shape but the second and third table of one engine, which are shapes of the first)
        assert a["oracle"]["hash"] not in (b["hash"], "0000000000000000") and (a["oracle"]["results"] > 0 or name == "reviews_1")
    return a


@pytest.mark.parametrize("n", CU.REVIEWS)
def test_reviews(n):
    """a partial last word and a partial last group: bitmap words beyond n_tiles are not written"""
    r = same_words_other_text("reviews_%d" % n)
    assert r["pairs"] > 0 or n == 1   # (the one object of the smallest table violates nothing)


@pytest.mark.parametrize("k", CU.CONSTRAINTS)
def test_constraints(k):
    """the batch loop of the output stage: the second and later batches of 64 constraints read `slots` through the segment"""
    assert same_words_other_text("constraints_%d" % k)["pairs"] > 0


def test_want_match_off_on_off():
    a, b = on()["want_match_sequence"], off()["want_match_sequence"]
    assert [s["plain"] for s in a] == [s["plain"] for s in b] and len({s["plain"] for s in a}) == 1
    assert a[2]["match"] == b[2]["match"] is not None
    assert all(x["hash"] != y["hash"] for x, y in zip(a, b))
    assert all(x["verified"] for x in a + b)   # (gk_table_verify with the null and with the non-null `match`)


@pytest.mark.parametrize("k", [1, 64, 65])
def test_launches_before_one_collecting_call(k):
    a, b = on()["launches_%d" % k], off()["launches_%d" % k]
    assert a["plain"] == b["plain"] == on()["want_match_sequence"][0]["plain"] and a["hash"] != b["hash"]
    assert a["n_launches"] == b["n_launches"] == k and a["verified"] and b["verified"]


def test_pair_list():
    """`list`, `list_count[0]` and `list_capacity` through the segment: the entries are the bits of the violation words"""
    a, b = on()["pair_list"], off()["pair_list"]
    assert a["pairs"] == b["pairs"] and a["n"] == b["n"] == a["list_total"] > 0 and a["equals_bitmap"] and b["equals_bitmap"]
    assert a["plain"] == b["plain"] and a["hash"] != b["hash"] and a["verified"] and b["verified"]


def test_two_tables_on_one_engine():
    for name in ("two_tables_a", "two_tables_b", "two_tables_a_again"):
        same_words_other_text(name)
    assert on()["two_tables_a"]["words"] == on()["two_tables_a_again"]["words"] == on()["reviews_513"]["words"]


def test_overflowed_reviews():
    """squeezed element capacities (2, 4, 2, as tests/test_step_overhead.py): `overflow`, `too_big` and the overflowed-review count"""
    assert same_words_other_text("overflowed")["overflow"] > 0


def test_plan_without_hoisted_classes():
    assert same_words_other_text("no_hoisted_class")["pairs"] > 0


def test_totals_rows_against_the_popcount_kernel():
    """the words hash the per-constraint totals: the epilogue's rows (through the segment's `partial`) against GK_FUSED_TOTALS=0"""
    a, c = on(), run((("GK_FUSED_TOTALS", "0"),))
    for name in ["reviews_%d" % n for n in CU.REVIEWS] + ["constraints_%d" % k for k in CU.CONSTRAINTS] + ["overflowed"]:
        assert a[name]["words"] == c[name]["words"], name
