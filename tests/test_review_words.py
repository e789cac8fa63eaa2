"""Review words on the device (csrc/review_words.hpp): the binding evaluates the plan's all-global predicate classes
once into rwords[K][n_pad], the plan-specialised kernel's lists leave those classes out and the kernel ORs the words of a review into its
accumulators.  Every case runs tests/review_words_util.py in a process of its own (the switches are read once per process) with
GK_REVIEW_WORDS_MIN=0, once with the feature on and once with GK_REVIEW_WORDS=0 -- the parent's text and lists -- and compares the result
words; gk_table_verify inside the helper compares the new path with the bytecode kernel, which keeps the full lists, on the device."""
import functools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def helper(args, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("GK_REVIEW_WORDS", "GK_RPT", "GK_FORCE_RPP", "GK_NO_JIT", "GK_JIT_REVIEW_WORDS"))}
    e.update({"GK_REVIEW_WORDS": "1", "GK_REVIEW_WORDS_MIN": "0", "GK_JIT_STRICT": "1"})
    e.update(dict(env))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "review_words_util.py")] + list(args), capture_output=True, text=True, env=e, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().split("\n")[-1])


def on_off(args, **env):
    env = tuple(sorted((k, str(v)) for k, v in env.items()))
    return helper(tuple(args), env), helper(tuple(args), env + (("GK_REVIEW_WORDS", "0"),))


def assert_verified(r):
    assert r["verify_ok"] and r["specialised_groups"] > 0 and r["specialised_groups"] == r["n_plan_groups"] and r["diff_total"] == 0 and r["diff_too_big"] == 0
    assert r["again"] == r["words"]


@pytest.mark.parametrize("rpt,n", [(256, 600), (128, 300)])
def test_bench_policy_words_equal_with_and_without(rpt, n):
    """configs[2]: three 256-review groups, the last one partial / three 128-review groups; violation, autoreject and match words"""
    on, off = on_off(["table", "configs2", str(n)], GK_RPT=rpt)
    assert on["words"] == off["words"] and on["pairs"] == off["pairs"] > 0
    assert on["hash"] != off["hash"], "the feature was not on: the same kernel text ran"
    assert on["n_rows_read"] < off["n_rows_read"] and on["algo_bytes"] < off["algo_bytes"]
    assert_verified(on)
    assert_verified(off)


@pytest.mark.parametrize("rpt,n", [(256, 600), (128, 300)])
def test_bench_policy_against_the_python_oracle(rpt, n):
    """parity_util.assert_parity with the feature on, and with it off; a table created as assert_parity creates its own is evaluated by the
    variant text (another hash, fewer rows streamed) in the first run and not in the second"""
    on, off = on_off(["oracle", "configs2", str(n)], GK_RPT=rpt)
    assert on["results"] == off["results"] > 0 and on["refused"] == off["refused"] and on["pairs"] == off["pairs"]
    assert on["hash"] != off["hash"] and "0000000000000000" not in (on["hash"], off["hash"])
    assert on["n_rows_read"] < off["n_rows_read"]


def test_switch_off_is_the_text_nobody_asked_the_variant_of():
    """GK_REVIEW_WORDS=0 against the same 600-object table under the default size threshold (8192: too small for the feature): the same
    kernel text, the same rows streamed, the same figures -- the plain text (tests/test_review_words_text.py, tests/test_plan_text_pins.py)
    and the full lists"""
    on, off = on_off(["table", "configs2", "600"], GK_RPT=256)
    small = helper(("table", "configs2", "600"), (("GK_REVIEW_WORDS_MIN", "8192"), ("GK_RPT", "256")))
    assert off == small and off["hash"] != on["hash"]


def test_multi_pass():
    """GK_FORCE_RPP=64: four passes per 256-review group, every pass takes the words of its reviews"""
    on, off = on_off(["table", "configs2", "600"], GK_RPT=256, GK_FORCE_RPP=64)
    one_pass, _ = on_off(["table", "configs2", "600"], GK_RPT=256)
    assert on["words"] == off["words"] == one_pass["words"] and on["hash"] != off["hash"]
    assert_verified(on)


def test_every_class_hoisted():
    """required labels: review-level tests only -- the sweep's lists hold no chunk at all"""
    on, off = on_off(["table", "labels", "600"], GK_RPT=256)
    assert on["words"] == off["words"] and on["pairs"] == off["pairs"] > 0
    assert on["n_rows_read"] == 0 < off["n_rows_read"] and on["hash"] != off["hash"]
    assert_verified(on)


def test_no_class_hoisted():
    """nothing for the binding pass: the parent's build, text and figures"""
    on, off = on_off(["table", "none", "600"], GK_RPT=256)
    assert on == off and on["pairs"] > 0
    assert_verified(on)


def test_reviews_on_the_big_path():
    """squeezed element capacities (2, 4, 2, as tests/test_step_overhead.py): reviews with more elements overflow the LDS accumulators and are
    evaluated again by the big variant, which keeps the full binding"""
    on, off = on_off(["table", "configs2", "600", "2,4,2"], GK_RPT=256)
    assert on["overflow"] == off["overflow"] > 0
    assert on["words"] == off["words"] and on["hash"] != off["hash"]
    assert_verified(on)


def test_warm_tables():
    """two tables on one engine; a constraint added under the warm tables (new plan, new binding, rebuilt words) and removed again; a
    sharded sweep at world size 1 between plain sweeps"""
    on, off = on_off(["warm"], GK_RPT=256)
    for r in (on, off):
        assert r["sharded_totals_equal"] and r["plain_equal_after_shard"]
        for k in ("a0", "b0", "a1", "b1", "a2"):
            assert_verified(r[k])
        assert r["a2"]["words"] == r["a0"]["words"] and r["a1"]["words"] != r["a0"]["words"]
    assert on["words_after_shard"] == off["words_after_shard"]
    for k in ("a0", "b0", "a1", "b1", "a2"):
        assert on[k]["words"] == off[k]["words"] and on[k]["hash"] != off[k]["hash"] and on[k]["n_rows_read"] < off[k]["n_rows_read"]


@pytest.mark.parametrize("seeds", [(12300, 12301), (12302, 12303), (12304, 12305), (12306, 12307)])
def test_template_fuzz_at_sweep_geometry(seeds):
    """20 templates over 14 objects per seed, ten templates per plan: two plans -- two hiprtc builds -- per seed"""
    r = helper(("fuzz",) + tuple(str(s) for s in seeds), (("GK_RPT", "256"),))
    assert r["loaded"] > 0 and r["compared"] > 0
