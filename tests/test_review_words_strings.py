"""Review words (test_review_words.py) over string ROW predicates: with the review facts' dictionary full, the prefix tests on an annotation
are an all-global class, which the binding pass evaluates once per plan and table (gk_bind_review_words) and the sweep's kernel otherwise.
tests/review_words_strings.py runs in a process of its own, with the feature on and with GK_REVIEW_WORDS=0, as every case of
test_review_words.py runs its helper."""
import json
import os
import subprocess
import sys

import pytest

from test_review_words import assert_verified

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def helper(n, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("GK_REVIEW_WORDS", "GK_RPT", "GK_FORCE_RPP", "GK_NO_JIT", "GK_JIT_REVIEW_WORDS"))}
    e.update({"GK_REVIEW_WORDS": "1", "GK_REVIEW_WORDS_MIN": "0", "GK_JIT_STRICT": "1", "GK_RPT": "256"})
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "review_words_strings.py"), str(n)], capture_output=True, text=True, env=e, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().split("\n")[-1])


def test_string_row_predicates_hoisted():
    """str_prefix_c on every length class of constant and string, evaluated by the binding pass (on) and by the sweep's kernel (off): equal
    result words, both verified against the bytecode kernel, and the pairs are those of the bytes reference (the fillers hold nowhere)"""
    on, off = helper(600), helper(600, GK_REVIEW_WORDS="0")
    assert on["words"] == off["words"] and on["pairs"] == off["pairs"] == on["want_pairs"] > 0
    assert on["hash"] != off["hash"], "the feature was not on: the same kernel text ran"
    assert_verified(on)
    assert_verified(off)
