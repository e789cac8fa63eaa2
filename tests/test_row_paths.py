"""The split / trim, path-prefix and regular-expression tests of test_split_masks.py and test_parity.py once more, on the device's ROW
predicates.  As those modules load their policies, the lowering promotes every split, trim and re_match test to a dictionary expression: the
HOST's builtins answer per distinct value and the device tests a bit of <leaf>.$d -- test_split_masks.py's "every length class of the
device's byte-position masks" is, as loaded, every length class of the host's builtins.  The cases here are the ones that reach the masks
(P_SPLIT_CMP, P_SPLIT_COUNT, P_SPLIT_PREFIX) and the four-bytes-per-round DFA walk (P_REGEX): the same test functions are called with their
module's load_both replaced by str_rows_util.rows_loader, which fills the dictionaries of the leaves the templates read before it loads the
same policies, and then fails the test (str_rows_util.require_rows) unless they were lowered to those row predicates.  Strings, oracle
comparison and assertions are the called tests' own."""
import pytest

import str_rows_util as S
import test_parity
import test_split_masks
from parity_util import BACKENDS

IMAGE, HOSTPATH = S.IMAGE, "input.review.object.spec.volumes[_].hostPath.path"


@pytest.mark.parametrize("backend", BACKENDS)
def test_split_and_trim_on_the_rows(backend, monkeypatch):
    def guard(c):   # six component comparisons and three component counts per template, all in the element scope
        for k in test_split_masks.T:
            S.require_rows(c, k, S.P_SPLIT_CMP, 1, dsts=(1,), min_preds=6)
            S.require_rows(c, k, S.P_SPLIT_COUNT, 1, dsts=(1,), min_preds=3)
    monkeypatch.setattr(test_split_masks, "load_both", S.rows_loader([IMAGE, HOSTPATH], guard))
    test_split_masks.test_split_and_trim_at_every_length_class(backend)


@pytest.mark.parametrize("backend", BACKENDS)
def test_path_prefixes_on_the_rows(backend, fixtures, monkeypatch):
    def guard(c):   # one fused prefix predicate per distinct trimmed prefix (/var/lib and /var/lib/ are one): seven constraints, seven at least
        S.require_rows(c, "K8sPSPHostFilesystem", S.P_SPLIT_PREFIX, 7, dsts=(1,))
    # (S.PROBE: the review facts' row, which the template's review-level tests would add a bit to)
    monkeypatch.setattr(test_split_masks, "load_both", S.rows_loader([HOSTPATH, S.PROBE], guard))
    test_split_masks.test_path_prefixes_at_every_length_class(backend, fixtures)


@pytest.mark.parametrize("backend", BACKENDS)
def test_regex_predicates_on_the_rows(backend, monkeypatch):
    """behind a full dictionary of the review facts the device walks the DFA itself"""
    n = len(test_parity.REGEXES)

    def guard(c):   # one pattern of REGEXES does not compile (undefined); the others on the three leaves, all review-level
        S.require_rows(c, "K8sLabelRegex", S.P_REGEX, n, dsts=(0,), min_preds=3 * (n - 1))
    monkeypatch.setattr(test_parity, "load_both", S.rows_loader([S.PROBE], guard))
    test_parity.test_regex_predicates(backend)
