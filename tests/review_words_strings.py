"""Helper of test_review_words_strings.py, run as a script in a process of its own on the GPU, as review_words_util.py is (the review-words
switches are read once per process).  Policy "strings": string ROW predicates as an all-global class -- the prefix family of
tests/test_string_rows.py on the annotation only, behind a full dictionary of the review facts.  Prints one JSON line: review_words_util's
summary of one resident table of the first N probe Pods, and the number of pairs the bytes reference holds.
usage: review_words_strings.py N"""
import json
import sys

import review_words_util as RW   # (puts the repository and tests/ on sys.path)
import str_rows_util as S

D = RW.D


def client():
    c = D.Client(D.Driver(device=0, hostemu=False))
    ft, fc = S.fill_policy([S.PROBE])
    templates, constraints, what = S.family_policy(S.FAMILIES["prefix"], places=("Rev",))
    for t in [ft] + templates:
        c.AddTemplate(t)
    for k in fc + constraints:
        c.AddConstraint(k)
    for kind in (S.kind_of(t, "Rev") for t in S.FAMILIES["prefix"]):
        S.require_rows(c, kind, S.P_STR_PREFIX, len(S.CONSTANTS), dsts=(0,))
    return c, what


def case(n):
    c, what = client()
    objs = [S.pod(i, [s], s) for i, s in enumerate(S.probe_strings()[:n])]
    table = c.driver.engine.create_table([D.to_review_in(r, None) for r in S.reviews_of(objs)], keep_docs=False, resident=True)
    try:
        print(json.dumps(dict(RW.summary(c, table), want_pairs=len(S.want_pairs(what, objs)))))
    finally:
        table.free()


if __name__ == "__main__":
    case(int(sys.argv[1]))
