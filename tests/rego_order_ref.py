"""A plain reference for Rego's total order on the JSON values a review can hold: sign(a, b) is -1, 0 or 1 as a sorts before, with
or behind b.  null < false < true < number < string < array < object.  It exists so that the oracle (oracle/values.py compare) is not
the only witness of the ordering tests: it imports nothing of the oracle and nothing of the product, and shares no code with either.

Numbers are the numbers a review holds after Kubernetes decoded its JSON: integral text that fits an int64 is that integer, every
other number is the float64 nearest to its text.  Python's json module has made exactly that split already -- an `int` for integral
text, a `float` for the rest --, so what is left is an int beyond int64 (the float64 of its text).  Both kinds are then compared as
exact rationals: an int64 against a double is never rounded.
Strings compare by their UTF-8 bytes (for well-formed text: the order of their code points), a proper prefix first.
Arrays compare element by element, then by length; objects by their sorted keys and the values under them, then by size: the empty
array sorts behind every string and before every other array, the empty object behind every array."""
from fractions import Fraction

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


def kind(v):
    if v is None:
        return 0
    if isinstance(v, bool):
        return 1
    if isinstance(v, (int, float)):
        return 2
    if isinstance(v, str):
        return 3
    if isinstance(v, (list, tuple)):
        return 4
    if isinstance(v, dict):
        return 5
    raise TypeError("not a JSON value: %r" % (v,))


def number(v):
    """the exact value of a decoded JSON number"""
    if isinstance(v, int) and not INT64_MIN <= v <= INT64_MAX:
        v = float(v)     # (the text does not fit an int64: the float64 nearest to it)
    if isinstance(v, float) and (v != v or v in (float("inf"), float("-inf"))):
        raise ValueError("not a JSON number: %r" % (v,))
    return Fraction(v)   # (exact for an int and for a float alike)


def _sgn(x, y):
    return (x > y) - (x < y)


def _seq(a, b):
    for x, y in zip(a, b):
        s = sign(x, y)
        if s:
            return s
    return _sgn(len(a), len(b))


def sign(a, b):
    ka, kb = kind(a), kind(b)
    if ka != kb:
        return _sgn(ka, kb)
    if ka == 0:
        return 0
    if ka == 1:
        return _sgn(int(a), int(b))
    if ka == 2:
        return _sgn(number(a), number(b))
    if ka == 3:
        return _sgn(a.encode("utf-8"), b.encode("utf-8"))
    if ka == 4:
        return _seq(a, b)
    ks, kt = sorted(a, key=lambda s: s.encode("utf-8")), sorted(b, key=lambda s: s.encode("utf-8"))
    for x, y in zip(ks, kt):
        s = sign(x, y) or sign(a[x], b[y])
        if s:
            return s
    return _sgn(len(ks), len(kt))


RELATIONS = {"Lt": lambda s: s < 0, "Le": lambda s: s <= 0, "Gt": lambda s: s > 0, "Ge": lambda s: s >= 0}


def relations(a, b):
    """the names of the four ordering relations (value_order_util.RELS) that hold between a and b, sorted"""
    s = sign(a, b)
    return sorted(r for r, f in RELATIONS.items() if f(s))
