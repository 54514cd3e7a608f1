"""The rules of the angular similarity on abundances (include/sourmash_amd.h, "Angular similarity") in plain
Python: sketches are dicts {hash: abundance}, dot and norm2 are Python ints, the floats come from math.sqrt / math.acos in
exactly the order the header fixes.  Nothing here knows the library."""
import math

U64 = 1 << 64


class Norm2Overflow(ValueError):
    """the sketch's norm2 does not fit 64 bits: the library refuses it"""


def norm2(a):
    n = sum(v * v for v in a.values())
    if n >= U64:
        raise Norm2Overflow(n)
    return n


def dot(a, b):
    if len(b) < len(a):
        a, b = b, a
    return sum(v * b[h] for h, v in a.items() if h in b)


def cosine_of(d, n2a, n2b):
    if d == 0 or n2a == 0 or n2b == 0:
        return 0.0
    c = float(d) / (math.sqrt(float(n2a)) * math.sqrt(float(n2b)))   # int -> float rounds to nearest
    return 1.0 if c > 1.0 else c


def angular_of(c):
    if c == 0.0:
        return 0.0
    if c == 1.0:
        return 1.0
    return 1.0 - (2.0 * math.acos(c)) / math.pi


def pair(a, b):
    """(dot, norm2 of a, norm2 of b, cosine, angular) of two sketches"""
    na, nb = norm2(a), norm2(b)
    d = dot(a, b)
    c = cosine_of(d, na, nb)
    return d, na, nb, c, angular_of(c)


def angular(a, b):
    return pair(a, b)[4]


def block(rows, cols, symmetric=False):
    """(dot, cosine, angular) as lists of lists.  symmetric: rows and cols are one collection -- the diagonal is dot = norm2,
    cosine = angular = 1.0 (0.0 for an empty sketch) and the lower triangle mirrors the upper one."""
    nr = [norm2(r) for r in rows]
    nc = nr if symmetric else [norm2(c) for c in cols]
    D = [[0] * len(cols) for _ in rows]
    Cs = [[0.0] * len(cols) for _ in rows]
    A = [[0.0] * len(cols) for _ in rows]
    for i, r in enumerate(rows):
        for j, c in enumerate(cols):
            if symmetric and j < i:
                D[i][j], Cs[i][j], A[i][j] = D[j][i], Cs[j][i], A[j][i]
            elif symmetric and j == i:
                D[i][j] = nr[i]
                Cs[i][j] = A[i][j] = 1.0 if nr[i] else 0.0
            else:
                d = dot(r, c)
                D[i][j] = d
                Cs[i][j] = cosine_of(d, nr[i], nc[j])
                A[i][j] = angular_of(Cs[i][j])
    return D, Cs, A
