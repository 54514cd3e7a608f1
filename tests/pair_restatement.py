"""One ordered pair of the compare restated in plain numpy (reference src/lib.rs:428-436, 470-508; src/index.rs:146-154).

No product import: this is what the pair, wave and few-vs-many kernels of compare_kernels.hip are compared against, with
`==` (the f64 results are quotients of exactly representable integers).  A sketch is an ascending array of distinct uint64
hashes; `n` is the num of `a`, the sketch the call is made on (0: no truncation).  test_pair_rules.py checks every function
here against the C oracle."""
import numpy as np

U64 = np.uint64


def _u64(a):
    return np.ascontiguousarray(a, dtype=U64).reshape(-1)


def pair(a, b, n):
    """(common, size, count_common, jaccard, containment) of a.compare(b) and its kin:
    u = a | b, cc = |a & b|;  |u| > n != 0: size = n, common = |a & b & u[:n]|;  otherwise size = |u|, common = cc;
    jaccard = common / max(size, 1);  containment = cc / |a| (NaN for an empty a)."""
    a, b = _u64(a), _u64(b)
    both = np.intersect1d(a, b, assume_unique=True)
    cc = int(both.size)
    tot_u = int(a.size) + int(b.size) - cc
    if n != 0 and tot_u > n:
        u = np.union1d(a, b)
        size = int(n)
        common = int(np.searchsorted(both, u[n - 1], side="right"))     # members of both among the n smallest of the union
    else:
        size, common = tot_u, cc
    jaccard = common / max(size, 1)
    containment = cc / a.size if a.size else float("nan")
    return common, size, cc, jaccard, containment


def union_rank_of_merged_prefix(a, b, m):
    """how many distinct hashes the first m elements of the merged sequence of a and b hold (ties: a first): the union rank
    at which a kernel that cuts the MERGED sequence into equal shares passes from one share to the next"""
    a, b = _u64(a), _u64(b)
    merged = np.sort(np.concatenate([a, b]), kind="stable")[:m]
    return int(np.unique(merged).size)


# ---- the inputs of the small-route tests (test_pair_rules.py runs the oracle over them, test_gpu_compare_small_routes.py the kernels)
EXTREMES = np.array([0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1], dtype=U64)


def _body(rng, k, lo=1, hi=(1 << 64) - 2):
    """k distinct hashes of [lo, hi], ascending, none of them one of EXTREMES"""
    if k == 0:
        return np.zeros(0, dtype=U64)
    while True:
        v = np.unique(rng.integers(lo, hi, size=k + 16, dtype=U64, endpoint=True))
        v = v[~np.isin(v, EXTREMES)]
        if v.size >= k:
            return np.sort(rng.choice(v, k, replace=False))


def _join(body, ext):
    return np.unique(np.concatenate([_u64(body), _u64(ext)]))


def structures(total, rng):
    """[(name, a, b)] with len(a) + len(b) == total: identical sketches (an odd total: b holds one hash more), interleaved
    disjoint ones, all of a below all of b and the reverse, either side empty, and a random overlap of about a half.  Every
    structure but the empty-sided ones comes twice: "both" holds 0, 2^63 - 1, 2^63 and 2^64 - 1 in both sketches, "one"
    holds each of them in one sketch only (neighbours across the sign bit in different sketches; the below-structures keep
    all of one sketch below all of the other).  Sketches too short for four extremes hold the first few.  The other hashes
    are spread over all of [1, 2^64 - 2]."""
    la, lb = total // 2, total - total // 2
    out = []
    for mode in ("both", "one"):
        ea, eb = (EXTREMES, EXTREMES) if mode == "both" else (EXTREMES[[0, 2]], EXTREMES[[1, 3]])
        ea, eb = ea[:la], eb[:lb]
        ka, kb = la - ea.size, lb - eb.size
        # identical bodies
        body = _body(rng, max(ka, kb))
        out.append(("identical-" + mode, _join(rng.choice(body, ka, replace=False), ea), _join(rng.choice(body, kb, replace=False), eb)))
        # interleaved disjoint bodies: the shorter side takes every other position
        body = _body(rng, ka + kb)
        odd = np.zeros(ka + kb, dtype=bool)
        odd[1:2 * min(ka, kb):2] = True
        out.append(("interleaved-" + mode, _join(body[odd if ka <= kb else ~odd], ea), _join(body[~odd if ka <= kb else odd], eb)))
        # all of one below all of the other (with "one": strictly, extremes included)
        for name, (lx, ly) in (("a-below-b-", (la, lb)), ("b-below-a-", (lb, la))):
            ex, ey = (EXTREMES, EXTREMES) if mode == "both" else (EXTREMES[:2], EXTREMES[2:])
            ex, ey = ex[:lx], ey[:ly]
            x = _join(_body(rng, lx - ex.size, 1, (1 << 63) - 2), ex)
            y = _join(_body(rng, ly - ey.size, (1 << 63) + 1, (1 << 64) - 2), ey)
            out.append((name + mode, x, y) if name[0] == "a" else (name + mode, y, x))
        # a random overlap of about a half
        c = min(ka, kb) // 2
        body = _body(rng, ka + kb - c)
        perm = rng.permutation(body.size)
        out.append(("half-overlap-" + mode, _join(body[perm[:ka]], ea), _join(body[np.concatenate([perm[:c], perm[ka:]])], eb)))
    ext = EXTREMES[:total]
    full = _join(_body(rng, total - ext.size), ext)
    out.append(("a-empty", np.zeros(0, dtype=U64), full))
    out.append(("b-empty", full.copy(), np.zeros(0, dtype=U64)))
    for name, a, b in out:
        assert a.size + b.size == total, (name, a.size, b.size, total)
        assert (a[1:] > a[:-1]).all() and (b[1:] > b[:-1]).all(), name
    return out


def matrix(rows, cols, nums):
    """pair() of every (row, column): dict name -> (len(rows), len(cols)) array.  nums: one n for every row, or one per row
    (quirk H6: row i's num truncates pair (i, j))."""
    nr, nc = len(rows), len(cols)
    nums = [int(nums)] * nr if np.isscalar(nums) else [int(v) for v in nums]
    assert len(nums) == nr
    out = {"common": np.zeros((nr, nc), dtype=U64), "size": np.zeros((nr, nc), dtype=U64),
           "count_common": np.zeros((nr, nc), dtype=U64), "jaccard": np.zeros((nr, nc), dtype=np.float64),
           "containment": np.zeros((nr, nc), dtype=np.float64)}
    for i, a in enumerate(rows):
        for j, b in enumerate(cols):
            c, s, cc, jac, cont = pair(a, b, nums[i])
            out["common"][i, j], out["size"][i, j], out["count_common"][i, j] = c, s, cc
            out["jaccard"][i, j], out["containment"][i, j] = jac, cont
    return out
