"""``mdx_topk_overlap`` (include/mdx_overlap.h; ops.topk_overlap) restated in numpy, one query and one depth at a time, and the row
makers the overlap tests share."""
import numpy as np

MAX_K = 4096
MAX_DEPTHS = 8
TOP = (1 << 31) - 1                 # the largest id the kernel compares


def topk_overlap(a, b, depths):
    """int32 ``[nq, T]``: the ids >= 0 among the first ``min(depths[t], ka)`` entries of ``a[q]`` that occur among the first
    ``min(depths[t], kb)`` entries of ``b[q]`` (ids at or above 2^31 are padding, as the kernel reads them)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    out = np.zeros((a.shape[0], len(depths)), dtype=np.int32)
    for q in range(a.shape[0]):
        for t, depth in enumerate(depths):
            theirs = {int(x) for x in b[q, :min(depth, b.shape[1])] if 0 <= x <= TOP}
            out[q, t] = sum(1 for x in a[q, :min(depth, a.shape[1])] if int(x) in theirs)
    return out


def recall_at(found, exact, depths):
    """float64 ``[nq, T]``: the counts over ``min(depth, valid entries of exact[q])`` (search.recall_at)."""
    valid = (np.asarray(exact) >= 0).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return topk_overlap(found, exact, depths).astype(np.float64) / np.minimum(np.asarray(depths, dtype=np.int64)[None, :], valid[:, None])


KINDS = ("identical", "disjoint", "half", "padding", "padded_tail", "shuffled")


def rows(kind, ka, kb, rng, high=False):
    """One query's ``(a [ka], b [kb])``: distinct ids >= 0 plus -1 padding.  ``high``: ids near 2^31 - 1."""
    pool = rng.permutation(3 * MAX_K)[:ka + kb].astype(np.int64)
    if high:
        pool = TOP - pool
    a, b = pool[:ka].copy(), pool[ka:ka + kb].copy()
    m = min(ka, kb)
    if kind == "identical":
        b[:m] = a[:m]
    elif kind == "half":                              # every other entry of the common prefix is shared, at the same position
        b[:m:2] = a[:m:2]
    elif kind == "padding":
        a[:], b[:] = -1, -1
    elif kind == "padded_tail":                       # shared ids, then padding from the middle on (at different places)
        b[:m] = a[:m]
        a[ka // 2:], b[(kb + 1) // 3:] = -1, -1
    elif kind == "shuffled":                          # the same ids in another order: what a hit's depth max(i, j) is about
        b[:m] = rng.permutation(a[:m])
    else:
        assert kind == "disjoint", kind
    return a, b


def problem(nq, ka, kb, seed, high=False):
    """``(a int64 [nq, ka], b int64 [nq, kb])`` whose queries cycle through :data:`KINDS`."""
    rng = np.random.default_rng(seed)
    pairs = [rows(KINDS[(q + seed) % len(KINDS)], ka, kb, rng, high) for q in range(nq)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def straddling(ka, kb, t):
    """``t`` ascending positive depths around ``ka`` and ``kb``: below both, at each, between and beyond."""
    lo, hi = min(ka, kb), max(ka, kb)
    want = sorted({1, max(1, lo // 2), max(1, lo - 1), lo, lo + 1, max(1, (lo + hi) // 2), hi, hi + 7})
    if t == 1:
        return [lo + 1 if lo < hi else lo]
    while len(want) < t:
        want.append(want[-1] + 1000)
    return want[-t:] if len(want) > t else want
