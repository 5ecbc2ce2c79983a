"""Spherical k-means (include/mdx_kmeans.h, mdir_amd/cluster.py) restated in numpy (a helper module, imported by test_kmeans_host.py,
test_gpu_kmeans.py and test_gpu_kmeans_memcontract.py; no GPU).

``sums32``      the segment chain that DEFINES ``mdx_kmeans_sums``, in fp32, to the bit
``argmax_first`` the first entry of the ranking of every row of a score block, with the library's tie rule
``finish64``    the normalisation of the sums in float64
``kmeans64``    the whole loop of ``cluster.kmeans`` in float64, with the reseed rule
``planted``     the planted data of the loop tests
"""
from collections import namedtuple

import numpy as np

SEGMENT = 256                   # MDX_KMEANS_SEGMENT of include/mdx_kmeans.h
F32 = np.float32
U = 2.0 ** -24                  # unit roundoff of fp32


def sums32(rows, members, offsets, k, segment=SEGMENT):
    """fp32 [k, d]: per cluster, the members cut into segments of ``segment``; a segment's partial is acc = +0, acc = acc + x over
    its members in order; the cluster's sum the same chain over its partials.  fp32 additions, one rounding each (numpy adds fp32
    arrays element by element in fp32).  Offsets are clamped to [0, n]; an id outside [0, n) is skipped."""
    rows = np.asarray(rows, F32)
    n, d = rows.shape
    members = np.asarray(members, np.int64)
    off = np.clip(np.asarray(offsets, np.int64), 0, n)
    out = np.zeros((k, d), F32)
    for c in range(k):
        total = np.zeros(d, F32)
        for s0 in range(int(off[c]), int(off[c + 1]), segment):
            part = np.zeros(d, F32)
            for i in members[s0:min(s0 + segment, int(off[c + 1]))]:
                if 0 <= i < n:
                    part = part + rows[i]
            total = total + part
        out[c] = total
    return out


def csr(labels, k):
    """(members, offsets) of the labels: a stable sort, so the members of a cluster ascend."""
    labels = np.asarray(labels, np.int64)
    members = np.argsort(labels, kind="stable").astype(np.int64)
    offsets = np.zeros(k + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(labels, minlength=k))
    return members, offsets


def order_key(block):
    """uint32 keys of an fp32 array: smaller = ranked earlier (larger score first, -0 == +0, NaN last); desc_key of the library."""
    u = np.ascontiguousarray(block, F32).view(np.uint32).copy()
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u[(u << 1) == 0] = 0
    neg = (u & 0x80000000) != 0
    u = np.where(neg, ~u, u | np.uint32(0x80000000))
    key = ~u
    key[nan] = 0xFFFFFFFF
    return key


def argmax_first(block):
    """(labels int64 [m], best fp32 [m]): per row the smallest (key, id); ``best`` keeps the bits of the winning element."""
    block = np.ascontiguousarray(block, F32)
    labels = np.argmin(order_key(block), axis=1).astype(np.int64)      # argmin returns the first of equal keys
    return labels, block[np.arange(block.shape[0]), labels]


def finish64(sums, eps=1e-6, previous=None):
    """float64 [k, d]: s / (||s|| + eps); a row of zeros takes ``previous`` (zeros without one)."""
    s = np.asarray(sums, np.float64)
    with np.errstate(invalid="ignore"):                                 # 0 / 0 with eps = 0: a zero row, replaced below
        out = s / (np.sqrt((s * s).sum(axis=1, keepdims=True)) + eps)
    zero = ~(s != 0).any(axis=1)
    out[zero] = 0.0 if previous is None else np.asarray(previous, np.float64)[zero]
    return out


def finish_tolerance(want, d):
    """|got - want| allowed per element of the finish: the any-order bound of a d-term fp32 sum of squares (d/2 after the square
    root), one square root, one addition and one division."""
    return (d / 2 + 4) * U * np.abs(np.asarray(want, np.float64))


Fit = namedtuple("Fit", ["centroids", "labels", "sizes", "history", "iterations", "reseeded", "best", "sum_abs", "terms", "norms"])


def assign64(centroids, rows):
    scores = np.asarray(rows, np.float64) @ np.asarray(centroids, np.float64).T
    labels = np.argmax(scores, axis=1).astype(np.int64)                 # the first of equal maxima
    return labels, scores[np.arange(scores.shape[0]), labels], scores


def kmeans64(rows, k, init_ids, iters=20, tol=0.0, eps=1e-6, train_ids=None):
    """The loop of cluster.kmeans in float64 (init: row ids of ``rows``; ``train_ids``: the training sample).  Beside the results:
    ``sum_abs`` [k, d], ``terms`` [k] and ``norms`` [k] of the LAST update -- per centroid the sum of |x| over the rows it was summed
    from, their number, and the norm of the sum (a reseeded centroid: its row, 1) -- from which a test bounds what any summation
    order in fp32 may do to a centroid."""
    rows = np.asarray(rows, np.float64)
    train = rows if train_ids is None else rows[np.asarray(train_ids)]
    m, d = train.shape
    centroids = rows[np.asarray(init_ids)].copy()
    history, updates, reseeded, previous = [], 0, 0, None
    sum_abs, terms, norms = np.abs(centroids), np.ones(k, np.int64), np.linalg.norm(centroids, axis=1)
    while True:
        labels, best, _ = assign64(centroids, train)
        history.append(float(best.sum()))
        changed = m if previous is None else int((labels != previous).sum())
        if changed <= tol * m or updates == iters:
            break
        sums, sum_abs = np.zeros((k, d)), np.zeros((k, d))
        np.add.at(sums, labels, train)
        np.add.at(sum_abs, labels, np.abs(train))
        terms = np.bincount(labels, minlength=k)
        norms = np.linalg.norm(sums, axis=1)
        centroids = finish64(sums, eps, centroids)
        empty = np.flatnonzero(terms == 0)
        if empty.size:
            worst = np.argsort(best, kind="stable")[:empty.size]        # the smallest best first, equal values by ascending row id
            centroids[empty] = finish64(train[worst], eps)
            sum_abs[empty], terms[empty], norms[empty] = np.abs(train[worst]), 1, np.linalg.norm(train[worst], axis=1)
            reseeded += int(empty.size)
        previous = labels
        updates += 1
    if train_ids is not None:
        labels, best, _ = assign64(centroids, rows)
    return Fit(centroids, labels, np.bincount(labels, minlength=k), history, updates, reseeded, best, sum_abs, terms, norms)


def centroid_tolerance(fit, d, eps=1e-6):
    """|got - want| allowed per element of a centroid that the device summed in fp32 in an order of its own: the finish tolerance plus
    what the error of the sum does to the quotient.  A sum of t fp32 terms in ANY order is within delta = gamma_t * sum|x| of the
    exact one, gamma_t = t u / (1 - t u); to first order c = s / (||s|| + eps) moves by at most
    (|delta_i| + |c_i| ||delta||_2) / (||s|| + eps), and the factor 1 + 2^-10 covers the higher orders (delta / ||s|| is below 2^-14
    here)."""
    t = fit.terms.astype(np.float64)[:, None]
    delta = t * U / (1 - t * U) * fit.sum_abs
    moved = (delta + np.abs(fit.centroids) * np.linalg.norm(delta, axis=1, keepdims=True)) / (fit.norms[:, None] + eps)
    return finish_tolerance(fit.centroids, d) + (1 + 2.0 ** -10) * moved


def planted(n=600, d=32, k=6, seed=5, noise=0.05):
    """(rows fp32 [n, d], truth int64 [n]): k unit centres, n / k rows each with ``noise`` per coordinate added, renormalised and
    shuffled."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    truth = np.repeat(np.arange(k), n // k)
    x = centres[truth] + noise * rng.standard_normal((truth.size, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    perm = rng.permutation(truth.size)
    return x[perm].astype(F32), truth[perm].astype(np.int64)


def planted_inits(truth, k):
    """(a) the first row of every planted cluster; (b) the same with id 5 replaced by id 0: two identical centroids."""
    first = [int(np.flatnonzero(truth == c)[0]) for c in range(k)]
    return first, first[:5] + [first[0]] + first[6:]


def pure(labels, truth, k):
    """True when every cluster holds the rows of exactly one planted cluster and every planted cluster is one cluster."""
    pairs = set(zip(labels.tolist(), truth.tolist()))
    return len(pairs) == k and len({a for a, _ in pairs}) == k and len({b for _, b in pairs}) == k
