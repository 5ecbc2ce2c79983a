"""The graph index (include/mdx_graph.h; mdir_amd/graph.py) restated in numpy: a helper module, imported by test_graph_host.py and the
GPU tests of the graph index.  Everything here is sequential and literal; the scores come from oracle.chain.scores_chain, the k-ascending
fmaf chain that mdx_scores is pinned to.

    graph_search   the walk of mdx_graph_search, with a switch for the visited set ("exact" | "none")
    detours        mdx_graph_detours
    strip_self, optimise, medoids      the build of GraphIndex.from_lists and graph.medoids
"""
import numpy as np

from oracle import chain

MAX_D, MAX_DEGREE, MAX_SEEDS, MAX_BEAM, MAX_WIDTH, MAX_CANDIDATES, MAX_K0 = 8192, 64, 512, 512, 8, 512, 128


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def desc_key(s):
    """The order key of mdx_rank_full as a Python int: smaller = earlier; larger score first, -0 == +0, NaN last."""
    u = int(np.float32(s).view(np.uint32))
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return 0xFFFFFFFF
    if (u << 1) & 0xFFFFFFFF == 0:
        u = 0
    u = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return ~u & 0xFFFFFFFF


def all_scores(rows, queries, center=None):
    """fp32 [nq, n]: the exact chain of every (query, row), x_q = q - center in fp32."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if center is not None:
        q = (q - np.asarray(center, dtype=np.float32)[None, :]).astype(np.float32)
    return chain.scores_chain(rows.T, q.T)


def graph_search(scores, graph, seeds, k, L, W=1, T=None, visited="exact"):
    """(ids int64 [nq, k], scores fp32 [nq, k], steps int32 [nq], scored int32 [nq]) of the walk over ``graph`` int [n, R] from
    ``seeds`` int [nq, S], on the precomputed ``scores`` fp32 [nq, n] (:func:`all_scores`).  ``visited``: "exact" never scores a row
    twice, "none" scores every candidate that is not in the beam; only ``scored`` may depend on it."""
    assert visited in ("exact", "none")
    graph, seeds = np.asarray(graph), np.asarray(seeds)
    nq, n = scores.shape
    T = 1 << 62 if T is None else T
    out_ids = np.full((nq, k), -1, dtype=np.int64)
    out_sc = np.full((nq, k), np.nan, dtype=np.float32)
    out_steps = np.zeros(nq, dtype=np.int32)
    out_scored = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        order = lambda i: (desc_key(scores[q, i]), i)
        seen, scored = set(), 0
        beam, expanded = [], set()

        def merge(cands):
            nonlocal beam, scored
            fresh = []
            for c in cands:
                c = int(c)
                if c < 0 or c >= n or c in beam or c in fresh:
                    continue
                if visited == "exact" and c in seen:
                    continue
                seen.add(c)
                fresh.append(c)
            scored += len(fresh)
            beam = sorted(beam + fresh, key=order)[:L]

        merge(seeds[q])
        steps = 0
        while steps < T:
            parents = [i for i in beam if i not in expanded][:W]
            if not parents:
                break
            expanded.update(parents)
            steps += 1
            merge([c for p in parents for c in graph[p]])
        head = beam[:k]
        out_ids[q, :len(head)] = head
        out_sc[q, :len(head)] = scores[q, head]
        out_steps[q], out_scored[q] = steps, scored
    return out_ids, out_sc, out_steps, out_scored


def same_scores(got, want):
    """The score contract: NaN where the restatement has NaN, the same bits everywhere else."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(bits(got)[~nan], bits(want)[~nan])


def detours(lists):
    """int32 [n, K0]: for a valid b = lists[i, j] the ranks t < j with a valid a = lists[i, t] whose list holds b before rank j; K0
    for an invalid entry."""
    lists = np.asarray(lists, dtype=np.int64)
    n, k0 = lists.shape
    out = np.full((n, k0), k0, dtype=np.int32)
    valid = (lists >= 0) & (lists < n)
    tri = np.arange(k0)[:, None] < np.arange(k0)[None, :]            # [t or r, j]: t < j, r < j
    for i in range(n):
        sub = lists[np.where(valid[i], lists[i], 0)]                  # [t, r]: the lists of row i's neighbours
        hit = (sub[:, :, None] == lists[i][None, None, :]) & tri[None, :, :]          # [t, r, j]: lists[a_t, r] == b_j, r < j
        walks = hit.any(axis=1) & tri & valid[i][:, None]                             # [t, j]: a detour i -> a_t -> b_j
        out[i, valid[i]] = walks.sum(axis=0)[valid[i]]
    return out


def strip_self(ids):
    """int64 [n, k - 1]: per row the valid entries that are not the row's own id, in order, the first k - 1, padded with -1."""
    ids = np.asarray(ids, dtype=np.int64)
    n, k = ids.shape
    out = np.full((n, k - 1), -1, dtype=np.int64)
    for i in range(n):
        keep = [int(x) for x in ids[i] if 0 <= x < n and x != i][:k - 1]
        out[i, :len(keep)] = keep
    return out


def optimise(lists, degree, det=None):
    """int32 [n, degree]: the search graph of neighbour lists (best first, own id removed): forward lists by (detours, rank), reverse
    lists by (rank in the source's forward list, source), interleaved, the first ``degree`` distinct ids that are not the row's own."""
    lists = np.asarray(lists, dtype=np.int64)
    n, k0 = lists.shape
    det = detours(lists) if det is None else np.asarray(det)
    fwd = []
    for i in range(n):
        pos = sorted(range(k0), key=lambda j: (int(det[i, j]), j))[:degree]
        fwd.append([int(lists[i, j]) for j in pos if 0 <= lists[i, j] < n])
    offers = [[] for _ in range(n)]
    for i in range(n):
        for j, b in enumerate(fwd[i]):
            offers[b].append((j, i))
    out = np.full((n, degree), -1, dtype=np.int32)
    for b in range(n):
        rev = [i for _, i in sorted(offers[b])[:degree]]
        seq = []
        for j in range(max(len(fwd[b]), len(rev))):
            seq += fwd[b][j:j + 1] + rev[j:j + 1]
        row = []
        for x in seq:
            if x != b and x not in row:
                row.append(x)
        row = row[:degree]
        out[b, :len(row)] = row
    return out


def truncate(lists, degree):
    """The plain kNN graph at the same degree: the first ``degree`` entries of every list, as int32 (padded with -1)."""
    lists = np.asarray(lists, dtype=np.int64)
    out = np.full((lists.shape[0], degree), -1, dtype=np.int32)
    m = min(degree, lists.shape[1])
    out[:, :m] = lists[:, :m]
    return out


def medoids(rows, centroids, labels):
    """int64 [number of non-empty lists]: per list, in ascending list id, the member with the best chain score against its centroid
    (rank_full's order), ties to the smaller id."""
    rows, centroids, labels = np.asarray(rows, np.float32), np.asarray(centroids, np.float32), np.asarray(labels)
    sc = chain.scores_chain(rows.T, centroids.T)                      # [K, n]
    out = []
    for c in range(centroids.shape[0]):
        members = np.nonzero(labels == c)[0]
        if members.size:
            out.append(min(members.tolist(), key=lambda i: (desc_key(sc[c, i]), i)))
    return np.array(out, dtype=np.int64)


def knn_lists(rows, k):
    """int64 [n, k]: the exact top-k of every row against all rows (its own match included), rank_full's order."""
    sc = all_scores(rows, rows)
    return chain.rank_full(sc)[:, :k]


# ---------------------------------------------------------------------------------------------------------------- problem makers

def random_graph(rng, n, R, spoil=True):
    """int32 [n, R]: random neighbours; with ``spoil`` also -1 padding, ids >= n, repeats and self loops."""
    g = rng.integers(0, n, size=(n, R)).astype(np.int32)
    if spoil:
        m = rng.random((n, R))
        g[m < 0.08] = -1
        g[(m >= 0.08) & (m < 0.14)] = n + 3
        g[(m >= 0.14) & (m < 0.16)] = np.iinfo(np.int32).max
        if R > 1:
            rep = m[:, 1] > 0.8
            g[rep, 1] = g[rep, 0]
        loops = m[:, 0] > 0.9
        g[loops, 0] = np.nonzero(loops)[0]
    return g


def ring_graph(n, R):
    """int32 [n, R]: row i lists i + 1, .., i + R (mod n): every row is reachable from every seed."""
    return ((np.arange(n)[:, None] + 1 + np.arange(R)[None, :]) % n).astype(np.int32)


def problem(n, d, nq, R, S, seed, spoil=True, ld=None):
    """(rows [n, d], queries [nq, d], graph, seeds int64 [nq, S]) of random data; the seeds hold -1, an id >= n and repeats."""
    rng = np.random.default_rng([seed, n, d, nq, R, S])
    rows = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    graph = random_graph(rng, n, R, spoil)
    seeds = rng.integers(0, n, size=(nq, S)).astype(np.int64)
    if spoil and S > 2:
        seeds[:, 1] = -1
        seeds[:, 2] = seeds[:, 0]
        if S > 3:
            seeds[:, 3] = n
    return rows, queries, graph, seeds


def clustered(n=4096, d=64, clusters=64, nq=64, seed=20, noise=1.0, qnoise=1.0):
    """(rows, queries): L2-normalised rows around ``clusters`` random centres, the queries noisy copies of random rows."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, d))
    which = rng.integers(0, clusters, size=n)
    rows = centres[which] + noise * rng.standard_normal((n, d))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    picks = rng.integers(0, n, size=nq)
    queries = rows[picks] + qnoise * rng.standard_normal((nq, d)) / np.sqrt(d)
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    return rows.astype(np.float32), queries.astype(np.float32), which


def recall(found, exact):
    """The mean share of ``exact`` [nq, k] that ``found`` [nq, k] holds."""
    return float(np.mean([len(set(f.tolist()) & set(e.tolist())) / len(e) for f, e in zip(found, exact)]))
