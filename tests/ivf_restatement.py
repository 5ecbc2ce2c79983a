"""The inverted file (include/mdx_ivf.h; mdir_amd/ivf.py) restated in numpy (a helper module, imported by test_ivf_host.py,
test_gpu_ivf.py and test_gpu_ivf_memcontract.py).

From labels (or members and offsets), the probes of every query and a full score matrix: the candidates of every query -- the members
of its probed lists in probe order, inside a list in member order --, their number, and the first k of them by (order key of the
score, id) with the padding rule.  The scores themselves are not restated here: they are the exact fp32 chain, the bits of an fp32
index of the same rows, and the tests take them from that index (or from tests/lattice.py's integer products)."""
import numpy as np

from kmeans_restatement import csr, order_key

F32 = np.float32
QUERY_GROUP = 8                 # MDX_IVF_QUERY_GROUP of include/mdx_ivf.h
TILE = 64                       # MDX_IVF_TILE


def clamped(offsets, m):
    """The offsets clamped to [0, m] as (start, size) per list; a list whose clamped end lies before its start is empty."""
    o = np.clip(np.asarray(offsets, np.int64), 0, m)
    return o[:-1], np.maximum(o[1:] - o[:-1], 0)


def plan(probes, offsets, m, cap):
    """(base int64 [nq, nprobe], count int64 [nq], entries: per list the sorted q * nprobe + p that probe it, items: the work items)."""
    probes = np.asarray(probes, np.int64)
    nq, nprobe = probes.shape
    k = len(offsets) - 1
    _, sizes = clamped(offsets, m)
    base = np.full((nq, nprobe), -1, np.int64)
    count = np.zeros(nq, np.int64)
    entries = [[] for _ in range(k)]
    for q in range(nq):
        run = 0
        for p in range(nprobe):
            l = int(probes[q, p])
            if 0 <= l < k:
                base[q, p] = run
                run += int(sizes[l])
                entries[l].append(q * nprobe + p)
        count[q] = min(run, cap)
    items = sum(-(-int(sizes[l]) // TILE) * -(-len(entries[l]) // QUERY_GROUP) for l in range(k))
    return base, count, entries, items


def candidates(members, offsets, probes, cap=None):
    """Per query the candidate ids (int64 arrays): the members of its valid probes' lists, in probe order, cut at ``cap``."""
    members = np.asarray(members, np.int64)
    starts, sizes = clamped(offsets, len(members))
    k = len(sizes)
    out = []
    for row in np.asarray(probes, np.int64):
        ids = [members[starts[l]:starts[l] + sizes[l]] for l in row if 0 <= l < k]
        ids = np.concatenate(ids) if ids else np.empty(0, np.int64)
        out.append(ids if cap is None else ids[:cap])
    return out


def candidate_scores(scores_row, ids):
    """The scores of one query's candidates: the full score row at the id; NaN for an id outside it."""
    n = scores_row.shape[0]
    ok = (ids >= 0) & (ids < n)
    out = np.full(ids.shape, np.nan, F32)
    out[ok] = scores_row[ids[ok]]
    return out


def select(cand_scores, cand_ids, k):
    """(ids int64 [k], scores fp32 [k]): the first k candidates by (order key, id); -1 / NaN beyond them."""
    order = np.lexsort((cand_ids, order_key(cand_scores)))[:k]
    ids = np.full(k, -1, np.int64)
    sc = np.full(k, np.nan, F32)
    ids[:len(order)] = cand_ids[order]
    sc[:len(order)] = cand_scores[order]
    return ids, sc


def search(members, offsets, probes, scores, k, cap=None):
    """(ids int64 [nq, k], scores fp32 [nq, k], scanned int64 [nq]) of the full score matrix ``scores`` fp32 [nq, n]."""
    scores = np.ascontiguousarray(scores, F32)
    cands = candidates(members, offsets, probes, cap)
    ids = np.empty((len(cands), k), np.int64)
    sc = np.empty((len(cands), k), F32)
    for q, c in enumerate(cands):
        ids[q], sc[q] = select(candidate_scores(scores[q], c), c, k)
    return ids, sc, np.array([len(c) for c in cands], np.int64)


def search_labels(labels, lists, probes, scores, k):
    """``search`` over the lists of ``labels`` (members ascending inside a list, as cluster._members)."""
    members, offsets = csr(labels, lists)
    return search(members, offsets, probes, scores, k)


def same_bits(got, want):
    """Both arrays hold the same bytes (NaN payloads and the sign of zero included)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    a, b = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
    if not np.array_equal(a, b):
        first = int(np.flatnonzero(a != b)[0]) // got.dtype.itemsize
        raise AssertionError("differs first at flat index %d: %r, not %r" % (first, got.reshape(-1)[first], want.reshape(-1)[first]))


def planted(seed=7, lists=8, per=40, d=64, nq=16, noise=0.05):
    """K unit centres on disjoint blocks of d / K coordinates, ``per`` rows per centre (centre + noise x normal, renormalised),
    queries drawn the same way, the rows shuffled: (rows fp32, truth int64, centres fp32, queries fp32, query truth)."""
    rng = np.random.default_rng(seed)
    block = d // lists
    centres = np.zeros((lists, d))
    for c in range(lists):
        v = rng.standard_normal(block)
        centres[c, c * block:(c + 1) * block] = v / np.linalg.norm(v)

    def draw(count_per):
        truth = np.repeat(np.arange(lists), count_per)
        x = centres[truth] + noise * rng.standard_normal((len(truth), d))
        return x / np.linalg.norm(x, axis=1, keepdims=True), truth
    queries, qtruth = draw(nq // lists)
    rows, truth = draw(per)
    perm = rng.permutation(len(truth))
    return rows[perm].astype(F32), truth[perm].astype(np.int64), centres.astype(F32), queries.astype(F32), qtruth.astype(np.int64)
