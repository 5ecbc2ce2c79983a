"""The staged exact chain of mdx_exact.h on its stage boundaries, in both kernels that run it: rescore_kernel (stages of 256 k,
``ops.rescore``) and exact_kernel (stages of 128 k; with a threshold behind ``search.range_search``, without one behind the kNN
join).  d = 192 and 320 end in a partial second stage of the one and of the other, 129 and 257 carry one element into a new
block of 64, 127 and 255 stop one short of a stage.  Every d runs on rows that lie contiguous (16-byte pieces where d % 4 == 0)
and on the same rows as a slice of a matrix one column wider (ld = d + 1: element loads, except at d = 127 and 255, where
ld % 4 == 0 and only a row's last piece is loaded by element); the spare column holds NaN, so a read beyond d shows.  Expected:
the fp32 chain kernel of an index of the same rows, compared bit for bit, NaN included, ids by the tie rule."""
import functools

import numpy as np
import pytest
import torch

from test_rescore_host import rank_order

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, NQ, KNN = 70, 3, 5
INF_ROW, NAN_ROW, ZERO_ROW = 5, 40, 69
DIMS = [127, 128, 129, 192, 255, 256, 257, 320]
LAYOUTS = ["contiguous", "slice"]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared arrays are read-only


@functools.lru_cache(maxsize=None)
def problem(d):
    """(rows [N, d], queries [NQ, d], chain scores [NQ, N], chain scores of the rows against themselves [N, N]) on the host: one
    fixed draw per d, the scores from the fp32 index; shared by every test of that d and never written."""
    from mdir_amd import ops
    rng = np.random.default_rng(1000 + d)
    x = rng.standard_normal((N, d), dtype=np.float32)
    x[INF_ROW] = np.inf
    x[NAN_ROW] = np.nan
    x[ZERO_ROW] = 0
    x[11] = x[10]                                            # equal scores: ascending id
    q = rng.standard_normal((NQ, d), dtype=np.float32)
    q[0] = np.abs(q[0])                                      # +inf against the infinite row; the other queries score NaN there
    rows = dev(x)
    fix = ops.DescriptorIndex(rows, "ND")
    full = fix.scores(dev(q), "ND").cpu().numpy()
    self_scores = fix.scores(rows, "ND").cpu().numpy()
    fix.close()
    assert np.isposinf(full[0, INF_ROW]) and np.isnan(full[:, NAN_ROW]).all() and (full[:, ZERO_ROW] == 0).all()
    for a in (x, q, full, self_scores):
        a.setflags(write=False)
    return x, q, full, self_scores


def device_rows(x, layout):
    if layout == "contiguous":
        return dev(x)
    big = torch.full((x.shape[0], x.shape[1] + 1), float("nan"), dtype=torch.float32, device=DEV)
    big[:, :-1] = dev(x)
    rows = big[:, :-1]
    assert rows.stride(0) == x.shape[1] + 1
    return rows


def same_bits(got, want):
    got, want = got.cpu(), torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32))
    return got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", DIMS)
def test_rescore_on_the_stage_boundaries(d, layout):
    from mdir_amd import ops
    x, q, full, _ = problem(d)
    rng = np.random.default_rng(d)
    ids = np.stack([rng.permutation(N) for _ in range(NQ)]).astype(np.int64)          # K = N: every row, in some order
    got_ids, got_sc = ops.rescore(device_rows(x, layout), dev(q), dev(ids), "ND")
    for i in range(NQ):
        want_ids, want_sc = rank_order(full[i, ids[i]], ids[i])
        np.testing.assert_array_equal(got_ids[i].cpu().numpy(), want_ids)
        assert same_bits(got_sc[i], want_sc), (d, layout, i)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", DIMS)
def test_range_search_on_the_stage_boundaries(d, layout):
    from mdir_amd import ops
    from mdir_amd.search import range_search
    x, q, full, _ = problem(d)
    rows = device_rows(x, layout)
    ix = ops.DescriptorIndex(rows.contiguous(), "ND", storage="i8")
    tau = -1e30                                              # below every score that is a number: only a NaN chain is no hit
    res = range_search(ix, rows, dev(q), tau)
    ix.close()
    offsets = res.offsets.cpu().numpy()
    assert offsets[0] == 0 and offsets[NQ] == res.ids.numel() == res.scores.numel()
    for i in range(NQ):
        hit = np.nonzero(full[i] >= np.float32(tau))[0].astype(np.int64)
        assert hit.size >= N - 2
        want_ids, want_sc = rank_order(full[i, hit], hit)
        lo, hi = offsets[i], offsets[i + 1]
        np.testing.assert_array_equal(res.ids[lo:hi].cpu().numpy(), want_ids)
        assert same_bits(res.scores[lo:hi], want_sc), (d, layout, i)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", DIMS)
def test_knn_join_on_the_stage_boundaries(d, layout):
    """bounds -> candidates -> resolve, the int8 route of ``search.knn_join`` with no way round exact_kernel: at 70 structureless
    rows the bound does not prune, and ``knn_join`` itself then takes its exact route, which reads contiguous rows only.  On
    contiguous rows ``knn_join`` is asked as well."""
    from mdir_amd import ops
    from mdir_amd.search import knn_join
    x, _, _, self_scores = problem(d)
    rows = device_rows(x, layout)
    want = [rank_order(self_scores[i], np.arange(N, dtype=np.int64)) for i in range(N)]
    want_ids = np.stack([w[0][:KNN] for w in want])
    want_sc = np.stack([w[1][:KNN] for w in want])
    ix = ops.DescriptorIndex(rows.contiguous(), "ND", storage="i8")
    st = ops.join_stats(ix, rows)
    t = ops.knn_bounds(ix, st, ix, st, 0, N, KNN)
    pairs, count = ops.join_candidates_rows(ix, st, ix, st, t, 0, N, N * N)
    assert N * KNN <= count == pairs.numel()
    ids, sc, counts = ops.knn_resolve(rows, rows, pairs, 0, N, KNN)
    np.testing.assert_array_equal(ids.cpu().numpy(), want_ids)
    assert same_bits(sc, want_sc), (d, layout)
    assert (counts.cpu().numpy() >= KNN).all()
    if layout == "contiguous":
        res = knn_join(ix, rows, KNN)
        np.testing.assert_array_equal(res.ids.cpu().numpy(), want_ids)
        assert same_bits(res.scores, want_sc), (d, layout)
    ix.close()
