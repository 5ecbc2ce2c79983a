"""ops.topk_overlap (include/mdx_overlap.h) and search.recall_at on the device against the restatement
(tests/overlap_restatement.py): the int32 counts are compared with ``torch.equal``.  Row lengths on both sides of a wave (63, 64, 65),
of one thread each (1), of several passes of the workgroup (1000) and at the limit (4096), mixed; 1, 3 and 70 queries; 1 and 8 depths
that straddle both lengths; rows that are identical, disjoint, half shared, shuffled, all padding and padded from the middle on (the
queries of a problem cycle through them); ids near 2^31 - 1; the wrapper's refusals."""
import numpy as np
import pytest
import torch

import overlap_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (ka, kb): every size of the issue on each side, mixed; the table is smallest (64 slots) at kb <= 32 and largest (8192) at 4096
SIZES = [(1, 1), (1, 4096), (63, 64), (64, 63), (65, 1000), (1000, 65), (4096, 4096), (4096, 1), (64, 64), (1000, 1000)]


def _run(a, b, depths):
    from mdir_amd import ops
    got = ops.topk_overlap(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), depths)
    assert got.dtype == torch.int32 and tuple(got.shape) == (a.shape[0], len(depths)) and got.is_cuda
    return got.cpu()


@pytest.mark.parametrize("ka,kb", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("t", (1, 8))
def test_counts_equal_the_restatement(ka, kb, t):
    depths = R.straddling(ka, kb, t)
    for nq in (1, 3, 70):
        a, b = R.problem(nq, ka, kb, seed=nq + ka + kb)
        want = torch.from_numpy(R.topk_overlap(a, b, depths))
        assert torch.equal(_run(a, b, depths), want), (nq, depths)
        assert torch.equal(_run(b, a, depths), torch.from_numpy(R.topk_overlap(b, a, depths))), (nq, depths)
    if t == 8 and min(ka, kb) > 1:
        assert int(want[:, -1].max()) == min(ka, kb) and int(want.min()) == 0       # identical / shuffled rows, disjoint rows


@pytest.mark.parametrize("ka,kb", [(65, 64), (1000, 4096)])
def test_ids_near_the_top_of_the_range(ka, kb):
    a, b = R.problem(7, ka, kb, seed=11, high=True)
    assert a.max() > R.TOP - 3 * R.MAX_K and b.max() > R.TOP - 3 * R.MAX_K
    a[0, 0] = b[0, kb - 1] = R.TOP                                # the largest id itself, shared at the two ends
    a[0, 1:][a[0, 1:] == R.TOP] = R.TOP - 3 * R.MAX_K - 1
    b[0, :-1][b[0, :-1] == R.TOP] = R.TOP - 3 * R.MAX_K - 2
    depths = R.straddling(ka, kb, 8)
    want = R.topk_overlap(a, b, depths)
    assert want[0, -1] >= 1 and want[:, -1].max() == min(ka, kb)
    assert torch.equal(_run(a, b, depths), torch.from_numpy(want))


def test_recall_at():
    from mdir_amd import search
    a, b = R.problem(12, 100, 50, seed=5)
    got = search.recall_at(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), [1, 10, 50, 100])
    assert got.dtype == np.float64 and got.shape == (12, 4)
    np.testing.assert_array_equal(got, R.recall_at(a, b, [1, 10, 50, 100]))
    one = search.recall_at(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), 50)
    np.testing.assert_array_equal(one, got[:, 2:3])
    assert np.isnan(got).any() and (got[~np.isnan(got)] <= 1.0).all() and (got == 1.0).any()   # an all-padding query; an identical one


def test_wrapper_refusals():
    from mdir_amd import ops
    ids = torch.arange(12, dtype=torch.int64, device=DEV).reshape(3, 4)
    for depths, msg in (([], "between 1 and 8 depths"), (list(range(1, 10)), "between 1 and 8 depths"), ([0], r"depths\[0\]"),
                        ([2, 1], "ascending"), ([1.5], r"depths\[0\]"), ([True], r"depths\[0\]"), ([1 << 31], "below 2\\^31")):
        with pytest.raises(ValueError, match=msg):
            ops.topk_overlap(ids, ids, depths)
    with pytest.raises(ValueError, match="b must be a contiguous"):
        ops.topk_overlap(ids, ids[:2], [1])
    with pytest.raises(ValueError, match="contiguous"):
        ops.topk_overlap(ids[:, :2], ids, [1])
    with pytest.raises(ValueError, match="must be torch.int64"):
        ops.topk_overlap(ids.to(torch.int32), ids, [1])
    with pytest.raises(ValueError, match="at most OVERLAP_MAX_K"):
        ops.topk_overlap(torch.zeros((1, 4097), dtype=torch.int64, device=DEV), ids[:1], [1])
    big = ids.clone()
    big[1, 2] = 1 << 31
    for a, b in ((big, ids), (ids, big)):
        with pytest.raises(ValueError, match="at or above 2\\^31"):
            ops.topk_overlap(a, b, [4])
    assert torch.equal(ops.topk_overlap(ids, ids, [2, 4]).cpu(), torch.tensor([[2, 4]] * 3, dtype=torch.int32))
