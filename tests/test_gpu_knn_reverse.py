"""ops.knn_reverse_merge (include/mdx_knn_reverse.h) on the device against the restatement (tests/knn_reverse_restatement.py): ids,
score bits and ``gained``.  Every case runs twice and the two runs must hold the same bytes -- the order in which offers arrive in
the offer buffer is the atomics', and must not show."""
import numpy as np
import pytest

import ivf_restatement as IR
import knn_reverse_restatement as KR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
NAN = np.nan


def _foreign(n, k, seed):
    """Random lists with the ids -5 and n written over entries of some rows (the scores stay): padding wherever they stand."""
    ids, sc = KR.random_lists(n, k, seed)
    rng = np.random.default_rng(seed)
    for i in rng.permutation(n)[:n // 3]:
        a, b = rng.permutation(k)[:2]
        ids[i, a], ids[i, b] = -5, n
    return ids, sc


def _ties_on_the_kth():
    """Full rows whose last entry ties an offer on the score: the offer wins where its id is smaller, and loses where it is larger."""
    lost = ([[1, 2], [0, 2], [0, 1], [0, 4], [0, 3]], [[0.9, 0.8], [0.9, 0.1], [0.8, 0.1], [0.8, 0.2], [0.85, 0.2]])
    won = ([[3, 4], [2, 3], [4, 5], [0, 1], [2, 0], [2, 0]], [[0.5, 0.4], [0.8, 0.3], [0.9, 0.8], [0.5, 0.3], [0.9, 0.4], [0.8, 0.1]])
    return [(np.array(i, np.int64), np.array(s, F32)) for i, s in (lost, won)]


def _special():
    ids = [[0, 1, -5], [1, 5, 2], [2, -1, -1], [3, 0, 1], [4, 0, -1]]
    sc = [[1.0, -0.0, 0.3], [1.0, 0.7, 0.0], [1.0, NAN, NAN], [1.0, 0.0, NAN], [1.0, NAN, NAN]]
    return np.array(ids, np.int64), np.array(sc, F32)


CASES = {
    "random n=300 k=8": lambda: KR.random_lists(300, 8, 1),
    "k=1": lambda: KR.random_lists(150, 1, 2),
    "k=128 n=200": lambda: KR.random_lists(200, 128, 3, share=0.8),
    "k=65 n=130": lambda: KR.random_lists(130, 65, 4, share=0.7),          # one entry in the second half of the lanes' pairs
    "n=1": lambda: (np.array([[0]], np.int64), np.array([[1.0]], F32)),
    "n=1 padded": lambda: (np.array([[-1, -1, -1]], np.int64), np.array([[NAN] * 3], F32)),
    "hub n=3000 k=4": lambda: KR.hub_lists(3000),
    "padding that offers fill": lambda: KR.random_lists(300, 8, 5, share=0.02),
    "tie on the k-th, lost": lambda: _ties_on_the_kth()[0],
    "tie on the k-th, won": lambda: _ties_on_the_kth()[1],
    "zeros, NaN, infinity": lambda: KR.random_lists(200, 6, 6, special=True),
    "hand-written special values": _special,
    "ids -5 and n": lambda: _foreign(240, 7, 7),
}


@pytest.mark.parametrize("name", list(CASES))
def test_merge_equals_the_restatement(name):
    import torch
    from mdir_amd import ops
    ids, sc = CASES[name]()
    want = KR.merge(ids, sc)
    t_ids, t_sc = torch.from_numpy(ids).to(DEV), torch.from_numpy(sc).to(DEV)
    runs = []
    for _ in range(2):
        got = [t.cpu().numpy() for t in ops.knn_reverse_merge(t_ids, t_sc)]
        assert got[0].dtype == np.int64 and got[1].dtype == F32 and got[2].dtype == np.int32
        runs.append(got)
    for got in runs:
        for g, w in zip(got, want):
            IR.same_bits(g, w)
    for a, b in zip(*runs):
        IR.same_bits(a, b)
    IR.same_bits(t_ids.cpu().numpy(), ids), IR.same_bits(t_sc.cpu().numpy(), sc)       # the inputs are read only
    if name.startswith("hub"):
        assert want[0][0].tolist() == [49, 99, 149, 199] and want[2][0] == 4
        counts = ops.knn_reverse_count(t_ids, t_sc).cpu().numpy()
        IR.same_bits(counts, KR.entering(ids, sc)[0])
        assert counts[0] == sum(1 for i in range(5, 3000) if i % 50 > 1)       # what precedes row 0's last entry (1, 1.0): 45 tiles
    if name.startswith("random") or name.startswith("padding"):
        assert want[2].sum() > 0


def test_the_three_stages_on_their_own():
    """count, the prefix sum, fill and apply, each against the restatement: the counts, the offsets, the offers of every segment as a
    set, and the merge of a buffer filled by hand in another order."""
    import torch
    from mdir_amd import ops
    ids, sc = KR.random_lists(300, 8, 11)
    counts, offsets, offers = KR.entering(ids, sc)
    assert 0 < counts.sum() < sum(len(v) for v in KR.offers(ids, sc).values())   # something enters, and something is dropped
    t_ids, t_sc = torch.from_numpy(ids).to(DEV), torch.from_numpy(sc).to(DEV)
    got_counts = ops.knn_reverse_count(t_ids, t_sc)
    IR.same_bits(got_counts.cpu().numpy(), counts)
    got_offsets = ops.knn_reverse_offsets(got_counts)
    IR.same_bits(got_offsets.cpu().numpy(), offsets)
    buf = ops.knn_reverse_fill(t_ids, t_sc, got_offsets)
    assert tuple(buf.shape) == (300 * 8,) and buf.dtype == torch.int64
    IR.same_bits(KR.sorted_segments(buf.cpu().numpy(), offsets), offers)
    # segments reversed, in a buffer of exactly the total
    mine = offers.copy()
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        mine[lo:hi] = mine[lo:hi][::-1]
    got = ops.knn_reverse_apply(t_ids, t_sc, got_offsets, torch.from_numpy(mine.view(np.int64).reshape(-1)).to(DEV))
    for g, w in zip(got, KR.merge(ids, sc)):
        IR.same_bits(g.cpu().numpy(), w)
    # a capacity below the total: nothing is written beyond it (the guard bands of the memory contract see that); here the call runs
    short = ops.knn_reverse_fill(t_ids, t_sc, got_offsets, capacity=7)
    assert tuple(short.shape) == (7,)
    torch.cuda.synchronize()
