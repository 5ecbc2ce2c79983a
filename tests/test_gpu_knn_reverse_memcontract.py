"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the three entry points of
include/mdx_knn_reverse.h.  Three inputs each, so that the leftovers of the largest call are the stale pre-fill of the smaller ones:
the hub of tests/knn_reverse_restatement.py (one row offered thousands of entries: many tiles, and the longest segment), random lists
with ties, foreign ids and padding, and a tiny one.  Every pointer lies at the alignment of its element, which is all the header asks,
and every buffer has exactly its size -- the offer buffer exactly n k entries, where the wrapper sizes it, and exactly the number of
offers where the test fills it by hand.  The oracle is the restatement, bit for bit; a segment of the offer buffer is compared sorted,
since the order inside one is that of atomic tickets."""
import numpy as np
import pytest

import knn_reverse_restatement as KR
import memguard
from test_gpu_memcontract import Lazy, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32

CASES = []
COVERED = {}


def add(entry, name, made, larger=None):
    case = memguard.Case("%s[%s]" % (entry, name), lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), larger=larger)
    case.release = made.release
    CASES.append(case)
    COVERED.setdefault(entry, []).append(case)
    return case


def _mixed(n, k, seed):
    """Random lists with ties; a third of the rows hold the ids -5 and n, and the last rows are short (padding that offers fill)."""
    ids, sc = KR.random_lists(n, k, seed)
    rng = np.random.default_rng(seed)
    if k >= 2:
        for i in rng.permutation(n)[:n // 3]:
            a, b = rng.permutation(k)[:2]
            ids[i, a], ids[i, b] = -5, n
    ids[-n // 8:, k // 2:], sc[-n // 8:, k // 2:] = -1, np.nan
    return ids, sc


INPUTS = {"hub": lambda: KR.hub_lists(3000), "mixed": lambda: _mixed(260, 9, 21), "tiny": lambda: _mixed(9, 1, 22)}


def _count(which):
    def make():
        ids, sc = INPUTS[which]()
        want = KR.entering(ids, sc)[0]

        def run(env):
            return {"counts": env.ops.knn_reverse_count(env.put("ids", ids), env.put("scores", sc))}

        def verify(o):
            bits_equal(o["counts"], want, "counts")
        return [(run, verify)]
    return make


def _fill(which):
    def make():
        ids, sc = INPUTS[which]()
        _, offsets, want = KR.entering(ids, sc)

        def run(env):
            buf = env.ops.knn_reverse_fill(env.put("ids", ids), env.put("scores", sc), env.put("offsets", offsets))
            assert buf.numel() == ids.size                                    # the bound n k, and not an entry more
            return {"offers": KR.sorted_segments(buf.cpu().numpy(), offsets)}

        def verify(o):
            bits_equal(o["offers"], want, "offers")
        return [(run, verify)]
    return make


def _merge(which, by_hand):
    """``by_hand``: mdx_knn_reverse_merge alone on an offer buffer of exactly the number of offers, its segments reversed; otherwise
    the three calls as ops.knn_reverse_merge chains them, every buffer between them guarded."""
    def make():
        ids, sc = INPUTS[which]()
        want = KR.merge(ids, sc)
        _, offsets, offers = KR.entering(ids, sc)
        for lo, hi in zip(offsets[:-1], offsets[1:]):
            offers[lo:hi] = offers[lo:hi][::-1]
        packed = offers.view(np.int64).reshape(-1)

        def run(env):
            t_ids, t_sc = env.put("ids", ids), env.put("scores", sc)
            if by_hand:
                got = env.ops.knn_reverse_apply(t_ids, t_sc, env.put("offsets", offsets), env.put("offers", packed))
            else:
                got = env.ops.knn_reverse_merge(t_ids, t_sc)
            return dict(zip(("ids", "scores", "gained"), got))

        def verify(o):
            for name, w in zip(("ids", "scores", "gained"), want):
                bits_equal(o[name], w, name)
        return [(run, verify)]
    return make


for _entry, _builder in (("knn_reverse_count", _count), ("knn_reverse_fill", _fill), ("knn_reverse_merge", lambda w: _merge(w, False))):
    _big = add(_entry, "hub", Lazy(_builder("hub")))
    for _which in ("mixed", "tiny"):
        _small = add(_entry, _which, Lazy(_builder(_which)), larger=_big)
        if _big.larger is None:
            _big.larger = _small
add("knn_reverse_merge", "mixed, by hand", Lazy(_merge("mixed", True)), larger=COVERED["knn_reverse_merge"][0])
add("knn_reverse_merge", "hub, by hand", Lazy(_merge("hub", True)), larger=COVERED["knn_reverse_merge"][1])


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_memory_contract(case):
    from mdir_amd import ops
    log = []
    assert case.larger is not None and case.larger is not case
    try:
        memguard.run_contract(ops, case, DEV, alignment_run=True, log=log.append)
        assert "stale" in log and any(step.startswith("align ") and step.endswith("same bits") for step in log), log
    finally:
        case.release()
        case.larger.release()
        print("%s: %s" % (case.name, "; ".join(log)))

