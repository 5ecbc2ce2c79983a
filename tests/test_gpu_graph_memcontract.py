"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of mdx_graph_search and mdx_graph_detours
(include/mdx_graph.h).  Neither has a workspace.  Guard bands around every input and output, the outputs pre-filled 0xFF, 0x00 and with
the leftovers of a larger call, the bytes after the inputs 0xFF (-1: padding, NaN) and 0x00 (the id 0, the score 0: a load past the end
of the graph, the seeds or the lists would find a valid row), and every pointer at its element's alignment -- rows at 4 bytes takes the
scalar path of row_piece.  The graphs hold -1, ids >= n, repeats and self loops; the searches run at the default table size, where
`scored` is as deterministic as the rest."""
import numpy as np
import pytest

import graph_restatement as R
import memguard
from test_gpu_memcontract import WORKSPACE_ALIGN, Lazy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = []


def _add(name, make, larger):
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), larger=larger,
                         workspace_align=WORKSPACE_ALIGN)
    made = Lazy(make)
    case.release = made.release
    CASES.append(case)
    return case


def _search(n, d, nq, deg, S, k, L, W, T, seed, larger=None):
    def make():
        rows, queries, graph, seeds = R.problem(n, d, nq, deg, S, seed)
        want = R.graph_search(R.all_scores(rows, queries), graph, seeds, k, L, W, T)

        def run(env):
            ids, scores, steps, scored = env.ops.graph_search(env.put("rows", rows), env.put("graph", graph), env.put("queries", queries),
                                                              env.put("seeds", seeds), k, L, W, T)
            return {"ids": ids, "scores": scores, "steps": steps, "scored": scored}

        def verify(o):
            np.testing.assert_array_equal(o["ids"], want[0])
            R.same_scores(o["scores"], want[1])
            np.testing.assert_array_equal(o["steps"], want[2])
            assert (o["scored"] <= S + o["steps"] * W * deg).all() and (o["scored"] >= (o["ids"] >= 0).sum(axis=1)).all()
        return [(run, verify)]
    return _add("graph_search[%d x %d nq=%d R=%d S=%d k=%d L=%d W=%d T=%d]" % (n, d, nq, deg, S, k, L, W, T), make, larger)


def _detours(n, k0, seed, larger=None):
    def make():
        rng = np.random.default_rng([seed, n, k0])
        lists = np.stack([rng.permutation(n + 4)[:k0] for _ in range(n)]).astype(np.int64)      # distinct; n .. n + 3 are out of range
        lists[rng.random(lists.shape) < 0.1] = -1
        lists[:, 0] = np.where(lists[:, 0] == 0, 1 % n, lists[:, 0])
        want = R.detours(lists)

        def run(env):
            return {"detours": env.ops.graph_detours(env.put("lists", lists))}

        def verify(o):
            np.testing.assert_array_equal(o["detours"], want)
            assert o["detours"].dtype == np.int32
        return [(run, verify)]
    return _add("graph_detours[%d x %d]" % (n, k0), make, larger)


_big = _search(300, 70, 5, 7, 9, 20, 65, 2, 30, 1)
_big.larger = _search(120, 65, 3, 32, 4, 64, 64, 1, 12, 2, larger=_big)
_search(40, 1, 2, 1, 1, 1, 1, 1, 5, 3, larger=_big)
_search(64, 256, 1, 64, 70, 5, 63, 8, 3, 4, larger=_big)

_wide = _detours(90, 128, 5)
_wide.larger = _detours(70, 65, 6, larger=_wide)
_detours(3, 1, 7, larger=_wide)
_detours(64, 63, 8, larger=_wide)

# entry point -> its cases; tests/test_graph_host.py::test_every_graph_entry_point_is_covered reads this table (the census of
# tests/test_memguard_host.py does not see the prototypes of include/mdx_graph.h)
COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")] for entry in ("graph_search", "graph_detours")}


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
