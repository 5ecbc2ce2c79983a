"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of mdx_topk_overlap
(include/mdx_overlap.h).  The lists are the case's inputs, the counts its only output and there is no workspace: guard bands around
all three, the output pre-filled 0xFF, 0x00 and with the leftovers of the largest call, the bytes after the lists 0xFF (-1: padding)
and 0x00 (the id 0, which the lists of these cases hold at position 0: a load past the end of a row would count it), and every
pointer at its element's alignment.  The deepest depth lies below, at and beyond the row lengths, so the clamp of every row is used."""
import numpy as np
import pytest

import memguard
import overlap_restatement as R
from test_gpu_memcontract import WORKSPACE_ALIGN, Lazy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = []


def _case(nq, ka, kb, depths, seed, larger=None):
    def make():
        a, b = R.problem(nq, ka, kb, seed)
        # the id 0 at the head of every row that is not all padding: what a read past the end of a zero-tailed list would find
        for m in (a, b):
            live = m[:, 0] >= 0
            m[m == 0] = 3 * R.MAX_K + 1
            m[live, 0] = 0

        def run(env):
            return {"counts": env.ops.topk_overlap(env.put("a", a), env.put("b", b), depths)}

        def verify(o):
            np.testing.assert_array_equal(o["counts"], R.topk_overlap(a, b, depths))
            assert o["counts"].dtype == np.int32
        return [(run, verify)]
    name = "topk_overlap[%d x %d|%d depths=%s]" % (nq, ka, kb, depths)
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), larger=larger,
                         workspace_align=WORKSPACE_ALIGN)
    made = Lazy(make)
    case.release = made.release
    CASES.append(case)
    return case


_big = _case(9, 1000, 4096, [10, 999, 1000, 1001, 4096, 5000], 1)
_big.larger = _case(7, 65, 63, [1, 63, 64, 65, 66], 2, larger=_big)
_case(3, 4096, 1, [1, 2, 4096], 3, larger=_big)
_case(1, 1, 1, [1], 4, larger=_big)
_case(5, 64, 1000, [50], 5, larger=_big)            # the deepest depth below both lengths: the tails of the rows are never read

# entry point -> its cases; tests/test_overlap_host.py::test_every_overlap_entry_point_is_covered reads this table (the census of
# tests/test_memguard_host.py does not see the prototype of include/mdx_overlap.h)
COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")] for entry in ("topk_overlap",)}


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
