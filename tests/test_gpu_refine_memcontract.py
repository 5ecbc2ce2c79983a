"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of mdx_refine_i8, the entry point that
scores shortlists on int8 codes kept in list order.  Three shapes, so that the leftovers of the largest call are the stale pre-fill of
the smaller ones; every caller pointer at the smallest alignment include/mdx_refine.h allows -- 16 bytes for the codes (refused below),
1 byte for the query codes (off the 16-byte grid: the byte loads; on it, where d % 16 == 0: the 16-byte loads; the same bits), 4 for
the fp32 vectors, 8 for the int64 ones, 16 for the workspace, at exactly the size the size function says.  Ids outside [0, n), ids that
are not stored (where = -1, m, 2^40), a repeated padding id, a position with a NaN scale and one with scale 0 are among the inputs.
The oracle is the restatement (tests/refine_restatement.py), bit for bit."""
import numpy as np
import pytest

import lists_i8_restatement as LI
import memguard
import refine_restatement as RR
from test_gpu_memcontract import Lazy, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32

CASES = []


def add(name, made, larger=None, **kw):
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), larger=larger, **kw)
    case.release = made.release
    CASES.append(case)
    return case


def problem(seed, nq, s, m, n, d):
    """The inputs of one call on the host: (codes, scales, where, qcodes, qscales, ids) with the special values of the module
    docstring; m < n, so some ids are not stored."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d)).astype(F32)
    members = np.sort(rng.permutation(n)[:m]).astype(np.int64)
    rows[members[m // 2]] = 0                                               # scale 0
    codes, scales = LI.encode(rows, members)
    if m > 2:
        codes[m // 3], scales[m // 3] = 0, np.nan                           # what the encoder leaves for an id it refuses
    where = RR.where_of(members, n)
    gone = np.flatnonzero(where < 0)
    where[gone[::3]], where[gone[1::3]] = m, 1 << 40                        # not stored, said in two more ways
    qcodes, qscales = LI.quantize_np(rng.standard_normal((nq, d)).astype(F32))
    ids = rng.integers(0, n, (nq, s)).astype(np.int64)
    for q in range(nq):
        ids[q, :min(s, n)] = rng.permutation(n)[:min(s, n)]
    if s >= 8:
        ids[:, 1], ids[:, 3], ids[:, 4], ids[:, -1], ids[:, -2] = -1, n, n + 5, n, n
    return codes, scales, where, qcodes, qscales, ids


def _refine(nq, s, m, n, d):
    def make():
        given = problem(nq + s + d, nq, s, m, n, d)
        want = RR.refine(given[0], given[1], d, *given[2:])

        def run(env):
            t = [env.put(name, a) for name, a in zip(("codes", "scales", "where", "qcodes", "qscales", "ids"), given)]
            out_ids, out_scores = env.ops.refine_i8(t[0], t[1], d, *t[2:])
            return {"ids": out_ids, "scores": out_scores}

        def verify(o):
            bits_equal(o["ids"], want[0], "ids"), bits_equal(o["scores"], want[1], "scores")
            assert np.isnan(o["scores"][:, -1]).all()
        return [(run, verify)]
    return make


# (nq, S, m, n, d): the largest first; d = 1040 takes two slices of a lane and the byte loads of the query, d = 64 the 16-byte loads
SHAPES = ((3, 257, 150, 200, 1040), (2, 65, 40, 70, 64), (1, 9, 5, 11, 5))
_KW = {"aligns": {"codes": 16}, "workspace_align": 16}
_big = add("refine_i8[big]", Lazy(_refine(*SHAPES[0])), **_KW)
for _i, _shape in enumerate(SHAPES[1:]):
    _small = add("refine_i8[small%d]" % _i, Lazy(_refine(*_shape)), larger=_big, **_KW)
    if _big.larger is None:
        _big.larger = _small

# entry point -> its cases.  The census of tests/test_memguard_host.py does not see this entry point (its prototype is in
# include/mdx_refine.h); tests/test_refine_host.py::test_every_launching_entry_point_has_memory_contract_cases reads this table.
COVERED = {"refine_i8": list(CASES)}


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


def test_codes_and_workspace_below_16_bytes_are_refused():
    from mdir_amd import ops
    case = next(c for c in CASES if c.name == "refine_i8[small1]")
    try:
        for buffer in ("codes", "ws0"):
            for align in (8, 4):
                assert memguard.refuses(ops, case, DEV, {buffer: align}), (buffer, align)
            assert not memguard.refuses(ops, case, DEV, {buffer: 16})
    finally:
        case.release()
