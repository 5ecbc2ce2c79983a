"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the two entry points of the
product-quantised lists of the inverted file: mdx_pq_lut and mdx_lists_pq_scan.  Several shapes each, so that the leftovers of the
largest call are the stale pre-fill of the smaller ones; every caller pointer at the smallest alignment include/mdx_lists_pq.h allows --
1 byte for the codes (off the 16-byte grid: the byte or dword loads of the scan; on it: the 16-byte loads; the same bits), 4 for the
fp32 tensors (the table and the codewords off the 16-byte grid: dword loads), 8 for the int64 vectors; the plan at 16 bytes, refused
below.  The shapes cover the smallest M, an M that is no multiple of 4 and M = 128; member ids of -1 and n, probes outside [0, K) (which
the plan marks invalid) and an offset beyond m are among the inputs.  The oracle is the restatement (tests/pq_restatement.py), bit for
bit."""
import numpy as np
import pytest

import memguard
import pq_restatement as PR
from test_gpu_ivf_memcontract import _lists, _probes
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


def _lut(m_sub, dsub, nq, qlayout, centred):
    def make():
        rng = np.random.default_rng(m_sub + dsub)
        d = m_sub * dsub
        words = rng.standard_normal((m_sub, 256, dsub)).astype(F32)
        queries = rng.standard_normal((nq, d)).astype(F32)
        center = (F32(0.1) * rng.standard_normal(d)).astype(F32) if centred else None
        want = PR.lut(words, queries, center)
        given = np.ascontiguousarray(queries.T) if qlayout == "DN" else queries

        def run(env):
            return {"lut": env.ops.pq_lut(env.put("codewords", words), env.put("queries", given), qlayout,
                                          None if center is None else env.put("center", center))}

        def verify(o):
            bits_equal(o["lut"], want)
        return [(run, verify)]
    return make


def _scan(m_sub, nq, nprobe, sizes):
    """The last offset lies beyond m; ids -1 and n among the members; two probes outside [0, K)."""
    def make():
        rng = np.random.default_rng(m_sub + nq)
        lists, n = len(sizes), sum(sizes)
        members, offsets = _lists(rng, sizes)
        offsets = offsets.copy()
        offsets[-1] = n + 7                                                # clamped to m
        probes = _probes(rng, nq, nprobe, lists)
        codes = rng.integers(0, 256, (n, m_sub)).astype(np.uint8)
        table = rng.standard_normal((nq, m_sub, 256)).astype(F32)
        coarse = rng.standard_normal((nq, nprobe)).astype(F32)
        cap = int(np.sort(sizes)[::-1][:nprobe].sum())
        cands = PR.scan(codes, members, n, offsets, table, coarse, probes, cap)

        def run(env):
            members_t, offsets_t, probes_t = env.put("members", members), env.put("offsets", offsets), env.put("probes", probes)
            plan = env.ops.ivf_plan(probes_t, offsets_t, n, cap)
            cand_scores, cand_ids = env.ops.lists_pq_scan(env.put("codes", codes), members_t, n, offsets_t, env.put("lut", table),
                                                          env.put("coarse", coarse), probes_t, plan, cap)
            return {"cand_scores": cand_scores, "cand_ids": cand_ids}

        def verify(o):
            nans = 0
            for q, (ids, scores) in enumerate(cands):
                bits_equal(o["cand_ids"][q, :len(ids)], ids), bits_equal(o["cand_scores"][q, :len(ids)], scores)
                assert (o["cand_ids"][q, len(ids):] == -1).all() and np.isnan(o["cand_scores"][q, len(ids):]).all()
                nans += int(np.isnan(scores).sum())
            assert nans > 0 and min(len(c[0]) for c in cands) < cap            # an id outside the rows was scanned; a probe was invalid
        return [(run, verify)]
    return make


# entry point -> (builder, the arguments of the largest shape and of the smaller ones, what the header asks of a pointer beyond its
# element's size)
BIG_LISTS = (70, 0, 130, 65, 1)
STAGES = {
    "pq_lut": (_lut, (128, 2, 19, "ND", True), ((1, 5, 3, "DN", False), (3, 20, 9, "DN", True), (2, 300, 2, "ND", False)), {}),
    "lists_pq_scan": (_scan, (128, 19, 3, BIG_LISTS), ((1, 3, 2, (5, 66, 0)), (3, 4, 2, (5, 66, 0)), (4, 5, 2, (5, 66, 0)), (16, 9, 5, BIG_LISTS)),
                      {"workspace_align": 16}),
}

for _entry, (_builder, _big_args, _smaller, _kw) in STAGES.items():
    _big = add("%s[big]" % _entry, Lazy(_builder(*_big_args)), **_kw)
    for _i, _args in enumerate(_smaller):
        _small = add("%s[small%d]" % (_entry, _i), Lazy(_builder(*_args)), larger=_big, **_kw)
        if _big.larger is None:
            _big.larger = _small

# entry point -> its cases.  The census of tests/test_memguard_host.py does not see these entry points (their prototypes are in
# include/mdx_lists_pq.h); tests/test_pq_host.py::test_every_launching_entry_point_has_memory_contract_cases reads this table.
COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")] for entry in STAGES}


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


def test_a_plan_below_16_bytes_is_refused():
    from mdir_amd import ops
    case = next(c for c in CASES if c.name == "lists_pq_scan[small0]")
    try:
        for align in (8, 4):
            assert memguard.refuses(ops, case, DEV, {"ws0": align}), align
        assert not memguard.refuses(ops, case, DEV, {"ws0": 16})
    finally:
        case.release()
