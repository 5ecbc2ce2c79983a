"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the three launching entry points of
the inverted file: mdx_ivf_plan, mdx_ivf_scan, mdx_ivf_select.  Two shapes each, so that the leftovers of the larger call are the stale
pre-fill of the smaller; every caller pointer at the smallest alignment include/mdx_ivf.h allows -- 4 bytes for the fp32 matrices (off
the 16-byte grid: the dword loads of the scan; on it: the 16-byte loads; the same bits), 8 for the int64 vectors; the plan at 16
bytes, refused below, at exactly the size the size function says, and refused one byte short.  The data are small integers: every
score is exact in any order (the idea of tests/lattice.py), so the oracle is an integer product and the restatement
(tests/ivf_restatement.py), bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import ivf_restatement as IR
import kmeans_restatement as KR
import memguard
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


def _lists(rng, sizes, spoil=True):
    """(members, offsets) of lists of the given sizes over shuffled rows; an id of -1 and an id of n among the members."""
    n = sum(sizes)
    members, offsets = KR.csr(rng.permutation(np.repeat(np.arange(len(sizes)), sizes)), len(sizes))
    members = members.copy()
    if spoil:
        members[[1, n - 2]] = (-1, n)
    return members, offsets


def _probes(rng, nq, nprobe, lists):
    """Distinct lists per query, one probe outside [0, K) in the first and in the last query."""
    probes = np.stack([rng.permutation(lists)[:nprobe] for _ in range(nq)]).astype(np.int64)
    probes[0, 0], probes[-1, -1] = -1, lists
    return probes


def _exact(rows, queries, center=None):
    """The scores of integer data: exact in fp32 in any order, +0 where they are zero."""
    q = queries.astype(np.int64) - (0 if center is None else center.astype(np.int64))
    acc = q @ rows.astype(np.int64).T
    assert (np.abs(q) @ np.abs(rows.astype(np.int64)).T).max() < (1 << 24)
    return acc.astype(F32)


def _plan_outputs(ops, plan, nq, nprobe, lists):
    """The defined extent of a plan: base, count, first, item, and the entries sorted inside every list."""
    views = {k: v.cpu().numpy().copy() for k, v in ops.ivf_plan_views(plan, nq, nprobe, lists).items()}
    first = views["first"]
    entry = views.pop("entry")
    views["entries"] = np.concatenate([np.sort(entry[first[l]:first[l + 1]]) for l in range(lists)] + [np.empty(0, np.int64)])
    return views


def _plan(nq, nprobe, sizes, cap):
    def make():
        rng = np.random.default_rng(nq + nprobe)
        lists, m = len(sizes), sum(sizes)
        _, offsets = _lists(rng, sizes)
        offsets = offsets.copy()
        offsets[-1] = m + 7                                                # clamped to m
        probes = _probes(rng, nq, nprobe, lists)
        base, count, entries, items = IR.plan(probes, offsets, m, cap)

        def run(env):
            plan = env.ops.ivf_plan(env.put("probes", probes), env.put("offsets", offsets), m, cap)
            return _plan_outputs(env.ops, plan, nq, nprobe, lists)

        def verify(o):
            bits_equal(o["base"], base), bits_equal(o["count"], count)
            bits_equal(o["first"], np.concatenate([[0], np.cumsum([len(e) for e in entries])]).astype(np.int64))
            bits_equal(o["entries"], np.array([e for es in entries for e in es], np.int64))
            assert o["item"][0] == 0 and o["item"][-1] == items and (np.diff(o["item"]) >= 0).all()
        return [(run, verify)]
    return make


def _scan(nq, nprobe, sizes, d, ld, qlayout, centred):
    """``ld > d``: the rows are the first d columns of a wider matrix.  ``items`` is a bound above the plan's work items."""
    def make():
        rng = np.random.default_rng(nq + d)
        lists, n = len(sizes), sum(sizes)
        members, offsets = _lists(rng, sizes)
        probes = _probes(rng, nq, nprobe, lists)
        wide = rng.integers(-3, 4, (n, ld)).astype(F32)
        queries = rng.integers(-3, 4, (nq, d)).astype(F32)
        center = rng.integers(-2, 3, d).astype(F32) if centred else None
        cap = int(np.sort(sizes)[::-1][:nprobe].sum())
        scores = _exact(wide[:, :d], queries, center)
        cands = IR.candidates(members, offsets, probes, cap)
        items = IR.plan(probes, offsets, n, cap)[3] + 3
        given = np.ascontiguousarray(queries.T) if qlayout == "DN" else queries

        def run(env):
            members_t, offsets_t = env.put("members", members), env.put("offsets", offsets)
            plan = env.ops.ivf_plan(env.put("probes", probes), offsets_t, n, cap)
            cand_scores, cand_ids = env.ops.ivf_scan(env.put("rows", wide)[:, :d], members_t, offsets_t, env.put("queries", given), plan, nprobe,
                                                     cap, items, qlayout, None if center is None else env.put("center", center))
            return {"cand_scores": cand_scores, "cand_ids": cand_ids}

        def verify(o):
            for q, c in enumerate(cands):
                bits_equal(o["cand_ids"][q, :len(c)], c), bits_equal(o["cand_scores"][q, :len(c)], IR.candidate_scores(scores[q], c))
                assert (o["cand_ids"][q, len(c):] == -1).all() and np.isnan(o["cand_scores"][q, len(c):]).all()
        return [(run, verify)]
    return make


def _select(nq, count, k):
    """One list of ``count`` members probed by every query but the last, which probes the empty list: scores of few distinct values,
    -0, NaN and infinities among them; ids in no order."""
    def make():
        rng = np.random.default_rng(count + k)
        offsets = np.array([0, count, count], np.int64)
        probes = np.zeros((nq, 1), np.int64)
        probes[-1] = 1
        ids = np.stack([rng.permutation(count).astype(np.int64) for _ in range(nq)])
        sc = rng.integers(-2, 3, (nq, count)).astype(F32)
        sc[rng.random((nq, count)) < 0.1] = F32(-0.0)
        sc[rng.random((nq, count)) < 0.02] = F32(np.nan)
        sc[0, :2] = (np.inf, -np.inf)
        sc[1 % nq] = rng.standard_normal(count).astype(F32)
        want = [IR.select(sc[q, :c], ids[q, :c], k) for q, c in enumerate([count] * (nq - 1) + [0])]

        def run(env):
            plan = env.ops.ivf_plan(env.put("probes", probes), env.put("offsets", offsets), count, count)
            out_ids, out_scores = env.ops.ivf_select(env.put("cand_scores", sc), env.put("cand_ids", ids), plan, 1, 2, k)
            return {"ids": out_ids, "scores": out_scores}

        def verify(o):
            bits_equal(o["ids"], np.stack([w[0] for w in want])), bits_equal(o["scores"], np.stack([w[1] for w in want]))
        return [(run, verify)]
    return make


# entry point -> (builder, big arguments, small arguments)
STAGES = {
    "ivf_plan": (_plan, (2 * IR.QUERY_GROUP + 3, 3, (70, 0, 130, 65, 1), 200), (3, 2, (5, 9, 0), 12)),
    "ivf_scan": (_scan, (2 * IR.QUERY_GROUP + 3, 3, (70, 0, 130, 65, 1), 260, 264, "ND", True), (3, 2, (5, 66, 0), 5, 5, "DN", False)),
    "ivf_select": (_select, (3, 5000, 300), (2, 70, 100)),
}

for _entry, (_builder, _big_args, _small_args) in STAGES.items():
    _big = add("%s[big]" % _entry, Lazy(_builder(*_big_args)), workspace_align=16)
    _big.larger = add("%s[small]" % _entry, Lazy(_builder(*_small_args)), larger=_big, workspace_align=16)

# entry point -> its cases.  The census of tests/test_memguard_host.py does not see these entry points (their prototypes are in
# include/mdx_ivf.h); tests/test_ivf_host.py::test_every_launching_entry_point_has_memory_contract_cases reads this table instead.
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


def test_plan_below_16_bytes_is_refused():
    from mdir_amd import ops
    for name in ("ivf_plan[small]", "ivf_scan[small]", "ivf_select[small]"):
        case = next(c for c in CASES if c.name == name)
        try:
            assert memguard.workspace_names(ops, case, DEV) == ["ws0"]
            for align in (8, 4):
                assert memguard.refuses(ops, case, DEV, {"ws0": align}), (name, align)
            assert not memguard.refuses(ops, case, DEV, {"ws0": 16})
        finally:
            case.release()


def test_plan_exact_size_and_one_byte_less():
    """The wrappers hand the library exactly mdx_ivf_plan_workspace bytes (the guarded runs above); one byte less is MDX_ERR_WORKSPACE
    in all three calls and nothing is written."""
    from mdir_amd import _lib, ops
    h = _lib.lib()
    rng = np.random.default_rng(0)
    sizes = (40, 0, 70)
    lists, n, d, nq, nprobe, cap, k = len(sizes), sum(sizes), 5, 4, 2, 110, 9
    members, offsets = _lists(rng, sizes, spoil=False)
    probes = np.stack([rng.permutation(lists)[:nprobe] for _ in range(nq)]).astype(np.int64)
    rows, queries = rng.integers(-3, 4, (n, d)).astype(F32), rng.integers(-3, 4, (nq, d)).astype(F32)
    t = {name: torch.from_numpy(a).to(DEV) for name, a in (("members", members), ("offsets", offsets), ("probes", probes), ("rows", rows),
                                                           ("queries", queries))}
    need = h.mdx_ivf_plan_workspace(nq, nprobe, lists)
    assert need == 6 * 256
    plan = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    cand_scores, cand_ids = torch.full((nq, cap), 7.0, device=DEV), torch.full((nq, cap), 7, dtype=torch.int64, device=DEV)
    out_ids, out_scores = torch.full((nq, k), 7, dtype=torch.int64, device=DEV), torch.full((nq, k), 7.0, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())

    def call_plan(nbytes):
        return h.mdx_ivf_plan(p(t["probes"]), nq, nprobe, p(t["offsets"]), lists, n, cap, p(plan), nbytes, None)

    def call_scan(nbytes):
        return h.mdx_ivf_scan(p(t["rows"]), n, d, d, p(t["members"]), n, p(t["offsets"]), lists, p(t["queries"]), nq, 1, None, nprobe, p(plan),
                              nbytes, cap, 16, p(cand_scores), p(cand_ids), None)

    def call_select(nbytes):
        return h.mdx_ivf_select(p(cand_scores), p(cand_ids), nq, cap, nprobe, lists, p(plan), nbytes, k, p(out_ids), p(out_scores), None)
    for call, name in ((call_plan, b"mdx_ivf_plan"), (call_scan, b"mdx_ivf_scan"), (call_select, b"mdx_ivf_select")):
        assert call(need - 1) == -4 and h.mdx_last_error().startswith(name + b": workspace")
    torch.cuda.synchronize()
    assert bool((plan == 0xA5).all()) and bool((cand_scores == 7.0).all()) and bool((cand_ids == 7).all())
    assert bool((out_ids == 7).all()) and bool((out_scores == 7.0).all())
    assert call_plan(need) == 0 and call_scan(need) == 0 and call_select(need) == 0
    torch.cuda.synchronize()
    want_ids, want_sc, scanned = IR.search(members, offsets, probes, _exact(rows, queries), k, cap)
    bits_equal(out_ids.cpu().numpy(), want_ids), bits_equal(out_scores.cpu().numpy(), want_sc)
    bits_equal(ops.ivf_plan_views(plan, nq, nprobe, lists)["count"].cpu().numpy(), scanned)
