"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the three entry points of the int8
lists of the inverted file: mdx_lists_i8_encode, mdx_lists_i8_bounds, mdx_lists_i8_scan.  Two shapes each, so that the leftovers of the
larger call are the stale pre-fill of the smaller; every caller pointer at the smallest alignment include/mdx_lists_i8.h allows -- 16
bytes for the codes (refused below), 1 byte for the query codes (off the 16-byte grid: the byte loads of the scan; on it: the 16-byte
loads; the same bits), 4 for the fp32 vectors and the rows (dword loads off the grid), 8 for the int64 vectors and the bounds; the plan at
16 bytes, refused below, at exactly the size the size function says, and refused one byte short.  Member ids of -1 and n, probes
outside [0, K) and an offset beyond m are among the inputs.  The oracle is the restatement (tests/lists_i8_restatement.py), bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import ivf_restatement as IR
import lists_i8_restatement as LR
import memguard
from test_gpu_ivf_memcontract import _lists, _probes
from test_gpu_memcontract import Lazy, bits_equal
from test_rescore_host import bounds_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32

CASES = []


def add(name, made, larger=None, **kw):
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), larger=larger, **kw)
    case.release = made.release
    CASES.append(case)
    return case


def _rows(rng, n, d, ld):
    """Unit-scale normal rows in the first d columns of a wider matrix; one all-zero row."""
    wide = rng.standard_normal((n, ld)).astype(F32)
    wide[n // 2, :d] = 0
    return wide


def _encode(sizes, d, ld):
    """``ld > d``: the rows are the first d columns of a wider matrix."""
    def make():
        rng = np.random.default_rng(d + ld)
        n = sum(sizes)
        members, _ = _lists(rng, sizes)
        wide = _rows(rng, n, d, ld)
        codes, scales = LR.encode(wide[:, :d], members)

        def run(env):
            got_codes, got_scales = env.ops.lists_i8_encode(env.put("rows", wide)[:, :d], env.put("members", members))
            return {"codes": got_codes, "scales": got_scales}

        def verify(o):
            bits_equal(o["codes"], codes), bits_equal(o["scales"], scales)
            assert np.isnan(o["scales"][[1, n - 2]]).all() and not o["codes"][[1, n - 2]].any() and not o["codes"][:, d:].any()
        return [(run, verify)]
    return make


def _bounds(sizes, d, spoil):
    def make():
        rng = np.random.default_rng(d)
        n = sum(sizes)
        members, _ = _lists(rng, sizes, spoil=spoil)
        rows = _rows(rng, n, d, d)
        codes, scales = LR.encode(rows, members)
        ok = (members >= 0) & (members < n)
        s_max, s_min, l_max, flag = bounds_np(rows[members[ok]])
        want = np.array([s_max, s_min, l_max, 0.0], np.float64)
        want[3:].view(np.int32)[0] = 1 if spoil else flag                    # a NaN scale sets the flag

        def run(env):
            return {"bounds": env.ops.lists_i8_bounds(env.put("codes", codes), env.put("scales", scales), d)}

        def verify(o):
            bits_equal(o["bounds"], want)
        return [(run, verify)]
    return make


def _scan(nq, nprobe, sizes, d, centred):
    """``items`` is a bound above the plan's work items; the last offset lies beyond m."""
    def make():
        rng = np.random.default_rng(nq + d)
        lists, n = len(sizes), sum(sizes)
        members, offsets = _lists(rng, sizes)
        offsets = offsets.copy()
        offsets[-1] = n + 7                                                # clamped to m
        probes = _probes(rng, nq, nprobe, lists)
        rows = _rows(rng, n, d, d)
        queries = rng.standard_normal((nq, d)).astype(F32)
        center = (F32(0.1) * rng.standard_normal(d)).astype(F32) if centred else None
        cap = int(np.sort(sizes)[::-1][:nprobe].sum())
        codes, scales = LR.encode(rows, members)
        qcodes, qscales = LR.quantize_np(LR.centred(queries, center))
        scores = LR.i8_scores(rows, queries, center)
        cands = IR.candidates(members, offsets, probes, cap)
        items = IR.plan(probes, offsets, n, cap)[3] + 3

        def run(env):
            members_t, offsets_t = env.put("members", members), env.put("offsets", offsets)
            plan = env.ops.ivf_plan(env.put("probes", probes), offsets_t, n, cap)
            cand_scores, cand_ids = env.ops.lists_i8_scan(env.put("codes", codes), env.put("scales", scales), d, members_t, offsets_t,
                                                          env.put("qcodes", qcodes), env.put("qscales", qscales), plan, nprobe, cap, items)
            return {"cand_scores": cand_scores, "cand_ids": cand_ids}

        def verify(o):
            for q, c in enumerate(cands):
                bits_equal(o["cand_ids"][q, :len(c)], c), bits_equal(o["cand_scores"][q, :len(c)], IR.candidate_scores(scores[q], c))
                assert (o["cand_ids"][q, len(c):] == -1).all() and np.isnan(o["cand_scores"][q, len(c):]).all()
        return [(run, verify)]
    return make


# entry point -> (builder, big arguments, small arguments, what the header asks of a pointer beyond its element's size)
STAGES = {
    "lists_i8_encode": (_encode, ((70, 0, 130, 65, 1), 260, 264), ((5, 9, 0), 5, 5), {"aligns": {"out0": 16}}),
    "lists_i8_bounds": (_bounds, ((70, 0, 130, 65, 1), 260, True), ((5, 9, 0), 5, False), {"aligns": {"codes": 16}}),
    "lists_i8_scan": (_scan, (2 * IR.QUERY_GROUP + 3, 3, (70, 0, 130, 65, 1), 1040, True), (3, 2, (5, 66, 0), 5, False),
                      {"aligns": {"codes": 16}, "workspace_align": 16}),
}

for _entry, (_builder, _big_args, _small_args, _kw) in STAGES.items():
    _big = add("%s[big]" % _entry, Lazy(_builder(*_big_args)), **_kw)
    _big.larger = add("%s[small]" % _entry, Lazy(_builder(*_small_args)), larger=_big, **_kw)

# entry point -> its cases.  The census of tests/test_memguard_host.py does not see these entry points (their prototypes are in
# include/mdx_lists_i8.h); tests/test_lists_i8_host.py::test_every_launching_entry_point_has_memory_contract_cases reads this table.
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


def test_codes_and_plan_below_16_bytes_are_refused():
    from mdir_amd import ops
    for name, buffer in (("lists_i8_encode[small]", "out0"), ("lists_i8_bounds[small]", "codes"), ("lists_i8_scan[small]", "codes"),
                         ("lists_i8_scan[small]", "ws0")):
        case = next(c for c in CASES if c.name == name)
        try:
            for align in (8, 4):
                assert memguard.refuses(ops, case, DEV, {buffer: align}), (name, buffer, align)
            assert not memguard.refuses(ops, case, DEV, {buffer: 16})
        finally:
            case.release()


def test_plan_exact_size_and_one_byte_less():
    """The wrapper hands the library exactly mdx_ivf_plan_workspace bytes (the guarded runs above); one byte less is MDX_ERR_WORKSPACE
    and nothing is written."""
    from mdir_amd import _lib
    h = _lib.lib()
    rng = np.random.default_rng(0)
    sizes = (40, 0, 70)
    lists, n, d, nq, nprobe, cap = len(sizes), sum(sizes), 70, 4, 2, 110
    members, offsets = _lists(rng, sizes, spoil=False)
    probes = np.stack([rng.permutation(lists)[:nprobe] for _ in range(nq)]).astype(np.int64)
    rows, queries = rng.standard_normal((n, d)).astype(F32), rng.standard_normal((nq, d)).astype(F32)
    codes, scales = LR.encode(rows, members)
    qcodes, qscales = LR.quantize_np(queries)
    t = {name: torch.from_numpy(a).to(DEV) for name, a in (("members", members), ("offsets", offsets), ("probes", probes), ("codes", codes),
                                                           ("scales", scales), ("qcodes", qcodes), ("qscales", qscales))}
    need = h.mdx_ivf_plan_workspace(nq, nprobe, lists)
    assert need == 6 * 256
    plan = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    cand_scores, cand_ids = torch.full((nq, cap), 7.0, device=DEV), torch.full((nq, cap), 7, dtype=torch.int64, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())

    def call_scan(nbytes):
        return h.mdx_lists_i8_scan(p(t["codes"]), p(t["scales"]), n, d, p(t["members"]), p(t["offsets"]), lists, p(t["qcodes"]), p(t["qscales"]),
                                   nq, nprobe, p(plan), nbytes, cap, 16, p(cand_scores), p(cand_ids), None)
    assert call_scan(need - 1) == -4 and h.mdx_last_error().startswith(b"mdx_lists_i8_scan: workspace")
    torch.cuda.synchronize()
    assert bool((plan == 0xA5).all()) and bool((cand_scores == 7.0).all()) and bool((cand_ids == 7).all())
    assert h.mdx_ivf_plan(p(t["probes"]), nq, nprobe, p(t["offsets"]), lists, n, cap, p(plan), need, None) == 0 and call_scan(need) == 0
    torch.cuda.synchronize()
    scores = LR.i8_scores(rows, queries)
    for q, c in enumerate(IR.candidates(members, offsets, probes, cap)):
        bits_equal(cand_ids[q, :len(c)].cpu().numpy(), c), bits_equal(cand_scores[q, :len(c)].cpu().numpy(), IR.candidate_scores(scores[q], c))
        assert bool((cand_ids[q, len(c):] == -1).all()) and bool(torch.isnan(cand_scores[q, len(c):]).all())
