"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the three entry points of the
exact kNN join: mdx_knn_bounds, mdx_join_candidates_rows, mdx_knn_resolve.  Two shapes each, so that the leftovers of the larger
call are the stale pre-fill of the smaller; every caller pointer at the smallest alignment include/mdx.h allows (the stats at 16
bytes, the workspaces at 16, everything else at its element size).  No tolerance is new: the oracles are the exact chain of
oracle/chain.py and the float64 restatement of test_knn_join_host.py."""
import numpy as np
import pytest
import torch

import memguard
from oracle import chain as OC
from test_gpu_memcontract import WORKSPACE_ALIGN, Lazy, _join_rows, bits_equal
from test_knn_join_host import rank_order, thresholds_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
INDEX_ALIGNS = {"out0": 256, "out1": 16}        # the int8 index's own memory and the stats (include/mdx.h "Alignment")

CASES = []


def add(name, made, larger=None):
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), aligns=INDEX_ALIGNS,
                         larger=larger, workspace_align=WORKSPACE_ALIGN)
    case.release = made.release
    CASES.append(case)
    return case


def _bounds_case(n, d, lo, hi, k, slices, larger=None):
    def make():
        x = _join_rows(n, d, n + d)

        def run(env):
            ops = env.ops
            ix = ops.DescriptorIndex(env.put("vecs", x), "ND", storage="i8")
            st = ops.join_stats(ix, env.put("rows", x))
            t = ops.knn_bounds(ix, st, ix, st, lo, hi, k, slices)
            torch.cuda.synchronize()
            ix.close()
            return {"t": t}

        def verify(o):
            exact = OC.gemm_nt_chain(x[lo:hi], x)
            kth = np.take_along_axis(exact, rank_order(exact)[:, k - 1:k], axis=1)[:, 0]
            t64 = thresholds_np(x[lo:hi], x, k)[0]
            t = o["t"]
            assert t.shape == (hi - lo,) and np.isfinite(t).all()
            assert (t <= kth).all()                                            # a lower bound of the exact k-th score
            assert (t <= t64 + 1e-12).all() and (t64 - t <= 1e-5).all()        # the float64 restatement, rounded downwards in fp32
        return [(run, verify)]
    return add("knn_bounds[%dx%d rows %d..%d k=%d slices=%d]" % (n, d, lo, hi, k, slices), Lazy(make), larger)


_kb_big = _bounds_case(400, 100, 0, 400, 10, 0)
_kb_big.larger = _bounds_case(300, 64, 128, 300, 7, 2, larger=_kb_big)
_bounds_case(131, 7, 0, 131, 3, 1, larger=_kb_big)
_bounds_case(131, 7, 128, 131, 64, 0, larger=_kb_big)


def _rows_case(n, d, lo, hi, capacity, larger=None):
    """capacity: a number or "count" (resolved inside the run from a first call with capacity 0)."""
    def make():
        x = _join_rows(n, d, n + d)
        rng = np.random.default_rng(n)
        taus = rng.choice(np.array([0.5, 0.8, 0.95, 2.0], F32), hi - lo)
        taus[1] = -np.inf                                                      # every pair of the row
        taus[2] = np.nan

        def run(env):
            ops = env.ops
            ix = ops.DescriptorIndex(env.put("vecs", x), "ND", storage="i8")
            st = ops.join_stats(ix, env.put("rows", x))
            tau = env.put("taus", taus)
            _, count = ops.join_candidates_rows(ix, st, ix, st, tau, lo, hi, 0)
            cap = count if capacity == "count" else capacity
            pairs, count2 = ops.join_candidates_rows(ix, st, ix, st, tau, lo, hi, cap)
            assert count2 == count and pairs.numel() == min(count, cap), (count, count2, cap)
            ix.close()
            out = {"count": np.array([count2], np.int64)}
            if cap >= count:
                out["pairs"] = np.sort(pairs.cpu().numpy())                    # the order comes from an atomic: compared as a sorted set
            return out

        def verify(o):
            exact = OC.gemm_nt_chain(x[lo:hi], x)
            with np.errstate(invalid="ignore"):
                hit = exact >= taus[:, None]
            hit[1] = hit[2] = True
            i, j = np.nonzero(hit)
            assert o["count"][0] >= len(i) > 2 * n
            if "pairs" in o:
                got = o["pairs"]
                assert len(np.unique(got)) == len(got) == o["count"][0]
                assert np.isin(((i + lo).astype(np.int64) << 32) | j.astype(np.int64), got).all()      # every exact hit is a candidate
                gi, gj = got >> 32, got & 0xFFFFFFFF
                assert (gi >= lo).all() and (gi < hi).all() and (gj < n).all()
                assert o["count"][0] < (hi - lo) * n                           # and rows are pruned
        return [(run, verify)]
    return add("join_candidates_rows[%dx%d rows %d..%d capacity=%s]" % (n, d, lo, hi, capacity), Lazy(make), larger)


_jr_big = _rows_case(400, 100, 0, 400, "count")
_jr_big.larger = _rows_case(300, 64, 128, 300, "count", larger=_jr_big)
_rows_case(131, 7, 0, 131, "count", larger=_jr_big)
_rows_case(131, 7, 0, 131, 3, larger=_jr_big)


def _resolve_case(n, d, ld, k, m_lo, larger=None):
    def make():
        wide = _join_rows(n, d, n + d, ld)
        x = np.ascontiguousarray(wide[:, :d])
        x[3] = x[2]                                                            # equal scores: ascending id
        wide[:, :d] = x
        m = n - m_lo
        exact = OC.gemm_nt_chain(x[m_lo:], x)
        keep = exact >= F32(0.3)
        keep[:, :3] = True
        keep[0, 3:] = False                                                    # a row with fewer candidates than k: 3
        keep[1] = True                                                         # and one with all of them
        i, j = np.nonzero(keep)
        perm = np.random.default_rng(n).permutation(len(i))
        pairs = (((i + m_lo).astype(np.int64) << 32) | j.astype(np.int64))[perm]

        def run(env):
            a = env.put("rows_a", wide)[:, :d]
            b = env.put("rows_b", wide)[:, :d]
            ids, sc, counts = env.ops.knn_resolve(a, b, env.put("pairs", pairs), m_lo, m, k)
            return {"ids": ids, "scores": sc, "counts": counts}

        def verify(o):
            masked = np.where(keep, exact, F32(-np.inf))
            order = rank_order(masked)[:, :k]
            have = keep.sum(axis=1)
            want_ids = np.where(np.arange(k)[None, :] < have[:, None], order, -1).astype(np.int64)
            want_sc = np.where(want_ids >= 0, np.take_along_axis(exact, order, axis=1), F32(np.nan)).astype(F32)
            assert (have[2:] >= 3).all() and have[0] == 3 and (k <= 3 or (want_ids[0, 3:] == -1).all())
            bits_equal(o["counts"], have.astype(np.int32))
            bits_equal(o["ids"], want_ids)
            np.testing.assert_array_equal(np.isnan(o["scores"]), np.isnan(want_sc))
            ok = ~np.isnan(want_sc)
            bits_equal(o["scores"][ok], want_sc[ok])
        return [(run, verify)]
    return add("knn_resolve[%dx%d ld=%d k=%d m_lo=%d]" % (n, d, ld, k, m_lo), Lazy(make), larger)


_kr_big = _resolve_case(400, 100, 100, 10, 0)
_kr_big.larger = _resolve_case(131, 7, 9, 5, 0, larger=_kr_big)
_resolve_case(131, 7, 7, 1, 128, larger=_kr_big)
_resolve_case(200, 8, 12, 64, 72, larger=_kr_big)


# entry point -> its cases.  The census of tests/test_memguard_host.py does not see these entry points (their prototypes are in
# include/mdx_knn_join.h); tests/test_knn_join_host.py::test_every_knn_join_entry_point_is_covered reads this table instead.
COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")] for entry in ("knn_bounds", "join_candidates_rows", "knn_resolve")}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_memory_contract(case):
    from mdir_amd import ops
    log = []
    assert case.larger is not None and case.larger is not case
    try:
        memguard.run_contract(ops, case, DEV, alignment_run=True, log=log.append)
        assert "stale" in log and any(step.startswith("align ") for step in log), log
    finally:
        case.release()
        case.larger.release()
        print("%s: %s" % (case.name, "; ".join(log)))


def test_stats_below_16_bytes_and_short_workspaces_are_refused():
    """include/mdx.h "Alignment": stats_a / stats_b of mdx_knn_bounds and mdx_join_candidates_rows at 8 mod 16 are refused, and so
    is a workspace below 16 bytes of alignment -- before anything is launched (no guard touched)."""
    from mdir_amd import ops
    x = _join_rows(200, 64, 1)
    rows = torch.from_numpy(x).to(DEV)
    ix = ops.DescriptorIndex(rows, "ND", storage="i8")
    good = ops.join_stats(ix, rows)
    arena = memguard.Arena(DEV)
    bad = arena.put(good.cpu().numpy(), 8, 0xFF, "stats")
    t = torch.zeros(200, dtype=torch.float32, device=DEV)
    for a, b in ((bad, good), (good, bad)):
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.knn_bounds(ix, a, ix, b, 0, 200, 5)
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.join_candidates_rows(ix, a, ix, b, t, 0, 200, 16)
    arena.check()
    ix.close()
    for case in (CASES[1], CASES[9]):                                          # knn_bounds, knn_resolve: the wrapper's workspace
        names = memguard.workspace_names(ops, case, DEV)
        assert names, case.name
        for name in names:
            assert memguard.refuses(ops, case, DEV, {name: 8}), (case.name, name)
            assert not memguard.refuses(ops, case, DEV, {name: 16}), (case.name, name)
        case.release()
