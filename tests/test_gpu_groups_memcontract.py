"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the four entry points of the
near-duplicate groups: mdx_groups_init, mdx_groups_union_pairs, mdx_groups_union_dense, mdx_groups_labels.  Two shapes each, so
that the leftovers of one call are the stale pre-fill of the other; every caller pointer at the smallest alignment include/mdx.h
allows, its element size (the rows of union_pairs at 4 bytes: the kernel then takes its scalar loads).  parent, status and labels
are written within their bounds only.  No tolerance: the oracle is the sequential union-find of test_gpu_groups.py over the exact
chain of oracle/chain.py."""
import numpy as np
import pytest
import torch

import memguard
from oracle import chain as OC
from test_gpu_groups import components
from test_gpu_memcontract import Lazy, _join_rows, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32

CASES = []


def add(name, made, larger=None):
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), larger=larger)
    case.release = made.release
    CASES.append(case)
    return case


def _hits(chain, keep, tau):
    with np.errstate(invalid="ignore"):
        return np.nonzero(keep & (chain >= F32(tau)))


def _init_case(T, n, larger=None):
    def make():
        def run(env):
            parent, status = env.ops.groups_init(T, n, DEV)
            return {"parent": parent, "status": status}

        def verify(o):
            bits_equal(o["parent"], np.tile(np.arange(n, dtype=np.int32), (T, 1)))
            bits_equal(o["status"], np.zeros(4, np.int64))
        return [(run, verify)]
    return add("groups_init[%dx%d]" % (T, n), Lazy(make), larger)


_gi_big = _init_case(3, 1000)
_gi_big.larger = _init_case(1, 7, larger=_gi_big)
_init_case(8, 257, larger=_gi_big)


def _forest_outputs(ops, parent, status):
    labels = ops.groups_labels(parent)
    return {"labels": labels, "hooks_flags": status.cpu().numpy()[2:].copy()}      # chains and edges depend on the schedule


def _verify_forest(o, n, want):
    bits_equal(o["labels"], want)
    bits_equal(o["hooks_flags"], np.array([sum(n - len(np.unique(w)) for w in want), 0], np.int64))


def _pairs_case(n, d, ld, taus, larger=None):
    def make():
        wide = _join_rows(n, d, n + d, ld)
        x = np.ascontiguousarray(wide[:, :d])
        chain = OC.gemm_nt_chain(x, x)
        upper = np.arange(n)[None, :] > np.arange(n)[:, None]
        i, j = _hits(chain, upper, min(taus) - 0.3)                            # a superset of every level's edges ...
        i, j = np.concatenate([i, i[:50], [3, n - 1]]), np.concatenate([j, j[:50], [3, n - 1]])     # ... duplicates, and i == j
        perm = np.random.default_rng(n).permutation(len(i))
        pairs = ((i.astype(np.int64) << 32) | j.astype(np.int64))[perm]

        def run(env):
            ops = env.ops
            rows = env.put("rows", wide)[:, :d]
            parent, status = ops.groups_init(len(taus), n, DEV)
            ops.groups_union_pairs(rows, env.put("pairs", pairs), list(taus), parent, status)
            return _forest_outputs(ops, parent, status)

        def verify(o):
            want = np.stack([components(n, *_hits(chain, upper, t)) for t in taus])
            assert len(np.unique(want[-1])) < n
            _verify_forest(o, n, want)
        return [(run, verify)]
    return add("groups_union_pairs[%dx%d ld=%d T=%d]" % (n, d, ld, len(taus)), Lazy(make), larger)


_up_big = _pairs_case(300, 200, 200, (0.95, 0.8, 0.5))                         # two stages of 128 k, 16-byte loads
_up_big.larger = _pairs_case(131, 7, 9, (0.9,), larger=_up_big)                # ld % 4 != 0: scalar loads, one short stage
_pairs_case(200, 64, 68, (0.7, 0.9), larger=_up_big)


def _dense_case(n, m, ncols, ld, row_base, col_base, taus, larger=None):
    def make():
        x = _join_rows(n, 32, n + m)
        chain = OC.gemm_nt_chain(x, x)
        wide = np.random.default_rng(n + ld).standard_normal((m, ld)).astype(F32) + F32(2)     # beyond ncols: all above the thresholds
        wide[:, :ncols] = chain[row_base:row_base + m, col_base:col_base + ncols]
        keep = np.zeros((n, n), bool)
        keep[row_base:row_base + m, col_base:col_base + ncols] = True
        keep &= np.arange(n)[None, :] > np.arange(n)[:, None]

        def run(env):
            ops = env.ops
            scores = env.put("scores", wide)[:, :ncols]
            parent, status = ops.groups_init(len(taus), n, DEV)
            ops.groups_union_dense(scores, row_base, col_base, list(taus), parent, status)
            return _forest_outputs(ops, parent, status)

        def verify(o):
            want = np.stack([components(n, *_hits(chain, keep, t)) for t in taus])
            assert len(np.unique(want[-1])) < n
            _verify_forest(o, n, want)
        return [(run, verify)]
    return add("groups_union_dense[n=%d %dx%d ld=%d at (%d, %d) T=%d]" % (n, m, ncols, ld, row_base, col_base, len(taus)), Lazy(make), larger)


_ud_big = _dense_case(300, 170, 300, 304, 20, 0, (0.95, 0.3))                  # the fp32-index form: every column, rows from row_base
_ud_big.larger = _dense_case(131, 67, 67, 67, 64, 64, (0.2,), larger=_ud_big)  # the rowmajor form: the block's own corner
_dense_case(300, 1, 257, 257, 0, 43, (0.5, 0.2), larger=_ud_big)


def _labels_case(T, n, larger=None):
    def make():
        rng = np.random.default_rng(T * n)
        parent = np.stack([np.minimum(np.arange(n), rng.integers(0, n, n) // (1 + t)) for t in range(T)]).astype(np.int32)     # parent[x] <= x
        parent[:, n // 2] = n // 2                                             # one more root

        def run(env):
            return {"labels": env.ops.groups_labels(env.put("parent", parent))}

        def verify(o):
            want = np.empty((T, n), np.int64)
            for t in range(T):
                for i in range(n):
                    r = i
                    while parent[t, r] != r:
                        r = parent[t, r]
                    want[t, i] = r
            assert (want <= np.arange(n)).all() and len(np.unique(want[0])) > 1
            bits_equal(o["labels"], want)
        return [(run, verify)]
    return add("groups_labels[%dx%d]" % (T, n), Lazy(make), larger)


_gl_big = _labels_case(3, 1000)
_gl_big.larger = _labels_case(1, 7, larger=_gl_big)
_labels_case(8, 257, larger=_gl_big)


# entry point -> its cases.  The census of tests/test_memguard_host.py does not see these entry points (their prototypes are in
# include/mdx_groups.h); tests/test_groups_host.py::test_every_groups_entry_point_is_covered reads this table instead.
COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")]
           for entry in ("groups_init", "groups_union_pairs", "groups_union_dense", "groups_labels")}


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
