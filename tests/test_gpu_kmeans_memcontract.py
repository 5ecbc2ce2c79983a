"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the three launching entry points of
spherical k-means: mdx_kmeans_argmax, mdx_kmeans_sums, mdx_kmeans_finish.  Several shapes each, so that the leftovers of one call are
the stale pre-fill of the other; every caller pointer at the smallest alignment include/mdx_kmeans.h allows -- 4 bytes for the fp32
matrices (off the 16-byte grid: the dword paths; on it: the 16-byte paths; the same bits), 8 for the int64 vectors; the workspace at 16
bytes, refused below, at exactly the size the size function says, and refused one byte short.  The optional outputs of the argmax are
left out one at a time.  The oracles are those of test_gpu_kmeans.py: the restatement (tests/kmeans_restatement.py), bit for bit for
the argmax and the sums, at the finish tolerance for the finish."""
import ctypes

import numpy as np
import pytest
import torch

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


def _argmax(m, k, ld, labels=True, best=True):
    """``ld > k``: the block is the first k columns of a wider matrix.  Ties, -0 / +0, -inf and NaN among the scores."""
    def make():
        rng = np.random.default_rng(m + k)
        wide = rng.integers(-4, 5, size=(m, ld)).astype(F32)
        wide[rng.random((m, ld)) < 0.05] = F32(np.nan)
        wide[rng.random((m, ld)) < 0.05] = F32(-np.inf)
        wide[(wide == 0) & (rng.random((m, ld)) < 0.5)] = F32(-0.0)
        wide[m - 1] = F32(np.nan)
        want_l, want_b = KR.argmax_first(wide[:, :k])

        def run(env):
            got_l, got_b = env.ops.kmeans_argmax(env.put("scores", wide)[:, :k], out_labels=None if labels else False,
                                                 out_best=None if best else False)
            assert (got_l is None) == (not labels) and (got_b is None) == (not best)
            return {name: t for name, t in (("labels", got_l), ("best", got_b)) if t is not None}

        def verify(o):
            if labels:
                bits_equal(o["labels"], want_l)
            if best:
                bits_equal(o["best"], want_b)
        return [(run, verify)]
    return make


def _sums(n, d, k, ld, sizes):
    """Clusters of the given sizes over a shuffled subset of the rows (the rest is left out), an id of -1 and an id of n among the
    members of the first non-empty cluster."""
    def make():
        rng = np.random.default_rng(n + d)
        wide = rng.standard_normal((n, ld)).astype(F32)
        assert len(sizes) == k and sum(sizes) + 2 <= n
        chosen = rng.permutation(n)[:sum(sizes)]
        parts, at, spoiled = [], 0, False
        for s in sizes:
            ids = np.sort(chosen[at:at + s])
            at += s
            if s and not spoiled:
                ids, spoiled = np.concatenate([[-1], ids, [n]]), True
            parts.append(ids.astype(np.int64))
        members = np.concatenate(parts)
        offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        assert (members == -1).sum() == 1 and (members == n).sum() == 1 and len(members) <= n
        want = KR.sums32(wide[:, :d], members, offsets, k)

        def run(env):
            return {"sums": env.ops.kmeans_sums(env.put("rows", wide)[:, :d], env.put("members", members), env.put("offsets", offsets), k)}
        return [(run, lambda o: bits_equal(o["sums"], want))]
    return make


def _finish(k, d, previous):
    def make():
        rng = np.random.default_rng(k + d)
        sums = (rng.standard_normal((k, d)) * 7).astype(F32)
        sums[k - 1] = 0
        sums[k - 1, ::2] = F32(-0.0)
        prev = rng.standard_normal((k, d)).astype(F32)
        want = KR.finish64(sums, 1e-6, prev if previous else None)

        def run(env):
            return {"centroids": env.ops.kmeans_finish(env.put("sums", sums), 1e-6, env.put("previous", prev) if previous else None)}

        def verify(o):
            got = o["centroids"].astype(np.float64)
            assert o["centroids"].dtype == F32 and (np.abs(got - want) <= KR.finish_tolerance(want, d)).all()
            bits_equal(o["centroids"][k - 1], prev[k - 1] if previous else np.zeros(d, F32))
        return [(run, verify)]
    return make


S = KR.SEGMENT
# entry point -> (builder, big arguments, small arguments, Case keywords)
STAGES = {
    "kmeans_argmax": (_argmax, (65, 1025, 1028), (3, 63, 64), {}),
    "kmeans_sums": (_sums, (3 * S + 40, 36, 5, 40, (0, 1, S + 1, S, S - 1)), (40, 5, 3, 5, (7, 0, 20)), {"workspace_align": 16}),
    "kmeans_finish": (_finish, (5, 257, True), (2, 3, False), {}),
}

for _entry, (_builder, _big_args, _small_args, _kw) in STAGES.items():
    _big = add("%s[big]" % _entry, Lazy(_builder(*_big_args)), **_kw)
    _big.larger = add("%s[small]" % _entry, Lazy(_builder(*_small_args)), larger=_big, **_kw)
# the optional outputs of the argmax, one at a time (the other pointer is NULL); one wave per row and one workgroup per row
_argmax_big = next(c for c in CASES if c.name == "kmeans_argmax[big]")
add("kmeans_argmax[labels only]", Lazy(_argmax(5, 1030, 1030, best=False)), larger=_argmax_big)
add("kmeans_argmax[best only]", Lazy(_argmax(6, 65, 65, labels=False)), larger=_argmax_big)

# entry point -> its cases.  The census of tests/test_memguard_host.py does not see these entry points (their prototypes are in
# include/mdx_kmeans.h); tests/test_kmeans_host.py::test_every_launching_entry_point_has_memory_contract_cases reads this table instead.
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


def test_workspace_below_16_bytes_is_refused():
    from mdir_amd import ops
    case = next(c for c in CASES if c.name == "kmeans_sums[small]")
    try:
        assert memguard.workspace_names(ops, case, DEV) == ["ws0"]
        for align in (8, 4):
            assert memguard.refuses(ops, case, DEV, {"ws0": align}), align
        assert not memguard.refuses(ops, case, DEV, {"ws0": 16})
    finally:
        case.release()


def test_workspace_exact_size_and_one_byte_less():
    """The wrapper hands the library exactly mdx_kmeans_sums_workspace bytes (the guarded runs above); one byte less is
    MDX_ERR_WORKSPACE and nothing is written."""
    from mdir_amd import _lib
    h = _lib.lib()
    n, d, k = 300, 5, 3
    rng = np.random.default_rng(0)
    rows = torch.from_numpy(rng.standard_normal((n, d)).astype(F32)).to(DEV)
    labels = rng.integers(0, k, n)
    members, offsets = (torch.from_numpy(a).to(DEV) for a in KR.csr(labels, k))
    need = h.mdx_kmeans_sums_workspace(n, k, d)
    assert need == 256 + (4 * (2 + k) * 8 + 255) // 256 * 256
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    sums = torch.full((k, d), 7.0, device=DEV)

    def call(nbytes):
        return h.mdx_kmeans_sums(ctypes.c_void_p(rows.data_ptr()), n, d, d, ctypes.c_void_p(members.data_ptr()), ctypes.c_void_p(offsets.data_ptr()), k,
                                 ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(ws.data_ptr()), nbytes, None)
    assert call(need - 1) == -4 and h.mdx_last_error().startswith(b"mdx_kmeans_sums: workspace")
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all())
    assert call(need) == 0
    torch.cuda.synchronize()
    bits_equal(sums.cpu().numpy(), KR.sums32(rows.cpu().numpy(), members.cpu().numpy(), offsets.cpu().numpy(), k))
