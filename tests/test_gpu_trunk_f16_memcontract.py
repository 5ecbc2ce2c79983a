"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the three entry points of the
fp16 trunk mode: mdx_bn_act_f16, mdx_pool_l2n_f16, mdx_pool_multi_f16.  Several shapes each, so that the leftovers of the larger
call are the stale pre-fill of the smaller; every caller pointer at the smallest alignment include/mdx.h allows -- 2 bytes for the
fp16 maps, 4 for the fp32 statistics and outputs.  No tolerance is new: the oracles are the two contracts of include/mdx.h, "fp16
trunk", bit for bit -- ``bn_act_exact`` of oracle/chain.py on the upcast input, then numpy's conversion to float16 (to nearest
even); and the fp32 entry point on the upcast maps, itself under the memory contract in test_gpu_memcontract.py."""
import numpy as np
import pytest
import torch

import memguard
from conftest import sparse_map
from oracle import chain as OC
from test_gpu_memcontract import WORKSPACE_ALIGN, Lazy, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16 = np.float32, np.float16

CASES = []


def add(name, made, inplace=(), larger=None):
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), inplace=inplace, larger=larger,
                         workspace_align=WORKSPACE_ALIGN)
    case.release = made.release
    CASES.append(case)
    return case


def _bn_case(shape, use_res, relu, affine, larger=None):
    """H*W a multiple of 8 (the 16-byte path, reached off the grid only in run 5), of 4 only, and odd."""
    def make():
        rng = np.random.default_rng(sum(shape))
        c = shape[1]
        x = (rng.standard_normal(shape) * 2).astype(F16)
        res = rng.standard_normal(shape).astype(F16)
        mean, var = rng.standard_normal(c).astype(F32), rng.uniform(0.2, 3.0, c).astype(F32)
        wt, bs = rng.uniform(0.5, 1.5, c).astype(F32), rng.standard_normal(c).astype(F32)

        def run(env):
            return {"x": env.ops.bn_act_(env.put("x", x), env.put("mean", mean), env.put("var", var), env.put("weight", wt) if affine else None,
                                         env.put("bias", bs) if affine else None, 1e-5, env.put("residual", res) if use_res else None, relu)}

        def verify(o):
            want = OC.bn_act_exact(x.astype(F32), mean, var, wt if affine else None, bs if affine else None, 1e-5,
                                   res.astype(F32) if use_res else None, relu, add_zero=True)
            assert o["x"].dtype == F16
            np.testing.assert_array_equal(o["x"], want.astype(F16))
        return [(run, verify)]
    return add("bn_act_f16[%s res=%s relu=%s affine=%s]" % (shape, use_res, relu, affine), Lazy(make), inplace=("x",), larger=larger)


_bn_big = _bn_case((2, 3, 4, 8), True, True, True)
_bn_big.larger = _bn_case((1, 5, 3, 4), True, False, True, larger=_bn_big)
_bn_case((1, 2, 3, 5), False, True, False, larger=_bn_big)
_bn_case((1, 3, 2, 8), True, True, False, larger=_bn_big)


def _pool_case(shape, kind, p, larger=None):
    """H*W % 4 == 0 (the 8-byte pieces) and odd; the fp32 twin runs under ordinary allocations inside ``run``."""
    def make():
        x = sparse_map(sum(shape), shape).astype(F16)
        x[-1, 0] = 0.0                                                          # an all-zero plane

        def run(env):
            out = env.ops.pool_l2n(env.put("feat", x), kind, p)
            torch.cuda.synchronize()
            return {"out": out}

        def verify(o):
            from mdir_amd import ops
            want = ops.pool_l2n(torch.from_numpy(x.astype(F32)).to(DEV), kind, p)
            bits_equal(o["out"], want.cpu().numpy())
        return [(run, verify)]
    return add("pool_l2n_f16[%s %s]" % (shape, kind), Lazy(make), larger=larger)


_pl_big = _pool_case((2, 5, 4, 6), "gem", 2.92)
_pl_big.larger = _pool_case((1, 7, 3, 5), "gem", 3.0, larger=_pl_big)
_pool_case((2, 5, 4, 6), "mac", 1.0, larger=_pl_big)
_pool_case((1, 7, 3, 5), "spoc", 1.0, larger=_pl_big)


def _multi_case(B, C, sizes, kind, p, larger=None):
    def make():
        maps = [(sparse_map(30 + i, (B, C, h, w)) + F32(0.01)).astype(F16) for i, (h, w) in enumerate(sizes)]

        def run(env):
            return {"out": env.ops.pool_multi([env.put("feat%d" % i, m) for i, m in enumerate(maps)], kind, p)}

        def verify(o):
            from mdir_amd import ops
            want = ops.pool_multi([torch.from_numpy(m.astype(F32)).to(DEV) for m in maps], kind, p)
            bits_equal(o["out"], want.cpu().numpy())
        return [(run, verify)]
    return add("pool_multi_f16[B%d C%d %s %s]" % (B, C, sizes, kind), Lazy(make), larger=larger)


_pm_big = _multi_case(2, 8, [(4, 6), (3, 5), (2, 2)], "gem", 2.92)
_pm_big.larger = _multi_case(3, 7, [(3, 3), (1, 5)], "gem", 2.92, larger=_pm_big)
_multi_case(1, 5, [(2, 4), (3, 3)], "mac", 1.0, larger=_pm_big)

# entry point -> its cases.  The census of tests/test_memguard_host.py does not see these entry points (their prototypes are in
# include/mdx_trunk_f16.h); tests/test_trunk_f16_host.py::test_every_f16_entry_point_is_covered reads this table instead.
COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")] for entry in ("bn_act_f16", "pool_l2n_f16", "pool_multi_f16")}


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
