"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of mdx_bn_act_into (include/mdx_unet.h).
The destination is a channel slice of a wider buffer, so the WHOLE buffer is the case's in-place input: it is uploaded poisoned
(NaN with a payload of its own), and after the call every byte outside the slice -- the other channels of each image, which lie
BETWEEN the slices of two images -- must still be that poison, while the slice holds the restatement (tests/unet_restatement.py)
to the bit.  Nothing is read past x: the input-tail runs poison the bytes after it.  Every pointer also at 4-byte alignment, where
the entry point falls back to its scalar form."""
import numpy as np
import pytest

import memguard
import unet_restatement as R
from test_gpu_memcontract import WORKSPACE_ALIGN, Lazy, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32

CASES = []


def poison(shape):
    return np.full(shape, 0x7FC0BEEF, dtype=np.uint32).view(F32)


def _case(shape, ctot, c0, act, stats, larger=None, inplace=False):
    """x [N,C,H,W] into channels [c0, c0 + C) of a [N,ctot,H,W] buffer (``inplace``: onto x itself)."""
    def make():
        n, c, h, w = shape
        rng = np.random.default_rng(sum(shape) + ctot + c0)
        x = (rng.standard_normal(shape) * 2).astype(F32)
        mean, var = rng.standard_normal(c).astype(F32), rng.uniform(0.2, 3.0, c).astype(F32)
        wt, bs = rng.uniform(0.5, 1.5, c).astype(F32), rng.standard_normal(c).astype(F32)
        kw = {"bn": dict(mean=mean, var=var, weight=wt, bias=bs, eps=1e-5), "bias": dict(bias=bs), "none": {}}[stats]

        def run(env):
            dev = {k: (env.put(k, v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
            args = (dev.get("mean"), dev.get("var"), dev.get("weight"), dev.get("bias"), kw.get("eps", 0.0), act, 0.2)
            xd = env.put("x", x)
            if inplace:
                env.ops.bn_act_into(xd, xd, *args)
                return {"x": xd}
            buf = env.put("buf", poison((n, ctot, h, w)))
            env.ops.bn_act_into(xd, buf[:, c0:c0 + c], *args)
            return {"buf": buf}

        def verify(o):
            want = R.bn_act_into(x.reshape(n, c, h * w), act=act, slope=0.2, **kw).reshape(shape)
            if inplace:
                return bits_equal(o["x"], want)
            whole = poison((n, ctot, h, w))
            whole[:, c0:c0 + c] = want
            bits_equal(o["buf"], whole)
        return [(run, verify)]
    name = "bn_act_into[%s into %d@%d act=%d %s%s]" % (shape, ctot, c0, act, stats, " in place" if inplace else "")
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs),
                         inplace=("x",) if inplace else ("buf",), larger=larger, workspace_align=WORKSPACE_ALIGN)
    made = Lazy(make)
    case.release = made.release
    CASES.append(case)
    return case


# H*W % 4 == 0 with aligned slices (the 16-byte path), H*W odd (scalar), a slice start off the 16-byte grid, in place
_big = _case((2, 3, 4, 8), 6, 3, R.ACT_LEAKY, "bn")
_big.larger = _case((2, 2, 3, 5), 5, 1, R.ACT_RELU, "bn", larger=_big)
_case((2, 3, 4, 8), 6, 0, R.ACT_RELU, "bias", larger=_big)
_case((1, 3, 3, 5), 7, 2, R.ACT_LEAKY, "bias", larger=_big)
_case((2, 3, 2, 6), 3, 0, R.ACT_NONE, "none", larger=_big)
_case((2, 3, 4, 4), 3, 0, R.ACT_LEAKY, "bn", larger=_big, inplace=True)

# entry point -> its cases; tests/test_unet_host.py::test_every_unet_entry_point_is_covered reads this table (the census of
# tests/test_memguard_host.py does not see the prototypes of include/mdx_unet.h)
COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")] for entry in ("bn_act_into",)}


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
