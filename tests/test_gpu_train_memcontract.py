"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the four launching entry points of
the trainable tail: mdx_pool_bwd, mdx_l2n_rows_bwd, mdx_contrastive_loss, mdx_triplet_loss.  Two shapes each, so that the leftovers
of one call are the stale pre-fill of the other; every caller pointer at the smallest alignment include/mdx_train.h allows, 4 bytes
(the planes of mdx_pool_bwd odd, and H W % 4 == 0 off the 16-byte grid); the workspaces at 16 bytes, and refused below.  The oracle is
the float64 restatement (tests/train_restatement.py) at the bounds of test_gpu_train.py."""
import numpy as np
import pytest

import memguard
import train_restatement as TR
from test_gpu_memcontract import Lazy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
EPS = 1e-6

CASES = []


def add(name, made, larger=None, **kw):
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), larger=larger, **kw)
    case.release = made.release
    CASES.append(case)
    return case


def close(got, want, bound):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) <= bound


def _pool(shape, kind, p):
    def make():
        rng = np.random.default_rng(sum(shape))
        x = (rng.random(shape, dtype=F32) * (rng.random(shape, dtype=F32) > 0.5)).astype(F32)
        gy = rng.standard_normal(shape[:2]).astype(F32)
        want_x, want_p, mag = TR.pool_bwd64(x, gy, kind, p, EPS)
        if kind == "gem" and p not in (1.0, 2.0, 3.0):
            bound = 1e-5 * float(np.abs(want_x).max())
        else:
            bound = 4 * TR.e32(TR.torch_grads(lambda a: TR.pool_torch(a, kind, p, EPS), [x], gy)[0], want_x)

        def run(env):
            feat = env.put("feat", x)
            pooled = env.ops.pool_l2n(feat, kind, p, EPS, l2n_eps=None)        # the forward's own result, as autograd saves it
            gx, gp = env.ops.pool_bwd(feat, pooled, env.put("grad_pooled", gy), kind, p, EPS)
            return {"grad_feat": gx} if gp is None else {"grad_feat": gx, "grad_p": gp}

        def verify(o):
            assert o["grad_feat"].dtype == F32 and close(o["grad_feat"], want_x, bound)
            if kind == "gem":
                assert close(o["grad_p"][0], want_p, 1e-5 * mag)
        return [(run, verify)]
    return make


def _l2n(r, d):
    def make():
        rng = np.random.default_rng(r + d)
        x, go = rng.standard_normal((r, d)).astype(F32), rng.standard_normal((r, d)).astype(F32)
        x[r - 1] = 0
        want = TR.l2n_bwd64(x, go, EPS)
        bound = 4 * TR.e32(TR.torch_grads(lambda a: TR.l2n_torch(a, EPS), [x], go)[0], want)

        def run(env):
            return {"grad_x": env.ops.l2n_rows_bwd(env.put("x", x), env.put("grad_out", go), EPS)}
        return [(run, lambda o: close(o["grad_x"], want, bound) or pytest.fail("grad_x"))]
    return make


def _loss(kind, d, s, nq):
    def make():
        rng = np.random.default_rng(d + s + nq)
        x = rng.standard_normal((d, s * nq))
        x = (x / np.linalg.norm(x, axis=0, keepdims=True) * rng.uniform(0.3, 0.8, s * nq)).astype(F32)
        label = np.tile(np.array([-1.0, 1.0] + [0.0] * (s - 2), F32), nq)
        margin = 0.7 if kind == "contrastive" else 0.1
        fn64, fn_t = (TR.contrastive64, TR.contrastive_torch) if kind == "contrastive" else (TR.triplet64, TR.triplet_torch)
        loss64, gx64 = fn64(x, label, margin)
        import torch
        leaf = torch.tensor(x, requires_grad=True)
        value = fn_t(leaf, torch.from_numpy(label), margin)
        value.backward()
        bounds = 4 * TR.e32(float(value.detach()), loss64), 4 * TR.e32(leaf.grad.numpy(), gx64)

        def run(env):
            loss, gx = getattr(env.ops, kind + "_loss")(env.put("x", x), env.put("label", label), nq, margin)
            return {"loss": loss, "grad_x": gx}

        def verify(o):
            assert close(o["loss"][0], loss64, bounds[0]) and close(o["grad_x"], gx64, bounds[1])
        return [(run, verify)]
    return make


# entry point -> (builder, big arguments, small arguments, Case keywords)
STAGES = {
    "pool_bwd": (_pool, ((3, 5, 7, 9), "gem", 2.92), ((2, 3, 4, 5), "gem", 3.0), {"workspace_align": 16}),
    "l2n_rows_bwd": (_l2n, (3, 257), (1, 7), {}),
    "contrastive_loss": (_loss, ("contrastive", 257, 3, 2), ("contrastive", 7, 2, 1), {"workspace_align": 16}),
    "triplet_loss": (_loss, ("triplet", 257, 4, 2), ("triplet", 7, 3, 1), {"workspace_align": 16}),
}

for _entry, (_builder, _big_args, _small_args, _kw) in STAGES.items():
    _big = add("%s[big]" % _entry, Lazy(_builder(*_big_args)), **_kw)
    _big.larger = add("%s[small]" % _entry, Lazy(_builder(*_small_args)), larger=_big, **_kw)
# the poolings without a workspace: MAC on odd planes, SPoC on H W % 4 == 0
_mac = add("pool_bwd[mac]", Lazy(_pool((2, 5, 5, 13), "mac", 1.0)))
_mac.larger = add("pool_bwd[spoc]", Lazy(_pool((1, 3, 2, 6), "spoc", 1.0)), larger=_mac)

# entry point -> its cases.  The census of tests/test_memguard_host.py does not see these entry points (their prototypes are in
# include/mdx_train.h); tests/test_train_host.py::test_every_launching_entry_point_has_memory_contract_cases reads this table instead.
COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")] for entry in STAGES}


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


@pytest.mark.parametrize("name", ["pool_bwd[small]", "contrastive_loss[small]", "triplet_loss[small]"])
def test_workspace_below_16_bytes_is_refused(name):
    from mdir_amd import ops
    case = next(c for c in CASES if c.name == name)
    try:
        assert memguard.workspace_names(ops, case, DEV) == ["ws0"]
        for align in (8, 4):
            assert memguard.refuses(ops, case, DEV, {"ws0": align}), align
        assert not memguard.refuses(ops, case, DEV, {"ws0": 16})
    finally:
        case.release()
