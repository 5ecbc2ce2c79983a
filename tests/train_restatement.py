"""The formulas of include/mdx_train.h in float64 numpy, and the op sequences they are the gradients of in torch (a helper module,
imported by test_train_host.py, test_gpu_train.py, test_gpu_train_memcontract.py and tools/train_tail_bench.py).

Two halves.  The numpy half evaluates the CLOSED FORMS the kernels implement (no autograd): it is the oracle where the reference
is not installed, and test_train_host.py holds it against the reference's own float64 autograd results (tests/golden/g20_train.npz)
to 1e-12.  The torch half states the forward passes -- pooling, L2N, whitening, the two losses -- in plain differentiable torch ops
on whatever device and dtype the inputs have: the fp32 error of that sequence against float64 is the yardstick of the bounds
(`e32`), and on the GPU it is the baseline the HIP tail is compared and timed against.
"""
import numpy as np
import torch

F64 = np.float64


# ------------------------------------------------------------------ closed forms, float64 numpy

def pool_fwd64(x, kind, p=3.0, eps=1e-6):
    x = np.asarray(x, F64)
    if kind == "mac":
        return x.max(axis=(2, 3))
    if kind == "spoc":
        return x.mean(axis=(2, 3))
    xc = np.where(x < eps, eps, x)
    return (xc ** p).mean(axis=(2, 3)) ** (1.0 / p)


def pool_bwd64(x, grad_y, kind, p=3.0, eps=1e-6):
    """(grad_x, grad_p, magnitude): grad_p and the sum of the magnitudes of its terms are None for MAC / SPoC."""
    x, g = np.asarray(x, F64), np.asarray(grad_y, F64)
    b, c, h, w = x.shape
    if kind == "spoc":
        return np.broadcast_to(g[:, :, None, None] / (h * w), x.shape).copy(), None, None
    if kind == "mac":
        flat = x.reshape(b, c, h * w)
        first = flat.argmax(axis=2)                                     # numpy: the first maximum in row-major order
        out = np.zeros_like(flat)
        np.put_along_axis(out, first[:, :, None], g[:, :, None], axis=2)
        return out.reshape(x.shape), None, None
    xc = np.where(x < eps, eps, x)
    xp = xc ** p
    m = xp.mean(axis=(2, 3))
    y = m ** (1.0 / p)
    grad_x = (g * y ** (1.0 - p))[:, :, None, None] * xc ** (p - 1.0) / (h * w) * (x >= eps)
    t1 = g * y * (-np.log(m) / p ** 2)
    t2 = g * y * (xp * np.log(xc)).mean(axis=(2, 3)) / (p * m)
    return grad_x, float((t1 + t2).sum()), float((np.abs(t1) + np.abs(t2)).sum())


def l2n_fwd64(x, eps=1e-6):
    x = np.asarray(x, F64)
    return x / (np.sqrt((x * x).sum(axis=1, keepdims=True)) + eps)


def l2n_bwd64(x, grad_out, eps=1e-6):
    """x: the rows before normalisation (bias added)."""
    x, g = np.asarray(x, F64), np.asarray(grad_out, F64)
    n = np.sqrt((x * x).sum(axis=1, keepdims=True))
    den = n + eps
    dot = (g * x).sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(n > 0, dot / (n * den * den), 0.0)
    return g / den - x * c


def tail_bwd64(x, grad_out, kind, p=3.0, pool_eps=1e-6, l2n_eps=1e-6):
    """Backward of l2n(pool(x)): (grad_x, grad_p, magnitude)."""
    return pool_bwd64(x, l2n_bwd64(pool_fwd64(x, kind, p, pool_eps), grad_out, l2n_eps), kind, p, pool_eps)


def _tuples(label, n):
    label = np.asarray(label, F64).reshape(-1)
    nq = int((label == -1).sum())
    assert nq > 0 and n % nq == 0 and label.size == n
    return label, nq, n // nq


def contrastive64(x, label, margin=0.7, eps=1e-6):
    """(loss, grad_x) for x [D,N]."""
    x = np.asarray(x, F64)
    label, nq, s = _tuples(label, x.shape[1])
    loss, grad = 0.0, np.zeros_like(x)
    for t in range(nq):
        q = t * s
        for j in range(q + 1, q + s):
            d = x[:, q] - x[:, j] + eps
            dist = np.sqrt((d * d).sum())
            slack = max(margin - dist, 0.0)
            l = label[j]
            loss += 0.5 * l * dist ** 2 + 0.5 * (1 - l) * slack ** 2
            gr = (l - (1 - l) * slack / dist) * d
            grad[:, q] += gr
            grad[:, j] -= gr
    return loss, grad


def triplet64(x, label, margin=0.1):
    x = np.asarray(x, F64)
    label, nq, s = _tuples(label, x.shape[1])
    loss, grad = 0.0, np.zeros_like(x)
    for t in range(nq):
        q = t * s
        pos = q + 1 + int(np.flatnonzero(label[q + 1:q + s] == 1)[0])
        dp = x[:, q] - x[:, pos]
        for j in range(q + 1, q + s):
            if label[j] != 0:
                continue
            dn = x[:, q] - x[:, j]
            arg = (dp * dp).sum() - (dn * dn).sum() + margin
            if arg >= 0:                                                 # the clamp passes the gradient at equality
                loss += arg
                grad[:, q] += 2 * dp - 2 * dn
                grad[:, pos] -= 2 * dp
                grad[:, j] += 2 * dn
    return loss, grad


# ------------------------------------------------------------------ the same forward passes as differentiable torch ops

def pool_torch(x, kind, p=None, eps=1e-6):
    """[B,C,H,W] -> [B,C]; ``p``: a tensor (it may require grad) or a number."""
    if kind == "mac":
        return torch.nn.functional.max_pool2d(x, (x.shape[-2], x.shape[-1])).flatten(1)
    if kind == "spoc":
        return x.mean(dim=(2, 3))
    return x.clamp(min=eps).pow(p).mean(dim=(2, 3)).pow(1.0 / p)


def l2n_torch(x, eps=1e-6):
    return x / (x.norm(p=2, dim=1, keepdim=True) + eps)


def tail_torch(x, kind, p=None, pool_eps=1e-6, l2n_eps=1e-6, weight=None, bias=None):
    """l2n(pool(x)), then l2n(W o + b) when a whitening is given: [B,C,H,W] -> [B,D]."""
    o = l2n_torch(pool_torch(x, kind, p, pool_eps), l2n_eps)
    if weight is not None:
        o = l2n_torch(torch.nn.functional.linear(o, weight, bias), l2n_eps)
    return o


def contrastive_torch(x, label, margin=0.7, eps=1e-6):
    """x [D,N], label [N] in the tuple layout: the queries repeated against the other columns, as the reference pairs them."""
    nq = int((label == -1).sum())
    s = x.shape[1] // nq
    queries = x[:, ::s].repeat_interleave(s - 1, dim=1)
    others = x[:, label != -1]
    l = label[label != -1].to(x.dtype)
    dist = (queries - others + eps).pow(2).sum(dim=0).sqrt()
    return (0.5 * l * dist.pow(2) + 0.5 * (1 - l) * (margin - dist).clamp(min=0).pow(2)).sum()


def triplet_torch(x, label, margin=0.1):
    nq = int((label == -1).sum())
    s = x.shape[1] // nq
    anchors = x[:, label == -1].repeat_interleave(s - 2, dim=1)
    positives = x[:, label == 1].repeat_interleave(s - 2, dim=1)
    negatives = x[:, label == 0]
    return ((anchors - positives).pow(2).sum(dim=0) - (anchors - negatives).pow(2).sum(dim=0) + margin).clamp(min=0).sum()


# ------------------------------------------------------------------ bounds

def ulp32(magnitude):
    """One fp32 ulp at ``magnitude`` (its spacing), at least the smallest normal."""
    return float(np.spacing(np.float32(max(float(magnitude), float(np.finfo(np.float32).tiny)))))


def e32(ref32, ref64):
    """The fp32 run's own error against the float64 run, with a floor of one ulp of the array's largest magnitude."""
    ref64 = np.asarray(ref64, F64)
    err = float(np.abs(np.asarray(ref32, F64) - ref64).max()) if ref64.size else 0.0
    return max(err, ulp32(np.abs(ref64).max() if ref64.size else 0.0))


def torch_grads(fn, inputs, grad_out=None, dtype=torch.float32):
    """Run ``fn(*inputs)`` on CPU copies of ``inputs`` (numpy arrays) in ``dtype`` with autograd; returns the gradients as float64
    numpy arrays, in order.  ``grad_out``: the cotangent (None for a scalar result)."""
    leaves = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in inputs]
    out = fn(*leaves)
    out.backward(None if grad_out is None else torch.tensor(np.asarray(grad_out), dtype=dtype))
    return [np.zeros(tuple(t.shape), F64) if t.grad is None else t.grad.double().numpy() for t in leaves]
