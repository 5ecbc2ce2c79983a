"""The descriptor tail and the tuple losses as ``torch.autograd.Function``s over libmdx.so (include/mdx_train.h).

The trunk trains through the plain torch modules (``backbones.TrunkSequential`` leaves its fused epilogues whenever
``torch.is_grad_enabled()``); everything after it -- pooling, L2N, the in-network whitening -- is raw-pointer launches, which cut
the graph.  These functions put it back: every forward makes the calls the ``no_grad`` route makes (the same bits), every
backward is a HIP launch of ``mdx_train.hip`` (the whitening's: three torch products on its [n, D] rows).  ``layers`` and
``ImageRetrievalNet.forward`` come here exactly when a gradient is asked for; there is no CPU or torch-op fallback.
"""
import torch

from . import ops


def wanted(*tensors):
    """True when autograd is recording and one of ``tensors`` (None entries skipped) requires a gradient."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _fp32_map(feat):
    if feat.dtype == torch.float16:
        raise NotImplementedError("fp16 feature maps (precision: f16) have no backward: train with precision: f32")
    return feat.contiguous()


class PoolL2N(torch.autograd.Function):
    """``l2n(pool(feat))`` (``l2n_eps=None``: the pooling alone), ``[B,C,H,W] -> [B,C]``.  ``p`` is the GeM exponent as a tensor of
    one element (None for MAC / SPoC) and receives its gradient.  Saves ``feat`` and the un-normalised pooled rows."""

    @staticmethod
    def forward(ctx, feat, p, kind, pool_eps, l2n_eps):
        feat = _fp32_map(feat)
        pv = float(p.detach().reshape(-1)[0]) if p is not None else 1.0
        # mdx_pool_l2n is these two launches (mdx_pool.hip, pool_l2n): the pooling, then mdx_l2n_rows on its result
        pooled = ops.pool_l2n(feat, kind, pv, pool_eps, l2n_eps=None)
        out = pooled if l2n_eps is None else ops.l2n_rows_(pooled.clone(), eps=l2n_eps)
        ctx.save_for_backward(feat, pooled)
        ctx.args = (kind, pv, pool_eps, l2n_eps, None if p is None else (tuple(p.shape), p.dtype))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        feat, pooled = ctx.saved_tensors
        kind, pv, pool_eps, l2n_eps, p_like = ctx.args
        grad_pooled = grad_out.contiguous()
        if l2n_eps is not None:
            grad_pooled = ops.l2n_rows_bwd(pooled, grad_pooled, l2n_eps)
        grad_feat, grad_p = ops.pool_bwd(feat, pooled, grad_pooled, kind, pv, pool_eps)
        if grad_p is not None and p_like is not None and ctx.needs_input_grad[1]:
            grad_p = grad_p.reshape(p_like[0]).to(p_like[1])
        else:
            grad_p = None
        return (grad_feat if ctx.needs_input_grad[0] else None), grad_p, None, None, None


class L2NRows(torch.autograd.Function):
    """``(x + bias) / (||x + bias|| + eps)`` per row of ``[R,D]`` (``bias`` may be None)."""

    @staticmethod
    def forward(ctx, x, bias, eps):
        x = x.contiguous()
        biased = x if bias is None else x + bias                       # what the kernel normalises: saved for the backward
        ctx.save_for_backward(biased)
        ctx.eps = eps
        return ops.l2n_rows_(x.clone(), bias=None if bias is None else bias.detach(), eps=eps)

    @staticmethod
    def backward(ctx, grad_out):
        biased, = ctx.saved_tensors
        grad_x = ops.l2n_rows_bwd(biased, grad_out.contiguous(), ctx.eps)
        return grad_x, (grad_x.sum(0) if ctx.needs_input_grad[1] else None), None


class WhitenLinear(torch.autograd.Function):
    """The in-network whitening ``l2n(W o + b)`` on ``[n, D_in]`` rows.  Forward: the network's resident weight shard
    (``shard.scores``) and ``mdx_l2n_rows`` with the bias, the calls of the ``no_grad`` route.  Backward: ``mdx_l2n_rows_bwd``, then
    ``grad_in = g W``, ``grad_weight = g^T o`` and ``grad_bias = 1^T g`` in torch."""

    @staticmethod
    def forward(ctx, rows, weight, bias, shard, eps):
        rows = rows.contiguous()
        y = shard.scores(rows, "ND")                                    # [n, D_out]: row i = W rows_i
        biased = y.clone() if bias is None else y + bias
        ctx.save_for_backward(rows, weight, biased)
        ctx.eps = eps
        return ops.l2n_rows_(y, bias=None if bias is None else bias.detach(), eps=eps)

    @staticmethod
    def backward(ctx, grad_out):
        rows, weight, biased = ctx.saved_tensors
        g = ops.l2n_rows_bwd(biased, grad_out.contiguous(), ctx.eps)
        need = ctx.needs_input_grad
        return (g @ weight if need[0] else None), (g.t() @ rows if need[1] else None), (g.sum(0) if need[2] else None), None, None


class TupleLoss(torch.autograd.Function):
    """``LF.contrastive_loss`` / ``LF.triplet_loss`` on ``x`` [D,N]: the kernel returns the loss and its gradient together, the
    backward scales the saved gradient.  ``label``: fp32 on ``x``'s device, its layout checked by the caller."""

    @staticmethod
    def forward(ctx, x, label, nq, kind, margin, eps):
        x = x.contiguous()
        if kind == "contrastive":
            loss, grad_x = ops.contrastive_loss(x, label, nq, margin, eps)
        elif kind == "triplet":
            loss, grad_x = ops.triplet_loss(x, label, nq, margin)
        else:
            raise ValueError("unknown loss %r, one of ['contrastive', 'triplet']" % (kind,))
        ctx.save_for_backward(grad_x)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        grad_x, = ctx.saved_tensors
        return grad_x * grad_out, None, None, None, None, None
