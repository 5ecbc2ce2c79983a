"""The reference's training criteria on the device: ``ContrastiveLoss`` and ``TripletLoss`` (cirtorch/layers/loss.py) over
``mdx_contrastive_loss`` / ``mdx_triplet_loss`` (include/mdx_train.h), which return the loss and its gradient in one call.

A batch is ``x`` [D,N], one descriptor per column, and ``label`` [N]: tuples of ``S`` columns each, ``(q, p, n1, .., n_{S-2})`` with the
labels ``(-1, 1, 0, .., 0)``.  ``LF.contrastive_loss`` (functional.py:141-157) finds the queries as ``x[:, ::S]`` and pairs them with
the other columns in order; labels in another layout make it pair the wrong columns silently.  Here the layout is checked on the
host first (:func:`tuple_layout`) and anything else is a ``ValueError``.
"""
import torch
import torch.nn as nn

from . import autograd

CRITERIA = {"contrastive", "triplet"}


def _labels(label, device=None):
    """``label`` (a tensor, a list of numbers or a list of per-tuple tensors, as ``target`` of the reference's loader) -> one fp32 vector."""
    if isinstance(label, (list, tuple)):
        label = torch.cat([torch.as_tensor(t, dtype=torch.float32).reshape(-1).cpu() for t in label]) if len(label) else torch.zeros(0)
    if not isinstance(label, torch.Tensor):
        raise TypeError("label must be a tensor or a list of tensors, got %s" % type(label).__name__)
    return label.reshape(-1).to(device=device or label.device, dtype=torch.float32)


def tuple_layout(label, n, kind="contrastive"):
    """``(nq, S)`` of a label vector in the tuple layout for ``n`` columns; ``ValueError`` for any other.  Checked: there is a query
    (label -1); ``n`` is a multiple of their number; the queries are the columns ``0, S, 2S, ..``; every other label is 1 or 0;
    ``S >= 2``; for ``kind="triplet"``: ``S >= 3`` and exactly one positive (label 1) in every tuple."""
    if kind not in CRITERIA:
        raise ValueError("unknown loss %r, one of %s" % (kind, sorted(CRITERIA)))
    lab = _labels(label).cpu()
    if lab.numel() != n:
        raise ValueError("%d labels for %d columns" % (lab.numel(), n))
    queries = (lab == -1).nonzero().reshape(-1).tolist()
    nq = len(queries)
    if nq == 0:
        raise ValueError("no query (label -1) among the labels: tuples are (q, p, n1, ..) with labels (-1, 1, 0, ..)")
    if n % nq:
        raise ValueError("N = %d columns is not divisible by the %d queries (label -1): tuples must have equal length" % (n, nq))
    s = n // nq
    if queries != list(range(0, n, s)):
        raise ValueError("the queries (label -1) must be every S-th column, S = N / nq = %d: columns %s expected, found at %s"
                         % (s, list(range(0, n, s))[:8], queries[:8]))
    if not bool(((lab == -1) | (lab == 0) | (lab == 1)).all()):
        raise ValueError("labels must be -1 (query), 1 (positive) or 0 (negative)")
    if s < (3 if kind == "triplet" else 2):
        raise ValueError("tuples of S = %d columns: the %s loss needs at least %d" % (s, kind, 3 if kind == "triplet" else 2))
    if kind == "triplet":
        positives = (lab.reshape(nq, s) == 1).sum(1)
        if not bool((positives == 1).all()):
            bad = int((positives != 1).nonzero()[0])
            raise ValueError("the triplet loss needs exactly one positive (label 1) per tuple: tuple %d has %d" % (bad, int(positives[bad])))
    return nq, s


def tuple_loss(kind, x, label, margin, eps=1e-6):
    """The loss of ``kind`` on ``x`` [D,N] (a CUDA/ROCm fp32 tensor; it may ask for its gradient) as a 0-d tensor."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("x must be a CUDA/ROCm tensor: the MI355X path has no CPU fallback")
    if x.dim() != 2:
        raise ValueError("x must be [D,N], got %s" % (tuple(x.shape),))
    nq, _ = tuple_layout(label, x.shape[1], kind)
    return autograd.TupleLoss.apply(x, _labels(label, x.device), nq, kind, float(margin), float(eps))


class ContrastiveLoss(nn.Module):
    """loss.py:10-33: ``0.5 l d^2 + 0.5 (1 - l) max(margin - d, 0)^2`` summed over the (query, other) pairs of every tuple."""
    reduction = "sum"

    def __init__(self, margin=0.7, eps=1e-6):
        super().__init__()
        self.margin = margin
        self.eps = eps

    def forward(self, x, label):
        return tuple_loss("contrastive", x, label, self.margin, self.eps)

    def __repr__(self):
        return "%s(margin=%.4f)" % (type(self).__name__, self.margin)


class TripletLoss(nn.Module):
    """loss.py:36-47: ``max(|q - p|^2 - |q - n|^2 + margin, 0)`` summed over the negatives of every tuple."""
    reduction = "sum"

    def __init__(self, margin=0.1):
        super().__init__()
        self.margin = margin

    def forward(self, x, label):
        return tuple_loss("triplet", x, label, self.margin)

    def __repr__(self):
        return "%s(margin=%s)" % (type(self).__name__, self.margin)


def initialize_criterion(params):
    """``{"loss": "contrastive" | "triplet", **arguments}`` -> the module (``loss`` is popped); None for empty params."""
    if not params:
        return None
    loss = params.pop("loss")
    if loss not in CRITERIA:
        raise ValueError("unknown loss %r, one of %s" % (loss, sorted(CRITERIA)))
    return {"contrastive": ContrastiveLoss, "triplet": TripletLoss}[loss](**params)
