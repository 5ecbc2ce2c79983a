#!/usr/bin/env python3
"""Generate tests/golden/g20_train.npz by RUNNING THE REFERENCE's pooling, normalisation and losses under torch's autograd, in
float64 and in float32, on the CPU of the build container.  The reference is imported through make_golden.import_reference; none
of its source is copied, only inputs and its results are stored.  Re-run:  python tests/golden/make_golden_train.py  -- the file
comes out bit for bit (fixed seeds, and the archive is written with a fixed time stamp).

Tail cases  (key prefix ``tail_<kind>_b<B>_c<C>_h<H>_w<W>``, kind = gem1 | gem2 | gem3 | gem2.92 | mac | spoc):
    x_b.._w..  the map (shared by the kinds), go_b.._w..  the cotangent of the [B,C] descriptor;
    <prefix>_gx64 / _gx32  d l2n(pool(x)) / dx of the reference in float64 / in float32 (stored as float64 / float32),
    <prefix>_gp64 / _gp32  the gradient of GeM's exponent.
Loss cases  (key prefix ``<loss>_d<D>_s<S>_q<nq>``, loss = contrastive | triplet):
    _x [D,N], _label [N], _margin; _loss64 / _loss32, _gx64 / _gx32.  Tuple 0 of every case with S >= 3 has a positive that EQUALS
    its query and a first negative INSIDE the margin; the other negatives are random unit vectors, BEYOND it.
"""
import io
import os
import zipfile

import numpy as np
import torch

from make_golden import HERE, import_reference, sparse_map

# (at least a few channels each: the L2N of a descriptor with one dominant component has a gradient that is all cancellation, and
# then even the float64 run is no reference to 1e-12; the one-channel maps are tested against the closed forms, without the L2N)
TAIL_SHAPES = [(1, 7, 1, 1), (1, 5, 1, 3), (1, 3, 2, 2), (3, 4, 7, 9), (1, 5, 8, 8), (1, 3, 5, 13), (2, 2, 15, 17), (1, 3, 16, 16)]
TAIL_KINDS = [("gem1", 1.0), ("gem2", 2.0), ("gem3", 3.0), ("gem2.92", 2.92), ("mac", None), ("spoc", None)]
LOSS_SHAPES = {"contrastive": [(1, 2, 1), (7, 2, 2), (64, 3, 2), (257, 3, 1), (64, 7, 5)],
               "triplet": [(1, 3, 1), (7, 3, 2), (64, 3, 2), (257, 3, 1), (64, 7, 5)]}
MARGIN = {"contrastive": 0.7, "triplet": 0.1}


def save_npz(path, arrays):
    """np.savez_compressed with the members' time stamp fixed, so that the file does not depend on when it was written."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as archive:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            archive.writestr(info, buf.getvalue())


def tuple_batch(rng, d, s, nq, inside):
    """Unit columns in the tuple layout; tuple 0 (S >= 3): positive == query, first negative at distance ``inside`` of the query."""
    x = rng.standard_normal((d, s * nq))
    x /= np.linalg.norm(x, axis=0, keepdims=True)
    if s >= 3:
        x[:, 1] = x[:, 0]
        step = rng.standard_normal(d) if d > 1 else np.ones(1)
        x[:, 2] = x[:, 0] + inside * step / np.linalg.norm(step)
    label = np.tile(np.array([-1.0, 1.0] + [0.0] * (s - 2)), nq)
    return x.astype(np.float32), label.astype(np.float32)


def main():
    import_reference()
    import cirtorch.layers.functional as LF
    out = {}
    for b, c, h, w in TAIL_SHAPES:
        tag = "b%d_c%d_h%d_w%d" % (b, c, h, w)
        x = sparse_map(2000 + 7 * h + w + c, (b, c, h, w))
        go = np.random.default_rng(3000 + h * w + c).standard_normal((b, c)).astype(np.float32)
        out["x_" + tag], out["go_" + tag] = x, go
        for kind, p in TAIL_KINDS:
            for dtype, suffix in ((torch.float64, "64"), (torch.float32, "32")):
                xt = torch.tensor(x, dtype=dtype, requires_grad=True)
                pt = torch.tensor([p], dtype=dtype, requires_grad=True) if p is not None else None
                pooled = LF.gem(xt, pt, 1e-6) if p is not None else (LF.mac(xt) if kind == "mac" else LF.spoc(xt))
                LF.l2n(pooled, 1e-6).backward(torch.tensor(go, dtype=dtype).reshape(b, c, 1, 1))
                key = "tail_%s_%s" % (kind, tag)
                out[key + "_gx" + suffix] = xt.grad.numpy()
                if pt is not None:
                    out[key + "_gp" + suffix] = pt.grad.numpy()
    for loss, shapes in LOSS_SHAPES.items():
        fn = LF.contrastive_loss if loss == "contrastive" else LF.triplet_loss
        for d, s, nq in shapes:
            x, label = tuple_batch(np.random.default_rng(4000 + d + 10 * s + nq), d, s, nq, 0.2)
            key = "%s_d%d_s%d_q%d" % (loss, d, s, nq)
            out[key + "_x"], out[key + "_label"], out[key + "_margin"] = x, label, np.float64(MARGIN[loss])
            for dtype, suffix in ((torch.float64, "64"), (torch.float32, "32")):
                xt = torch.tensor(x, dtype=dtype, requires_grad=True)
                value = fn(xt, torch.tensor(label, dtype=dtype), margin=MARGIN[loss])
                value.backward()
                out[key + "_loss" + suffix], out[key + "_gx" + suffix] = value.detach().numpy(), xt.grad.numpy()
    path = os.path.join(HERE, "g20_train.npz")
    save_npz(path, out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
