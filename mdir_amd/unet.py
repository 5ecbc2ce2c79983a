"""The illumination-normalising generators that stand in front of the embedding network in a ``SequentialNetwork``
(``network.py``): the U-Net labels of the reference registry, ``mdir/components/model/network/__init__.py``.

One builder serves all of them.  A label is a row of ``LABELS``: its constructor defaults, the option sets of its convolutions, a
``head`` and a ``tail`` around the outermost skip level, and the name of a level layout in ``LEVELS``.  A layout lists the named
children of a level, each a row of layer tokens; ``_stack`` turns a row into modules.  Child names and indices are the
reference's, so its ``state_dict`` loads unchanged (``outerblock.2.nested.0.weight``, ``outerblock.downconv.conv1.weight``).

Two routes compute the same function:

* the module route: every child called in order, ``torch.cat`` at the end of a level -- CPU, autograd, training, and
  ``MDIR_AMD_FUSED_UNET=0``;
* the fused route (inference on the GPU, fp32, BatchNorm in eval): every run ``Conv2d | ConvTranspose2d -> [BatchNorm2d] ->
  [Dropout] -> ReLU | LeakyReLU`` is the library convolution followed by ONE ``mdx_bn_act_into`` (include/mdx_unet.h).  Without a
  BatchNorm the conv bias is the epilogue's shift; with one it stays in the convolution.  A skip level owns one ``[N, 2C, H, W]``
  buffer: the producer of the level's input writes its epilogue into channels ``[0, C)``, the level's last epilogue into
  ``[C, 2C)``, and no ``torch.cat`` runs.  No synchronisation and no host read: the route captures into a ``graphs.ShapeGraphs``.

Tanh, MaxPool, ``F.interpolate`` and every convolution are torch's in both routes.
"""
import os
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F


class Identity(nn.Module):
    """``identity`` of the registry: returns its input."""

    def __init__(self):
        super().__init__()
        self.meta = {}

    def forward(self, x):
        return x


# ---------------------------------------------------------------------------------------------------------------- the tables
#
# A layer token is (op, *args).  Channel arguments are integers or names looked up in the level's environment:
#   outer / inter   the widths of a pix2pix level: its input and the map one resolution below
#   cat             what comes back from below: 2 * inter with a nested level, inter at the innermost
#   cin / ch / ch2  the classic level: input, width, 2 * width
# The last argument of a convolution names one of the label's option sets.  `bn` and `drop` vanish where the label has no
# batch-norm / dropout, `nested` where there is no deeper level.

def _conv_block(cin, cout):
    return ("block", [("conv", cin, cout, "k3"), ("relu",), ("conv", cout, cout, "k3"), ("relu",)], ["conv1", "relu1", "conv2", "relu2"])


LEVELS = {
    # pix2pix: y = nested(x); the level answers x || y
    "p2p": {"route": "cat_input",
            "children": [("nested", [("conv", "outer", "inter", "conv"), ("bn", "inter"), ("leaky",), ("nested",),
                                     ("convT", "cat", "outer", "conv"), ("bn", "outer"), ("drop",), ("relu",)])],
            "innermost": [("nested", [("conv", "outer", "inter", "conv"), ("relu",),
                                      ("convT", "cat", "outer", "conv"), ("bn", "outer"), ("drop",), ("relu",)])]},
    # a 1x1 convolution after each resampling one
    "shallow": {"route": "cat_input",
                "children": [("nested", [("conv", "outer", "inter", "conv"), ("relu",), ("conv", "inter", "inter", "k1"), ("relu",),
                                         ("nested",),
                                         ("convT", "cat", "outer", "conv"), ("relu",), ("conv", "outer", "outer", "k1"), ("relu",)])]},
    # up by interpolation to the size of the level's input, then a stride-1 convolution: any image size
    "dynint": {"route": "cat_input",
               "children": [("down", [("conv", "outer", "inter", "conv"), ("bn", "inter"), ("leaky",), ("nested",)]),
                            ("up", [("conv", "cat", "outer", "upconv"), ("bn", "outer"), ("drop",), ("relu",)])]},
    # the classic U-Net: two 3x3 convolutions, max-pool down, transposed convolution up; x1 || up joins INSIDE the level
    "orig": {"route": "cat_mid",
             "children": [("downconv", _conv_block("cin", "ch")), ("pool", ("pool",)), ("nested", ("nested",)),
                          ("convT", ("convT", "ch2", "ch", "t2")), ("upconv", _conv_block("ch2", "ch"))]},
}

_DOWN = {"kernel_size": 4, "stride": 2, "padding": 1}
_SAME3 = {"kernel_size": 3, "stride": 1, "padding": 1}

# defaults: the constructor's parameters after (in_channels, out_channels), in the reference's order
LABELS = {
    "p2p_unet": {
        "defaults": (("dropout", 0), ("conv_opts", None), ("batchnorm_opts", None), ("batchnorm", True), ("nested_levels", 7)),
        "conv": {**_DOWN, "bias": False}, "level": "p2p", "dropout_from": 4,
        "children": [("outerblock", [("conv", "in", 64, "conv"), ("leaky",), ("level",),
                                     ("convT", 128, "out", "conv_bias"), ("tanh",)])]},
    "outconv_unet": {
        "defaults": (("conv_opts", None), ("batchnorm_opts", None), ("nested_levels", 7), ("outconv_channels", 32),
                     ("outconv_kernel", 3), ("dropout", False), ("batchnorm", False)),
        "conv": _DOWN, "level": "p2p",
        "children": [("outerblock", [("conv", "in", 64, "conv"), ("leaky",), ("level",),
                                     ("convT", 128, "outconv", "conv"), ("relu",), ("conv", "outconv", "out", "outk")])]},
    "outconv_dynint_unet": {
        "defaults": (("conv_opts", None), ("upconv_opts", None), ("nested_levels", 7), ("upsample", "bilinear"),
                     ("outconv_channels", 32), ("outconv_kernel", 3), ("dropout", False), ("batchnorm", False)),
        "conv": _DOWN, "upconv": _SAME3, "level": "dynint",
        "children": [("down", [("conv", "in", 64, "conv"), ("leaky",), ("level",)]),
                     ("up", [("conv", 128, "outconv", "upconv"), ("relu",), ("conv", "outconv", "out", "outk")])]},
    "shallow_p2p_unet": {
        "defaults": (("conv_opts", None), ("nested_levels", 4)),
        "conv": _DOWN, "level": "shallow",
        "children": [("outerblock", [("conv", "in", 64, "conv"), ("relu",), ("conv", 64, 64, "k1"), ("relu",), ("level",),
                                     ("convT", 128, 64, "conv"), ("relu",), ("conv", 64, 64, "k1"), ("relu",),
                                     ("conv", 64, "out", "k1")])]},
    "inconv_p2p_unet": {
        "defaults": (("conv_opts", None), ("nested_levels", 7)),
        "conv": _DOWN, "level": "p2p",
        "children": [("outerblock", [("conv", "in", 64, "k1"), ("leaky",), ("conv", 64, 64, "conv"), ("leaky",), ("level",),
                                     ("convT", 128, "out", "conv"), ("tanh",)])]},
    "aligned_p2p_unet": {
        "defaults": (("conv_opts", None), ("nested_levels", 7)),
        "conv": _DOWN, "level": "p2p",
        "children": [("outerblock", [("conv", "in", 64, "k3"), ("relu",), ("conv", 64, 64, "k3"), ("relu",), ("level",),
                                     ("conv", 128, 64, "k3"), ("relu",), ("conv", 64, 64, "k3"), ("relu",),
                                     ("conv", 64, "out", "k3")])]},
    "orig_unet": {
        "defaults": (("nested_levels", 4), ("min_channels", 64)),
        "level": "orig",
        # the reference writes this 1x1 convolution's input width as the literal 64, its default min_channels, and cannot run
        # with another; here it is min_channels, which is the same module wherever the reference runs
        "children": [("outerblock", ("level",)), ("outconv", ("conv", "min", "out", "k1"))]},
}


# --------------------------------------------------------------------------------------------------------------- the builder

def _layer(tok, env):
    """One token -> one module, or None where the label leaves it out."""
    op = tok[0]

    def width(k):
        return env[k] if isinstance(k, str) else k
    if op == "conv":
        return nn.Conv2d(width(tok[1]), width(tok[2]), **env["opts"][tok[3]])
    if op == "convT":
        return nn.ConvTranspose2d(width(tok[1]), width(tok[2]), **env["opts"][tok[3]])
    if op == "bn":
        return nn.BatchNorm2d(width(tok[1]), **env["opts"]["bn"]) if env["batchnorm"] else None
    if op == "drop":
        return nn.Dropout(p=env["dropout"]) if env["dropout"] else None
    if op in ("nested", "level"):
        return env["nested"]
    if op == "block":
        return _stack(tok[1], env, tok[2])
    return {"relu": nn.ReLU, "leaky": lambda: nn.LeakyReLU(0.2), "tanh": nn.Tanh, "pool": lambda: nn.MaxPool2d(2)}[op]()


def _stack(spec, env, names=None):
    """A row of tokens -> ``nn.Sequential`` (indexed, or named by ``names``); a single token -> its module."""
    if isinstance(spec, tuple):
        return _layer(spec, env)
    mods = [m for m in (_layer(tok, env) for tok in spec) if m is not None]
    return nn.Sequential(OrderedDict(zip(names, mods))) if names else nn.Sequential(*mods)


def _level_envs(row, p):
    """The environments of the levels, outermost first, and the innermost module of the classic layout (else None)."""
    depth = p["nested_levels"]
    if row["level"] == "orig":
        mc = p["min_channels"]
        envs = [{"cin": p["in"] if i == 0 else mc * 2 ** i // 2, "ch": mc * 2 ** i, "ch2": mc * 2 ** (i + 1)} for i in range(depth)]
        return envs, _conv_block(mc * 2 ** (depth - 1), mc * 2 ** depth)
    envs = []
    for i in range(depth):
        outer, inter = min(64 << i, 512), min(128 << i, 512)
        dropout = p.get("dropout", False)
        if "dropout_from" in row:             # pix2pix: only the 512-wide levels below the fourth
            dropout = dropout * (i >= row["dropout_from"])
        envs.append({"outer": outer, "inter": inter, "cat": inter * (2 if i + 1 < depth else 1), "dropout": dropout})
    return envs, None


def build_unet(label, in_channels, out_channels, **params):
    row = LABELS[label]
    p = dict(row["defaults"])
    unknown = params.keys() - p.keys()
    if unknown:
        raise TypeError("%s got unexpected parameters %s" % (label, sorted(unknown)))
    p.update(params)
    p.update({"in": in_channels, "out": out_channels})
    assert p["nested_levels"] >= 1, p["nested_levels"]
    kernel = p.get("outconv_kernel", 3)
    assert kernel % 2 == 1, kernel
    conv = {**row.get("conv", {}), **(p.get("conv_opts") or {})}
    opts = {"conv": conv, "conv_bias": {**conv, "bias": True}, "upconv": {**row.get("upconv", {}), **(p.get("upconv_opts") or {})},
            "k1": {"kernel_size": 1}, "k3": {"kernel_size": 3, "padding": 1}, "t2": {"kernel_size": 2, "stride": 2},
            "outk": {"kernel_size": kernel, "padding": kernel // 2}, "bn": p.get("batchnorm_opts") or {}}
    base = {"opts": opts, "batchnorm": p.get("batchnorm", False), "dropout": False, "in": in_channels, "out": out_channels,
            "outconv": p.get("outconv_channels"), "min": p.get("min_channels")}
    layout = LEVELS[row["level"]]
    envs, innermost = _level_envs(row, p)
    nested = _stack(innermost, {**base, "nested": None}) if innermost is not None else None
    for env in reversed(envs):
        children = layout["children"] if nested is not None or "innermost" not in layout else layout["innermost"]
        env = {**base, **env, "nested": nested}
        nested = SkipLevel(layout["route"], [(name, _stack(spec, env)) for name, spec in children], p.get("upsample"))
    top = {**base, "nested": nested}
    return UNet({"in_channels": in_channels, "out_channels": out_channels},
                [(name, _stack(spec, top)) for name, spec in row["children"]], p.get("upsample"))


# ------------------------------------------------------------------------------------------------------------ the two routes

def _fused_unet():
    return os.environ.get("MDIR_AMD_FUSED_UNET", "1") != "0"


def _inference(module):
    return not any(m.training for m in module.modules()) and all(m.track_running_stats and m.running_mean is not None
                                       for m in module.modules() if isinstance(m, nn.BatchNorm2d))


def _chain(children, x, upsample):
    """The named children in order; a child called ``up`` of an interpolating label first brings its input to x's size."""
    size = x.shape[-2:]
    for name, mod in children:
        if upsample and name == "up":
            x = F.interpolate(x, size=size, mode=upsample)
        x = mod(x)
    return x


def _items(mod):
    return list(mod) if isinstance(mod, nn.Sequential) else [mod]


def _convolve(m, x, with_bias):
    bias = m.bias if with_bias else None
    if isinstance(m, nn.ConvTranspose2d):
        return F.conv_transpose2d(x, m.weight, bias, m.stride, m.padding, m.output_padding, m.groups, m.dilation)
    return F.conv2d(x, m.weight, bias, m.stride, m.padding, m.dilation, m.groups)


def _plain_conv(m):
    return isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)) and m.padding_mode == "zeros" and not isinstance(m.padding, str)


def _run(mods, x, out=None, widen=False):
    """The fused route over a flat list of modules.  ``out``: a channel slice the LAST convolution run writes its epilogue into
    (the upper half of a level's buffer).  ``widen``: the last run allocates ``[N, 2C, H, W]``, fills channels ``[0, C)`` and
    answers the whole buffer.  A run that is followed by a pix2pix level is widened for that level the same way."""
    from . import ops
    i, filled = 0, False
    while i < len(mods):
        m = mods[i]
        if isinstance(m, SkipLevel):
            if m.route == "cat_input":
                if not filled:              # the level's input did not come from a convolution run: place it
                    buf = x.new_empty((x.shape[0], 2 * x.shape[1]) + tuple(x.shape[2:]))
                    buf[:, :x.shape[1]].copy_(x)
                    x = buf
                x = m.fused_cat_input(x)
            else:
                x = m.fused_cat_mid(x)
            i, filled = i + 1, False
            continue
        if not _plain_conv(m):
            x, i, filled = m(x), i + 1, False
            continue
        j, bn, act, slope = i + 1, None, ops.ACT_NONE, 0.0
        if j < len(mods) and isinstance(mods[j], nn.BatchNorm2d):
            bn, j = mods[j], j + 1
        if j < len(mods) and isinstance(mods[j], nn.Dropout):          # identity at inference
            j += 1
        if j < len(mods) and isinstance(mods[j], nn.ReLU):
            act, j = ops.ACT_RELU, j + 1
        elif j < len(mods) and isinstance(mods[j], nn.LeakyReLU):
            act, slope, j = ops.ACT_LEAKY, mods[j].negative_slope, j + 1
        last = j == len(mods)
        feeds_level = not last and isinstance(mods[j], SkipLevel) and mods[j].route == "cat_input"
        dest = out if last else None
        if bn is None and act == ops.ACT_NONE and dest is None and not (last and widen) and not feeds_level:
            x, i, filled = m(x), j, False                             # a bare convolution: nothing to fold
            continue
        y = _convolve(m, x, with_bias=bn is not None).contiguous()
        if feeds_level or (last and widen):
            buf = y.new_empty((y.shape[0], 2 * y.shape[1]) + tuple(y.shape[2:]))
            dest, filled = buf[:, :y.shape[1]], feeds_level
        else:
            buf, filled = None, False
        if dest is None:
            dest = y
        if bn is not None:
            ops.bn_act_into(y, dest, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, act, slope)
        else:
            ops.bn_act_into(y, dest, None, None, None, m.bias, 0.0, act, slope)
        x = buf if buf is not None else dest
        i = j
    return x


class SkipLevel(nn.Module):
    """One level of a U-Net: named children (``LEVELS``) and one of two ways the skip connection joins.

    ``cat_input``: the level answers ``x || f(x)``, f = its children in order.  ``cat_mid``: ``upconv(x1 || convT(nested(pool(x1))))``
    with ``x1 = downconv(x)``."""

    def __init__(self, route, children, upsample=None):
        super().__init__()
        self.route = route
        self.upsample = upsample
        for name, mod in children:
            self.add_module(name, mod)

    def forward(self, x):
        if self.route == "cat_input":
            return torch.cat([x, _chain(self.named_children(), x, self.upsample)], dim=1)
        x1 = self.downconv(x)
        return self.upconv(torch.cat([x1, self.convT(self.nested(self.pool(x1)))], dim=1))

    def fused_cat_input(self, buf):
        """``buf [N, 2C, H, W]`` holds the level's input in channels ``[0, C)``; the upper half is written here."""
        c = buf.shape[1] // 2
        x, size = buf[:, :c], buf.shape[-2:]
        children = list(self.named_children())
        for k, (name, mod) in enumerate(children):
            if self.upsample and name == "up":
                x = F.interpolate(x, size=size, mode=self.upsample)
            x = _run(_items(mod), x, out=buf[:, c:] if k + 1 == len(children) else None)
        if x.data_ptr() != buf[:, c:].data_ptr():           # the last child did not end in a convolution run
            buf[:, c:].copy_(x)
        return buf

    def fused_cat_mid(self, x):
        buf = _run(_items(self.downconv), x, widen=True)
        c = buf.shape[1] // 2
        below = _run([self.pool] + _items(self.nested), buf[:, :c])
        up = _run([self.convT], below, out=buf[:, c:])
        if up.data_ptr() != buf[:, c:].data_ptr():
            buf[:, c:].copy_(up)
        return _run(_items(self.upconv), buf)


class UNet(nn.Module):
    """A generator built by ``build_unet``: named children run in order (``up`` after an interpolation back to the input size
    where the label has one)."""

    def __init__(self, meta, children, upsample=None):
        super().__init__()
        self.meta = meta
        self.upsample = upsample
        for name, mod in children:
            self.add_module(name, mod)

    def fused(self, x):
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and not torch.is_grad_enabled() and _fused_unet()
                and _inference(self))

    def forward(self, x):
        if not self.fused(x):
            return _chain(self.named_children(), x, self.upsample)
        size = x.shape[-2:]
        for name, mod in self.named_children():
            if self.upsample and name == "up":
                x = F.interpolate(x, size=size, mode=self.upsample)
            x = _run(_items(mod), x)
        return x


def _constructor(label):
    def init(in_channels, out_channels, **params):
        return build_unet(label, in_channels, out_channels, **params)
    init.__name__ = label
    return init


MODEL_LABELS = {"identity": Identity, **{label: _constructor(label) for label in LABELS}}
