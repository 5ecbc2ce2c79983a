"""The trainable tail (include/mdx_train.h; mdir_amd/autograd.py, criterion.py, training.py) on a CPU-only box: the float64
restatement against the reference's own autograd results (tests/golden/g20_train.npz), the census of include/mdx_train.h, every
refusal of the C ABI with nothing launched, the label-layout checks of the criteria and the Python checks of the ops wrappers."""
import ctypes
import os
import re

import numpy as np
import pytest

import train_restatement as TR
from conftest import ROOT

NEW = ("mdx_pool_bwd_workspace", "mdx_pool_bwd", "mdx_l2n_rows_bwd", "mdx_tuple_loss_workspace", "mdx_contrastive_loss",
       "mdx_triplet_loss")
KINDS = {"gem1": ("gem", 1.0), "gem2": ("gem", 2.0), "gem3": ("gem", 3.0), "gem2.92": ("gem", 2.92), "mac": ("mac", 1.0), "spoc": ("spoc", 1.0)}


def tail_cases(g):
    """(key prefix, kind, p, x, grad_out) of every tail case of the fixture."""
    for key in sorted(g.files):
        m = re.match(r"tail_(.+)_(b\d+_c\d+_h\d+_w\d+)_gx64$", key)
        if m:
            kind, p = KINDS[m.group(1)]
            yield key[:-5], kind, p, g["x_" + m.group(2)], g["go_" + m.group(2)]


def loss_cases(g):
    """(key prefix, loss) of every loss case."""
    for key in sorted(g.files):
        m = re.match(r"(contrastive|triplet)_d\d+_s\d+_q\d+_x$", key)
        if m:
            yield key[:-2], m.group(1)


def close(got, want, rel):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max()) <= rel * max(float(np.abs(want).max()), 1e-300)


def test_restatement_reproduces_the_reference_in_float64(golden):
    g = golden("g20_train.npz")
    tails = list(tail_cases(g))
    assert len(tails) == 6 * 8
    for key, kind, p, x, go in tails:
        gx, gp, mag = TR.tail_bwd64(x, go, kind, p)
        assert close(gx, g[key + "_gx64"], 1e-12), key
        assert g[key + "_gx64"].dtype == np.float64 and g[key + "_gx32"].dtype == np.float32
        if kind == "gem":
            assert abs(gp - float(g[key + "_gp64"][0])) <= 1e-12 * mag, key
        else:
            assert gp is None and key + "_gp64" not in g.files
    losses = list(loss_cases(g))
    assert len(losses) == 10
    for key, loss in losses:
        fn = TR.contrastive64 if loss == "contrastive" else TR.triplet64
        value, gx = fn(g[key + "_x"], g[key + "_label"], float(g[key + "_margin"]))
        assert abs(value - float(g[key + "_loss64"])) <= 1e-12 * abs(float(g[key + "_loss64"])), key
        assert close(gx, g[key + "_gx64"], 1e-12), key


def test_restatement_torch_ops_are_the_closed_forms():
    """The torch half of the restatement (the baseline on the device) differentiates to the numpy half, in float64."""
    import torch
    rng = np.random.default_rng(0)
    x = rng.random((2, 3, 5, 7)) * (rng.random((2, 3, 5, 7)) > 0.4)
    go = rng.standard_normal((2, 3))
    for kind, p in KINDS.values():
        if kind == "gem":
            gx, gp = TR.torch_grads(lambda a, b: TR.tail_torch(a, kind, b), [x, np.array([p])], go, torch.float64)
        else:
            gx, gp = TR.torch_grads(lambda a: TR.tail_torch(a, kind), [x], go, torch.float64)[0], None
        want = TR.tail_bwd64(x, go, kind, p)
        assert close(gx, want[0], 1e-12), (kind, p)
        assert gp is None or abs(float(gp[0]) - want[1]) <= 1e-12 * want[2]
    cols = rng.standard_normal((9, 8))
    label = np.array([-1, 1, 0, 0] * 2, np.float64)
    lt = torch.tensor(label)
    for fn_t, fn_n in ((lambda a: TR.contrastive_torch(a, lt), TR.contrastive64), (lambda a: TR.triplet_torch(a, lt, 3.0), lambda a, l: TR.triplet64(a, l, 3.0))):
        assert close(TR.torch_grads(fn_t, [cols], None, torch.float64)[0], fn_n(cols, label)[1], 1e-12)
    rows = rng.standard_normal((3, 6))
    rows[1] = 0
    want = TR.l2n_bwd64(rows, go.reshape(1, 6).repeat(3, 0))
    assert np.array_equal(want[1], go.reshape(-1) / 1e-6)                 # a zero row: grad_out / eps


def _declared():
    """The code of include/mdx_train.h, which mdx.h includes for its section "trainable tail"."""
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_train.h"$', text, flags=re.M) and "trainable tail" in text
    assert text.index('#include "mdx_photometric.h"') < text.index('#include "mdx_train.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_train.h")).read(), flags=re.S)


def test_header_exports_and_library_agree():
    from mdir_amd import _lib
    code = _declared()
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.TRAIN_EXPORTS) == set(NEW)
    others = (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS) | set(_lib.GROUPS_EXPORTS)
              | set(_lib.KRECIP_EXPORTS) | set(_lib.PHOTOMETRIC_EXPORTS))
    assert not declared & others
    assert re.search(r"int\s+mdx_l2n_rows_bwd\s*\(\s*const float \*x,\s*const float \*grad_out,\s*int64_t R,\s*int64_t D,\s*float eps,"
                     r"\s*float \*grad_x,\s*void \*stream\s*\)", code)
    assert re.search(r"int64_t\s+mdx_pool_bwd_workspace\s*\(\s*int B,\s*int C\s*\)", code)
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert "mdx_train.hip" in makefile and "include/mdx_train.h" in makefile
    mdx_h = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", mdx_h).group(1)) == 3
    _lib.build()
    h = _lib.lib()
    for name in NEW:
        assert hasattr(h, name) and getattr(h, name).argtypes is not None
    assert h.mdx_abi_version() == 3 == _lib.ABI_VERSION


def test_every_launching_entry_point_has_memory_contract_cases():
    from test_gpu_train_memcontract import CASES, COVERED
    assert {"mdx_" + entry for entry in COVERED} == {n for n in NEW if not n.endswith("_workspace")}
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


def test_workspace_formulas():
    from mdir_amd import _lib
    h = _lib.lib()
    for b, c in ((1, 1), (1, 64), (1, 65), (3, 257), (7, 2048)):
        assert h.mdx_pool_bwd_workspace(b, c) == (4 * b * c + 255) // 256 * 256
    for b, c in ((0, 4), (4, 0), (-1, 4)):
        assert h.mdx_pool_bwd_workspace(b, c) == 0
    for nq in (1, 64, 65, 1000):
        assert h.mdx_tuple_loss_workspace(nq) == (4 * nq + 255) // 256 * 256
    for nq in (0, -3, 1 << 31):
        assert h.mdx_tuple_loss_workspace(nq) == 0


def test_refusals_before_any_device_work():
    """Every MDX_ERR_INVALID / MDX_ERR_WORKSPACE of the section through the C ABI with pointers that are no memory: nothing is
    launched (there is no device here to launch on), and the error names the call."""
    from mdir_amd import _lib
    h = _lib.lib()
    p, ws = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)

    def refused(status, name, *words, code=-1):
        msg = h.mdx_last_error()
        assert status == code and msg.startswith(name.encode() + b":"), (status, msg)
        for w in words:
            assert w.encode() in msg, (w, msg)

    def pool(feat=p, pooled=p, gy=p, b=2, c=3, hh=4, w=5, kind=0, pw=3.0, eps=1e-6, gx=ctypes.c_void_p(1 << 22), gp=p, wsp=ws, wsb=4096):
        return h.mdx_pool_bwd(feat, pooled, gy, b, c, hh, w, kind, pw, eps, gx, gp, wsp, wsb, None)
    name = "mdx_pool_bwd"
    for kw in ({"feat": None}, {"pooled": None}, {"gy": None}, {"gx": None}, {"gp": None}):
        refused(pool(**kw), name, "NULL")
    for kw in ({"b": 0}, {"c": -1}, {"hh": 0}, {"w": 0}):
        refused(pool(**kw), name, "bad shape")
    refused(pool(hh=1 << 16, w=1 << 15), name, "H*W too large")
    for kind in (3, -1, 17):
        refused(pool(kind=kind), name, "unknown pooling kind")
    for kw in ({"pw": 0.0}, {"pw": -1.0}, {"eps": 0.0}):
        refused(pool(**kw), name, "p > 0 and eps > 0")
    for gx in (1 << 20, (1 << 20) + 4, (1 << 20) - 4):
        refused(pool(gx=ctypes.c_void_p(gx)), name, "overlaps")
    refused(pool(wsb=255), name, "workspace", code=-4)
    refused(pool(wsp=None), name, "workspace", code=-4)
    refused(pool(wsp=ctypes.c_void_p((1 << 24) + 8)), name, "16-byte aligned")
    for kind in (1, 2):                                                  # MAC / SPoC take neither grad_p nor a workspace: only the shape is left to refuse
        refused(pool(kind=kind, gp=None, wsp=None, wsb=0, b=0), name, "bad shape")

    def l2n(x=p, g=p, r=3, d=8, eps=1e-6, gx=p):
        return h.mdx_l2n_rows_bwd(x, g, r, d, eps, gx, None)
    name = "mdx_l2n_rows_bwd"
    for kw in ({"x": None}, {"g": None}, {"gx": None}):
        refused(l2n(**kw), name, "NULL")
    for kw in ({"r": 0}, {"d": 0}, {"r": -2}, {"r": 1 << 31}):
        refused(l2n(**kw), name, "R=")
    refused(l2n(eps=-1e-6), name, "eps=")

    for fn, name, min_s in ((lambda x, l, d, n, nq, loss, gx, w, wb: h.mdx_contrastive_loss(x, l, d, n, nq, 0.7, 1e-6, loss, gx, w, wb, None),
                             "mdx_contrastive_loss", 2),
                            (lambda x, l, d, n, nq, loss, gx, w, wb: h.mdx_triplet_loss(x, l, d, n, nq, 0.1, loss, gx, w, wb, None),
                             "mdx_triplet_loss", 3)):
        def call(x=p, l=p, d=8, n=12, nq=2, loss=p, gx=p, w=ws, wb=256):
            return fn(x, l, d, n, nq, loss, gx, w, wb)
        for kw in ({"x": None}, {"l": None}, {"loss": None}, {"gx": None}):
            refused(call(**kw), name, "NULL")
        for kw in ({"d": 0}, {"n": 0}, {"nq": 0}, {"nq": -1}):
            refused(call(**kw), name, ">= 1")
        refused(call(n=1 << 33, nq=1 << 31), name, "2^31")
        refused(call(n=13), name, "not a multiple")
        refused(call(n=(min_s - 1) * 4, nq=4), name, "at least %d" % min_s)
        refused(call(d=1 << 40, n=1 << 30, nq=1 << 10), name, "overflows")
        refused(call(wb=255), name, "workspace", code=-4)
        refused(call(w=None), name, "workspace", code=-4)
        refused(call(w=ctypes.c_void_p((1 << 24) + 4)), name, "16-byte aligned")


def test_label_layout_is_checked_on_the_host(monkeypatch):
    import torch
    from mdir_amd import criterion, layers
    T = torch.tensor
    assert criterion.tuple_layout(T([-1., 1, 0, 0, -1, 1, 0, 0]), 8) == (2, 4)
    assert criterion.tuple_layout([T([-1., 1, 0]), T([-1., 0, 1])], 6, "triplet") == (2, 3)          # the positive anywhere in its tuple
    assert criterion.tuple_layout(T([-1., 1, -1, 0]), 4) == (2, 2)
    for label, n, kind, word in ((T([1., -1, 0, 0, -1, 1, 0, 0]), 8, "contrastive", "every S-th column"),
                                 (T([-1., 1, 0, -1, 1, 0, 0, 0]), 8, "contrastive", "every S-th column"),
                                 (T([-1., 1, 0, -1, 1, 0, -1]), 7, "contrastive", "not divisible"),
                                 (T([1., 0, 0]), 3, "contrastive", "no query"),
                                 (T([-1., 1, 0]), 4, "contrastive", "3 labels for 4 columns"),
                                 (T([-1., 2, 0]), 3, "contrastive", "-1 .query., 1 .positive. or 0"),
                                 (T([-1., -1]), 2, "contrastive", "at least 2"),
                                 (T([-1., 1, -1, 1]), 4, "triplet", "at least 3"),
                                 (T([-1., 1, 1, -1, 1, 0]), 6, "triplet", "exactly one positive.*tuple 0 has 2"),
                                 (T([-1., 1, 0, -1, 0, 0]), 6, "triplet", "exactly one positive.*tuple 1 has 0")):
        with pytest.raises(ValueError, match=word):
            criterion.tuple_layout(label, n, kind)
    with pytest.raises(ValueError, match="unknown loss"):
        criterion.tuple_layout(T([-1., 1]), 2, "hinge")
    x = torch.zeros((5, 6))
    for call in (lambda: criterion.ContrastiveLoss()(x, T([-1., 1, 0] * 2)), lambda: criterion.TripletLoss()(x, T([-1., 1, 0] * 2)),
                 lambda: layers.contrastive_loss(x, T([-1., 1, 0] * 2)), lambda: layers.triplet_loss(x, T([-1., 1, 0] * 2))):
        with pytest.raises(RuntimeError, match="CUDA"):                                                # CPU tensors: no fallback
            call()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(ValueError, match="every S-th column"):
        criterion.ContrastiveLoss()(x, T([-1., 1, 0, 0, -1, 1]))
    with pytest.raises(ValueError, match="exactly one positive"):
        layers.triplet_loss(x, [T([-1., 1, 1]), T([-1., 1, 0])])
    with pytest.raises(ValueError, match=r"x must be \[D,N\]"):
        criterion.TripletLoss()(torch.zeros(6), T([-1., 1, 0] * 2))


def test_criterion_modules_and_registry():
    from mdir_amd import criterion, training
    import torch.nn as nn
    c, t = criterion.ContrastiveLoss(), criterion.TripletLoss()
    assert (c.margin, c.eps, t.margin) == (0.7, 1e-6, 0.1) and c.reduction == t.reduction == "sum"
    assert repr(c) == "ContrastiveLoss(margin=0.7000)" and repr(criterion.TripletLoss(0.25)) == "TripletLoss(margin=0.25)"
    assert criterion.CRITERIA == {"contrastive", "triplet"}
    assert criterion.initialize_criterion({}) is None and criterion.initialize_criterion(None) is None
    params = {"loss": "contrastive", "margin": 0.5}
    made = criterion.initialize_criterion(params)
    assert isinstance(made, criterion.ContrastiveLoss) and made.margin == 0.5 and params == {"margin": 0.5}
    assert isinstance(criterion.initialize_criterion({"loss": "triplet"}), criterion.TripletLoss)
    with pytest.raises(ValueError, match="unknown loss"):
        criterion.initialize_criterion({"loss": "mse"})
    net = nn.Sequential(nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4), nn.ReLU()).train()
    net.apply(training.set_batchnorm_eval)
    assert net.training and net[0].training and not net[1].training


def test_ops_checks_need_no_gpu(monkeypatch):
    import torch
    from mdir_amd import ops
    feat, pooled = torch.zeros((2, 3, 4, 5)), torch.zeros((2, 3))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.pool_bwd(feat, pooled, pooled)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.l2n_rows_bwd(pooled, pooled)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.contrastive_loss(torch.zeros((4, 6)), torch.zeros(6), 2)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.triplet_loss(torch.zeros((4, 6)), torch.zeros(6), 2)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(ValueError, match=r"must be \[B,C,H,W\]"):
        ops.pool_bwd(feat[0], pooled, pooled)
    with pytest.raises(ValueError, match=r"pooled and grad_pooled must be \[2,3\]"):
        ops.pool_bwd(feat, pooled[:1], pooled)
    with pytest.raises(ValueError, match="unknown pooling kind 'rmac'"):
        ops.pool_bwd(feat, pooled, pooled, "rmac")
    with pytest.raises(TypeError, match="feature map must be torch.float32"):
        ops.pool_bwd(feat.half(), pooled, pooled)
    with pytest.raises(ValueError, match=r"x and grad_out must be \[R,D\]"):
        ops.l2n_rows_bwd(pooled, torch.zeros((2, 4)))
    for fn, min_s in ((ops.contrastive_loss, 2), (ops.triplet_loss, 3)):
        with pytest.raises(ValueError, match=r"x must be \[D,N\] and label \[N\]"):
            fn(torch.zeros((4, 6)), torch.zeros(5), 2)
        for nq in (0, 4, 2.0, True, 6 // (min_s - 1)):
            with pytest.raises(ValueError, match="tuples of at least %d columns" % min_s):
                fn(torch.zeros((4, 6)), torch.zeros(6), nq)


def test_refusals_under_autograd():
    """What has no backward says so, naming the supported form; without a gradient asked for the present route is taken."""
    import torch
    from mdir_amd import autograd, layers
    x = torch.zeros((1, 2, 4, 4), requires_grad=True)
    for call in (lambda: layers.rmac(x), lambda: layers.RMAC()(x), lambda: layers.roipool(x, layers.MAC()), lambda: layers.Rpool(layers.MAC())(x)):
        with pytest.raises(NotImplementedError, match="gem, mac or spoc"):
            call()
    with pytest.raises(NotImplementedError, match="precision: f32"):
        autograd.PoolL2N.apply(x.half(), None, "mac", 1e-6, None)
    assert autograd.wanted(x) and not autograd.wanted(x.detach(), None)
    with torch.no_grad():
        assert not autograd.wanted(x)
