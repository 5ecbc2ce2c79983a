"""The trainable tail on the device (include/mdx_train.h; mdir_amd/autograd.py, criterion.py, training.py): the graph is connected,
the autograd route returns the bits of the no_grad route, and the four kernels agree with the reference's float64 autograd results
(tests/golden/g20_train.npz) and with the float64 restatement (tests/train_restatement.py) at every shape where they take another
path.

Bounds.  `e32` is the error of the reference's op sequence run in fp32 against its float64 run (from the fixture where the case is
in it, else the same sequence -- train_restatement's torch half -- run on the CPU here), floored at one ulp of the array's largest
magnitude; the kernels must stay within 4 e32 of the float64 result: the factor covers another summation order and nothing else.
GeM with p = 2.92 evaluates x^p through the hardware exp2 / log2 units like the forward, and has the forward's pinned bound, 1e-5 of the
array's largest magnitude (test_gpu_kernels.py::test_pool_l2n_golden); grad_p is a difference of two terms and is bounded by 1e-5 of
the sum of their magnitudes.  Every test prints the figures it asserts on."""
import numpy as np
import pytest
import torch

import train_restatement as TR
from test_train_host import KINDS, loss_cases, tail_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
EPS = 1e-6
PLANES = [(1, 1), (1, 3), (2, 2), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (257, 1), (17, 23), (24, 32)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def feature_map(seed, shape):
    """ReLU-like: U(0,1) with about half the entries zero (below eps: the clamp's dead side)."""
    rng = np.random.default_rng(seed)
    return (rng.random(shape, dtype=F32) * (rng.random(shape, dtype=F32) > 0.5)).astype(F32)


def within(name, got, ref64, bound, report):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref64, np.float64)).max()) if np.size(ref64) else 0.0
    report.append("%s err %.3g bound %.3g" % (name, err, bound))
    return err <= bound


def gem_bound(p, ref64, ref32):
    """4 e32 for the exact exponents, the forward's 1e-5 of the largest magnitude for the transcendental one."""
    return 4 * TR.e32(ref32, ref64) if p in (1.0, 2.0, 3.0) else 1e-5 * float(np.abs(ref64).max())


# ------------------------------------------------------------------ the graph

@pytest.fixture(scope="module")
def small_net():
    from mdir_amd.networks import init_network
    from mdir_amd.training import set_batchnorm_eval
    torch.manual_seed(5)
    net = init_network({"architecture": "resnet18", "pooling": "gem", "whitening": True, "pretrained": False}).to(DEV)
    net.train()
    net.apply(set_batchnorm_eval)
    return net


def test_the_graph_is_connected(small_net):
    from mdir_amd.criterion import ContrastiveLoss
    from mdir_amd.training import tuple_step
    net = small_net
    net.zero_grad(set_to_none=True)
    torch.manual_seed(6)
    out = net(torch.rand(1, 3, 64, 64, device=DEV))
    assert out.requires_grad and out.grad_fn is not None and tuple(out.shape) == (net.meta["outputdim"], 1)
    images = [torch.rand(1, 3, 64, 64) for _ in range(3)]
    loss = tuple_step(net, ContrastiveLoss(), images, torch.tensor([-1.0, 1.0, 0.0]))
    assert isinstance(loss, float) and np.isfinite(loss) and loss > 0
    names = [n for n, _ in net.named_parameters()]
    assert "pool.p" in names and "whiten.weight" in names and any(n.startswith("features.") for n in names)
    for name, param in net.named_parameters():
        assert param.grad is not None and bool(torch.isfinite(param.grad).all()), name
    assert float(net.pool.p.grad.abs()) > 0 and float(net.whiten.weight.grad.abs().max()) > 0
    print("loss %.6f, pool.p.grad %.6g" % (loss, float(net.pool.p.grad)))


def test_forward_bits_are_those_of_the_no_grad_route():
    import torch.nn as nn
    from mdir_amd import layers
    from mdir_amd.networks import ImageRetrievalNet
    torch.manual_seed(7)
    c = 40
    meta = {"architecture": "toy", "local_whitening": False, "pooling": "gem", "regional": False, "whitening": True, "outputdim": c}
    feat = dev(feature_map(1, (3, c, 7, 9)))
    for pool in (layers.GeM(p=3.0), layers.GeM(p=2.92), layers.MAC(), layers.SPoC()):
        for lin in (None, nn.Linear(c, c), nn.Linear(c, c, bias=False)):
            net = ImageRetrievalNet([nn.Identity()], None, pool, lin, dict(meta)).to(DEV)
            with torch.no_grad():
                want = net(feat)
            got = net(feat.clone().requires_grad_(True))
            assert got.requires_grad and not want.requires_grad
            assert torch.equal(got.detach(), want), (pool, lin)
            if isinstance(pool, layers.GeM) or lin is not None:            # parameters alone ask for the route, the map need not
                assert net(feat).requires_grad and torch.equal(net(feat).detach(), want)
        x = feat.clone().requires_grad_(True)
        with torch.no_grad():
            want = pool(feat), layers.l2n(pool(feat))
        got = pool(x), layers.l2n(pool(x))
        assert all(g.requires_grad and torch.equal(g.detach(), w) and g.shape == w.shape for g, w in zip(got, want)), pool
    x = feat.clone().requires_grad_(True)
    p = torch.tensor([2.5], device=DEV, requires_grad=True)
    with torch.no_grad():
        want = layers.gem(feat, p), layers.mac(feat), layers.spoc(feat)
    for got, w in zip((layers.gem(feat, p), layers.mac(x), layers.spoc(x)), want):
        assert got.requires_grad and torch.equal(got.detach(), w)
    with pytest.raises(NotImplementedError, match="precision: f32"):
        layers.mac(feat.half().requires_grad_(True))


# ------------------------------------------------------------------ mdx_pool_bwd

def pool_case(ops, x, gy, kind, p, report, tag):
    """One call against the restatement; the bounds of the module docstring."""
    xd, gd = dev(x), dev(gy)
    pooled = ops.pool_l2n(xd, kind, p, EPS, l2n_eps=None)
    gx, gp = ops.pool_bwd(xd, pooled, gd, kind, p, EPS)
    want_x, want_p, mag = TR.pool_bwd64(x, gy, kind, p, EPS)
    ok = True
    if kind == "mac":
        ok &= np.array_equal(host(gx), want_x.astype(F32)) and gp is None
    elif kind == "spoc":
        ok &= np.array_equal(host(gx), np.broadcast_to((gy / F32(x.shape[2] * x.shape[3]))[:, :, None, None], x.shape)) and gp is None
    else:
        if p in (1.0, 2.0, 3.0):
            ref32 = TR.torch_grads(lambda a: TR.pool_torch(a, kind, p, EPS), [x], gy)[0]
        else:
            ref32 = None
        ok &= within("%s gx" % tag, host(gx), want_x, gem_bound(p, want_x, ref32), report)
        ok &= within("%s gp" % tag, host(gp)[0], want_p, 1e-5 * mag, report)
        ok &= bool((host(gx)[x < F32(EPS)] == 0).all())                 # exactly 0 below eps
    return ok


@pytest.mark.parametrize("h,w", PLANES, ids=["%dx%d" % hw for hw in PLANES])
def test_pool_bwd_against_the_restatement(h, w):
    from mdir_amd import ops
    report, bad = [], []
    for c in (1, 5, 257):
        for b in (1, 3):
            x = feature_map(h * 1000 + w * 10 + c + b, (b, c, h, w))
            gy = np.random.default_rng(c * 7 + b).standard_normal((b, c)).astype(F32)
            for name, (kind, p) in KINDS.items():
                tag = "%s b%d c%d %dx%d" % (name, b, c, h, w)
                if not pool_case(ops, x, gy, kind, p, report, tag):
                    bad.append(tag)
    print("\n".join(report))
    assert not bad, bad


def test_pool_bwd_on_slices_and_twice():
    """Planes that start off the 16-byte grid (a channel slice of a larger map, H W % 4 == 0 and odd) give the bits of an aligned
    copy, and two runs give the same bits."""
    from mdir_amd import ops
    for h, w in ((4, 5), (7, 9), (8, 8)):
        big = dev(feature_map(h + w, (2 * 7 * h * w + 3,)))
        for off in (1, 2, 3):
            x = big[off:off + 2 * 7 * h * w].view(2, 7, h, w)
            assert x.data_ptr() % 16 == 4 * off
            gy = torch.randn(2, 7, device=DEV)
            for name, (kind, p) in KINDS.items():
                pooled = ops.pool_l2n(x, kind, p, EPS, l2n_eps=None)
                one = ops.pool_bwd(x, pooled, gy, kind, p, EPS)
                two = ops.pool_bwd(x.clone(), pooled, gy, kind, p, EPS)
                again = ops.pool_bwd(x, pooled, gy, kind, p, EPS)
                for a, b_, c in zip(one, two, again):
                    assert (a is None and b_ is None) or (torch.equal(a, b_) and torch.equal(a, c)), (name, h, w, off)


def test_spoc_and_mac_are_exact_and_the_clamp_is_the_reference_s():
    from mdir_amd import ops
    rng = np.random.default_rng(11)
    gy = rng.standard_normal((2, 3)).astype(F32)
    for h, w in ((1, 1), (2, 2), (8, 8), (16, 16), (4, 64)):               # H W a power of two: the division is exact
        x = feature_map(h, (2, 3, h, w))
        gx, gp = ops.pool_bwd(dev(x), dev(x.mean(axis=(2, 3))), dev(gy), "spoc")
        assert gp is None and np.array_equal(host(gx), np.broadcast_to((gy / F32(h * w))[:, :, None, None], x.shape))
    for h, w in ((3, 5), (8, 8), (17, 23)):
        x = feature_map(h * w, (2, 3, h, w))
        x[0, 0] = 0                                                          # an all-zero plane: element 0
        x[0, 1].reshape(-1)[[h * w - 1, h * w // 2, 1]] = 2.0                # tied maxima: the first in row-major order
        x[1, 2].reshape(-1)[[h * w - 1, h * w - 2]] = 3.0
        gx, _ = ops.pool_bwd(dev(x), dev(x.max(axis=(2, 3))), dev(gy), "mac")
        want = TR.pool_bwd64(x, gy, "mac")[0]
        assert want[0, 0, 0, 0] == gy[0, 0] and want[0, 1].reshape(-1)[1] == gy[0, 1] and want[1, 2].reshape(-1)[h * w - 2] == gy[1, 2]
        assert np.array_equal(host(gx), want.astype(F32)) and int((host(gx) != 0).sum()) == 6
    # GeM: x < eps gives exactly 0, x == eps passes the gradient (eps as the kernel holds it: the fp32 value)
    eps32 = float(F32(EPS))
    for p in (1.0, 2.0, 3.0, 2.92):
        x = feature_map(3, (1, 2, 5, 7))
        x[0, 0, 0, :4] = [F32(EPS), np.nextafter(F32(EPS), F32(0)), 0.0, np.nextafter(F32(EPS), F32(1))]
        x[0, 1] = 0                                                          # an all-zero plane: an all-zero gradient
        xd = dev(x)
        gx, gp = ops.pool_bwd(xd, ops.pool_l2n(xd, "gem", p, EPS, l2n_eps=None), dev(gy[:1, :2]), "gem", p, EPS)
        got = host(gx)
        assert got[0, 0, 0, 0] != 0 and got[0, 0, 0, 1] == 0 and got[0, 0, 0, 2] == 0 and got[0, 0, 0, 3] != 0 and not got[0, 1].any()
        want = TR.pool_bwd64(x, gy[:1, :2], "gem", p, eps32)
        assert float(np.abs(got - want[0]).max()) <= 1e-5 * float(np.abs(want[0]).max()) and abs(float(gp) - want[1]) <= 1e-5 * want[2]


def test_tail_against_the_reference(golden):
    """PoolL2N (mdx_l2n_rows_bwd, then mdx_pool_bwd) on the fixture's maps against the reference's float64 gradients."""
    from mdir_amd import autograd
    g = golden("g20_train.npz")
    report, bad = [], []
    for key, kind, p, x, go in tail_cases(g):
        xd = dev(x).requires_grad_(True)
        pt = torch.tensor([p], device=DEV, requires_grad=True) if kind == "gem" else None
        autograd.PoolL2N.apply(xd, pt, kind, EPS, EPS).backward(dev(go))
        ref64, ref32 = g[key + "_gx64"], g[key + "_gx32"]
        ok = within(key + " gx", host(xd.grad), ref64, gem_bound(p, ref64, ref32) if kind == "gem" else 4 * TR.e32(ref32, ref64), report)
        if kind == "gem":
            ok &= within(key + " gp", host(pt.grad)[0], g[key + "_gp64"][0], 1e-5 * TR.tail_bwd64(x, go, kind, p)[2], report)
        if not ok:
            bad.append(key)
    print("\n".join(report))
    assert not bad, bad


# ------------------------------------------------------------------ mdx_l2n_rows_bwd

@pytest.mark.parametrize("d", [1, 255, 256, 257, 2048])
def test_l2n_rows_bwd(d):
    from mdir_amd import autograd, ops
    report, bad = [], []
    for r in (1, 3):
        rng = np.random.default_rng(d + r)
        x, go, bias = (rng.standard_normal(s).astype(F32) for s in ((r, d), (r, d), (d,)))
        x[r - 1] = 0                                                         # a zero row: grad_out / eps
        want = TR.l2n_bwd64(x, go, EPS)
        ref32 = TR.torch_grads(lambda a: TR.l2n_torch(a, EPS), [x], go)[0]
        got = host(ops.l2n_rows_bwd(dev(x), dev(go), EPS))
        assert np.array_equal(got[r - 1], go[r - 1] / F32(EPS))
        if not within("d%d r%d" % (d, r), got, want, 4 * TR.e32(ref32, want), report):
            bad.append((d, r))
        # with a bias, through autograd: the rows' gradient and the bias' (the column sum)
        xd, bd = dev(x).requires_grad_(True), dev(bias).requires_grad_(True)
        out = autograd.L2NRows.apply(xd, bd, EPS)
        assert torch.equal(out.detach(), ops.l2n_rows_(dev(x), bias=dev(bias), eps=EPS))
        out.backward(dev(go))
        want_x = TR.l2n_bwd64(x.astype(np.float64) + bias, go, EPS)
        ref32 = TR.torch_grads(lambda a, b_: TR.l2n_torch(a + b_, EPS), [x, bias], go)
        if not (within("d%d r%d bias: gx" % (d, r), host(xd.grad), want_x, 4 * TR.e32(ref32[0], want_x), report)
                and within("d%d r%d bias: gb" % (d, r), host(bd.grad), want_x.sum(0), 4 * TR.e32(ref32[1], want_x.sum(0)), report)):
            bad.append((d, r, "bias"))
    print("\n".join(report))
    assert not bad, bad


# ------------------------------------------------------------------ the losses

def tuple_batch(seed, d, s, nq):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((d, s * nq))
    x = x / np.linalg.norm(x, axis=0, keepdims=True) * rng.uniform(0.3, 0.8, s * nq)      # pairs inside and beyond the margins
    return x.astype(F32), np.tile(np.array([-1.0, 1.0] + [0.0] * (s - 2), F32), nq)


def loss_case(kind, x, label, margin, ref, report, tag):
    """ref: (loss64, gx64, loss32, gx32), or None: the restatement and its torch half on the CPU."""
    from mdir_amd import criterion
    mod = criterion.ContrastiveLoss(margin) if kind == "contrastive" else criterion.TripletLoss(margin)
    runs = []
    for _ in range(2):
        xd = dev(x).requires_grad_(True)
        loss = mod(xd, torch.from_numpy(label))
        loss.backward()
        runs.append((host(loss), host(xd.grad)))
    same = runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    if ref is None:
        fn64, fn_t = (TR.contrastive64, TR.contrastive_torch) if kind == "contrastive" else (TR.triplet64, TR.triplet_torch)
        loss64, gx64 = fn64(x, label, margin)
        leaf = torch.tensor(x, requires_grad=True)
        value = fn_t(leaf, torch.from_numpy(label), margin)
        value.backward()
        loss32, gx32 = float(value.detach()), leaf.grad.numpy()
    else:
        loss64, gx64, loss32, gx32 = ref
    ok = within(tag + " loss", runs[0][0], loss64, 4 * TR.e32(loss32, loss64), report)
    ok &= within(tag + " gx", runs[0][1], gx64, 4 * TR.e32(gx32, gx64), report)
    return ok and same


@pytest.mark.parametrize("kind", ["contrastive", "triplet"])
def test_losses(kind, golden):
    g = golden("g20_train.npz")
    report, bad = [], []
    for key, loss in loss_cases(g):
        if loss == kind:
            ref = (float(g[key + "_loss64"]), g[key + "_gx64"], float(g[key + "_loss32"]), g[key + "_gx32"])
            if not loss_case(kind, g[key + "_x"], g[key + "_label"], float(g[key + "_margin"]), ref, report, "g20 " + key):
                bad.append(key)
    margin = 0.7 if kind == "contrastive" else 0.1
    for d in (1, 7, 64, 257, 2048):
        for s in (2, 3, 7):
            for nq in (1, 2, 5):
                if kind == "triplet" and s < 3:
                    continue
                x, label = tuple_batch(d + 10 * s + nq, d, s, nq)
                tag = "%s d%d s%d q%d" % (kind, d, s, nq)
                if not loss_case(kind, x, label, margin, None, report, tag):
                    bad.append(tag)
    print("\n".join(report))
    assert not bad, bad


# ------------------------------------------------------------------ end to end

def test_tuple_step_against_the_torch_tail(small_net):
    """The HIP tail and the HIP loss behind the trunk against the same trunk followed by the restatement's torch ops: the gradient that
    reaches the trunk's output and pool.p.grad, each held to the float64 chain from that output on within the bounds above."""
    from mdir_amd.criterion import ContrastiveLoss
    net = small_net
    eps = net.norm.eps
    torch.manual_seed(8)
    images = [torch.rand(1, 3, 64, 64, device=DEV) for _ in range(3)]
    label = torch.tensor([-1.0, 1.0, 0.0])
    maps = []

    def keep(module, inputs, output):           # (returns None: the output goes on as it is)
        output.retain_grad()
        maps.append(output)
    hook = net.features.register_forward_hook(keep)
    try:
        net.zero_grad(set_to_none=True)
        loss = ContrastiveLoss()(torch.cat([net(im) for im in images], dim=1), label)
        loss.backward()
        hip = [host(o.grad) for o in maps], float(net.pool.p.grad), float(loss.detach())
        del maps[:]
        net.zero_grad(set_to_none=True)
        cols = [TR.tail_torch(net.features(im), "gem", net.pool.p, net.pool.eps, eps, net.whiten.weight, net.whiten.bias).t() for im in images]
        value = TR.contrastive_torch(torch.cat(cols, dim=1), label.to(DEV))
        value.backward()
        base = [host(o.grad) for o in maps], float(net.pool.p.grad), float(value.detach())
        feats = [host(o) for o in maps]
    finally:
        hook.remove()
        net.zero_grad(set_to_none=True)
    # float64, from the trunk's output on
    p64 = torch.tensor(host(net.pool.p).astype(np.float64), requires_grad=True)
    w64, b64 = net.whiten.weight.detach().double().cpu(), net.whiten.bias.detach().double().cpu()
    leaves = [torch.tensor(f.astype(np.float64), requires_grad=True) for f in feats]
    pooled = [TR.pool_torch(o, "gem", p64, net.pool.eps) for o in leaves]
    for y in pooled:
        y.retain_grad()
    cols = [TR.l2n_torch(torch.nn.functional.linear(TR.l2n_torch(y, eps), w64, b64), eps).t() for y in pooled]
    value64 = TR.contrastive_torch(torch.cat(cols, dim=1), label.double())
    value64.backward()
    magnitude = sum(TR.pool_bwd64(f, y.grad.numpy(), "gem", float(p64.detach()), net.pool.eps)[2] for f, y in zip(feats, pooled))
    report = []
    ok = within("loss", hip[2], float(value64.detach()), 4 * TR.e32(base[2], float(value64.detach())), report)
    for i, leaf in enumerate(leaves):
        ok &= within("d loss / d features(image %d)" % i, hip[0][i], leaf.grad.numpy(), 4 * TR.e32(base[0][i], leaf.grad.numpy()), report)
    ok &= within("pool.p.grad", hip[1], float(p64.grad), 1e-5 * magnitude, report)
    print("\n".join(report))
    assert ok, report
