"""The fp16 trunk mode end to end (``precision: f16`` of mdir_amd/networks.py; include/mdx.h, "fp16 trunk"): seeded random
resnet18 (BasicBlock, stem), resnet50 (Bottleneck, downsample) through ``extract_ms`` at scales [1, 1/sqrt(2), 1/2] and vgg11
(conv bias + ReLU) through ``extract_ss``; four images of 96 x 128, as batches of 1 and of 4.

1. ``features`` returns fp16 on an f16 net; descriptors are fp32, finite, unit-norm.
2. Graph replay against eager launches, and batch 1 against batch 4.  The fp32 path promises NO bit identity there
   (tests/test_gpu_api.py::test_graph_replay_extraction_equals_eager: atol 2e-6, "MIOpen is not run-to-run bit-stable"; another
   batch size may get another convolution solver), so none is asserted here either.  What is asserted: the two runs differ by
   no more than e_torch, the distance of torch's own half path from fp32 on the same inputs -- a re-ordered fp16 convolution
   perturbs the descriptor by less than the rounding of every layer does, while a replay that missed the cast or the weights
   (another image's descriptor: 1e-1) is far outside.  Whether the bits were equal is printed.
3. Accuracy, with torch's half path as the yardstick (not the code under test):
       e_ours  = max over images of ||d_f16,fused - d_f32||_inf
       e_torch = the same with MDIR_AMD_FUSED_TRUNK=0: torch's fp16 bn / add / relu, three roundings where mdx_bn_act_f16 has one
   asserted: e_ours <= m * e_torch, m = max(1, 1.5 x the ratio measured on the MI355X) -- the margin is for MIOpen choosing
   other fp16 solvers for slightly different activations.  MEASURED (one MI355X, this file, both batch sizes): RATIO below,
   0.92 / 1.02 / 0.95 for resnet18 / resnet50 / vgg11 -- near 1, not clearly below it.
   And d_f16 != d_f32: the mode really ran.
4. The state dict after an f16 run is fp32 and equal to the one loaded; after ``load_state_dict`` of new weights the cached fp16
   copies are rebuilt and the descriptors change.
"""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS = [1, 2 ** -0.5, 0.5]

# e_ours / e_torch as measured on one MI355X (the larger of batch 1 and batch 4), printed by test_accuracy_against_torchs_half_path
# (two runs of this file; per run and batch size: resnet18 0.92 / 0.77, resnet50 0.83 / 1.00 and 1.02 in the other run, vgg11 0.87 /
# 0.95; e_torch itself is 2.4e-5 .. 8.8e-5 on descriptors whose largest entry is 0.13 .. 0.18).  The ratio is near 1, not well below
# it: the fp16 rounding of the convolutions' outputs, which both paths share, dominates the two extra roundings the fused epilogue saves.
RATIO = {"resnet18": 0.916, "resnet50": 1.022, "vgg11": 0.951}


def margin(arch):
    """m = max(1, 1.5 x the measured ratio): 1.374, 1.533, 1.427."""
    return max(1.0, 1.5 * RATIO[arch])


def make_net(arch, precision, seed=4):
    """Seeded random weights; the BatchNorm statistics and affine parameters random too, so that the epilogue does something."""
    from mdir_amd.networks import init_network
    torch.manual_seed(seed)
    net = init_network({"architecture": arch, "pooling": "gem", "whitening": False, "pretrained": False, "precision": precision})
    g = torch.Generator().manual_seed(seed + 1)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
            with torch.no_grad():
                m.weight.copy_(0.75 + 0.5 * torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.num_features, generator=g))
    return net.to(DEV).eval()


def images():
    return torch.randn(4, 3, 96, 128, generator=torch.Generator().manual_seed(11)).to(DEV)


def describe_fn(net, arch):
    from mdir_amd.networks import extract_ms, extract_ss
    if arch.startswith("vgg"):
        return lambda x: extract_ss(net, x).reshape(x.shape[0], -1)
    msp = net.pool.p_value()
    return lambda x: extract_ms(net, x, MS, msp).reshape(x.shape[0], -1)


def descriptors(net, arch, batch, graphs=False):
    """[4, D] fp32: the four images in batches of ``batch``; ``graphs``: every batch through a captured hipGraph replay."""
    from mdir_amd.graphs import ShapeGraphs
    fn = describe_fn(net, arch)
    x = images()
    with torch.no_grad():
        if graphs:
            sg = ShapeGraphs(fn, warmup=1)
            sg(x[:batch]), sg(x[:batch])                             # eager, capture + first replay
            rows = [sg(x[i:i + batch]) for i in range(0, 4, batch)]
            assert sg.replays == 1 + 4 // batch and len(sg.graphs) == 1 and not sg.refused
        else:
            rows = [fn(x[i:i + batch]) for i in range(0, 4, batch)]
    return torch.cat(rows).clone()


_cache = {}


def run(arch, precision, fused, batch, graphs=False):
    """Computed once per configuration and shared by the tests; ``fused``: MDIR_AMD_FUSED_TRUNK."""
    key = (arch, precision, fused, batch, graphs)
    if key not in _cache:
        old = os.environ.get("MDIR_AMD_FUSED_TRUNK")
        os.environ["MDIR_AMD_FUSED_TRUNK"] = "1" if fused else "0"
        try:
            _cache[key] = descriptors(make_net(arch, precision), arch, batch, graphs).cpu()
        finally:
            if old is None:
                del os.environ["MDIR_AMD_FUSED_TRUNK"]
            else:
                os.environ["MDIR_AMD_FUSED_TRUNK"] = old
    return _cache[key]


def linf(a, b):
    return float((a - b).abs().max())


ARCHS = ["resnet18", "resnet50", "vgg11"]


@pytest.mark.parametrize("arch", ARCHS)
def test_maps_are_fp16_and_descriptors_fp32_unit_norm(arch):
    net = make_net(arch, "f16")
    x = images()
    with torch.no_grad():
        maps = net.trunk(x[:1])
        assert maps.dtype == torch.float16 and net.features(x[:1].half()).dtype == torch.float16
        assert net.features(x[:1]).dtype == torch.float32                        # the modules themselves are fp32: the mode is the cast
        assert make_net(arch, "f32").trunk(x[:1]).dtype == torch.float32
    assert all(p.dtype == torch.float32 for p in net.parameters())
    for batch in (1, 4):
        d = run(arch, "f16", True, batch)
        assert d.dtype == torch.float32 and d.shape == (4, net.meta["outputdim"]) and bool(torch.isfinite(d).all())
        np.testing.assert_allclose(d.norm(dim=1).numpy(), 1.0, rtol=0, atol=1e-5)


@pytest.mark.parametrize("arch", ARCHS)
def test_accuracy_against_torchs_half_path(arch):
    worst = 0.0
    for batch in (1, 4):
        d32 = run(arch, "f32", True, batch)
        ours, theirs = run(arch, "f16", True, batch), run(arch, "f16", False, batch)
        assert not torch.equal(ours, d32) and not torch.equal(theirs, d32)        # the mode really ran
        e_ours, e_torch = linf(ours, d32), linf(theirs, d32)
        cos = float((1 - (ours * d32).sum(dim=1)).max())
        print("%s batch %d: e_ours %.3e  e_torch %.3e  ratio %.3f  max cosine distance to fp32 %.3e  (largest |d_f32| %.3e)"
              % (arch, batch, e_ours, e_torch, e_ours / e_torch, cos, float(d32.abs().max())))
        worst = max(worst, e_ours / e_torch)
        assert e_torch > 0 and e_ours <= margin(arch) * e_torch, (arch, batch, e_ours, e_torch, margin(arch))
    print("%s: measured ratio (max of the batch sizes) %.3f, margin %.3f" % (arch, worst, margin(arch)))


def repeat_atol(arch):
    """What two f16 evaluations of one network on one input may differ by (docstring, 2): 2^-10 x the largest fp32 entry."""
    return 2.0 ** -10 * float(run(arch, "f32", True, 4).abs().max())


@pytest.mark.parametrize("arch", ARCHS)
def test_graph_replay_and_batch_size_agree_to_one_fp16_step(arch):
    atol = repeat_atol(arch)
    eager1, eager4 = run(arch, "f16", True, 1), run(arch, "f16", True, 4)
    for batch, eager in ((1, eager1), (4, eager4)):
        replay = run(arch, "f16", True, batch, graphs=True)
        d = linf(replay, eager)
        print("%s batch %d: graph replay against eager %.3e (bit-identical: %s); atol %.3e" % (arch, batch, d, torch.equal(replay, eager), atol))
        assert d <= atol, (arch, batch, d, atol)
    d = linf(eager1, eager4)
    print("%s: batch 1 against batch 4 %.3e (bit-identical: %s); atol %.3e" % (arch, d, torch.equal(eager1, eager4), atol))
    assert d <= atol, (arch, d, atol)


def test_state_dict_stays_fp32_and_new_weights_rebuild_the_half_copies():
    arch = "resnet18"
    net = make_net(arch, "f16")
    loaded = copy.deepcopy(net.state_dict())
    first = descriptors(net, arch, 4)
    after = net.state_dict()
    assert after.keys() == loaded.keys()
    for k, v in after.items():
        assert v.dtype == loaded[k].dtype and (not v.is_floating_point() or v.dtype == torch.float32), k
        assert torch.equal(v, loaded[k]), k
    convs = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    assert convs and all(torch.equal(m._mdx_w16[1], m.weight.detach().half()) for m in convs)
    old_copies = [m._mdx_w16[1] for m in convs]
    other = make_net(arch, "f32", seed=9).state_dict()                       # an fp32 checkpoint of other weights
    net.load_state_dict(other)
    second = descriptors(net, arch, 4)
    assert all(m._mdx_w16[1] is not o and torch.equal(m._mdx_w16[1], m.weight.detach().half()) for m, o in zip(convs, old_copies))
    assert linf(first, second) > 1e-3                                        # other weights, other descriptors
    fresh = descriptors(make_net(arch, "f16", seed=9), arch, 4)             # and they are those of a net built with them
    atol = 2.0 ** -10 * float(fresh.abs().max())                                 # as repeat_atol, for these weights
    assert linf(second, fresh) <= atol, (linf(second, fresh), atol)
    assert all(v.dtype == torch.float32 for v in net.state_dict().values() if v.is_floating_point())
