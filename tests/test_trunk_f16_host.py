"""The fp16 trunk mode (include/mdx.h, "fp16 trunk"; ``precision: f16`` of mdir_amd/networks.py) on a CPU-only box: the census
of include/mdx_trunk_f16.h -- which tests/test_cabi.py and tests/test_memguard_host.py do not see -- the argument checks of its
entry points and of the wrappers, and the host side of the mode: the key, its refusals, fp32 parameters, the scenario overlay."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ("mdx_bn_act_f16", "mdx_pool_l2n_f16", "mdx_pool_multi_f16")


def _declared():
    """The code of include/mdx_trunk_f16.h, the prototypes that mdx.h includes for its section "fp16 trunk"."""
    assert re.search(r'^#include "mdx_trunk_f16.h"$', open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.M)
    text = open(os.path.join(ROOT, "include", "mdx_trunk_f16.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_f16_entry_points():
    from mdir_amd import _lib
    code = _declared()
    assert re.search(r"int\s+mdx_bn_act_f16\s*\(\s*__half \*x,\s*const __half \*residual,\s*int64_t N,\s*int64_t C,\s*int64_t HW,"
                     r"\s*const float \*mean,\s*const float \*var,\s*const float \*weight,\s*const float \*bias,\s*float eps,"
                     r"\s*int relu,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+mdx_pool_l2n_f16\s*\(\s*const __half \*feat,", code)
    assert re.search(r"int\s+mdx_pool_multi_f16\s*\(\s*const __half \*const \*feats,", code)
    for name in NEW:
        assert name in _lib.TRUNK_F16_EXPORTS
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert "fp16 trunk" in text and "rounded ONCE" in text and "BIT FOR BIT" in text and "LABELLED" in text
    assert "#define MDX_ABI_VERSION 3" in text                                          # additive: the version stays


def test_every_f16_entry_point_is_covered():
    """Every prototype of include/mdx_trunk_f16.h is exported and bound (apart from mdx.h's own), none is a size function, and
    each has at least two memory-contract cases, one of them the stale pre-fill of the others."""
    from mdir_amd import _lib
    from test_gpu_trunk_f16_memcontract import CASES, COVERED
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", _declared()))
    assert declared == set(_lib.TRUNK_F16_EXPORTS) == set(NEW)
    assert not declared & set(_lib.EXPORTS) and not declared & set(_lib.KNN_JOIN_EXPORTS)
    assert not {n for n in declared if "_workspace" in n}
    assert {"mdx_" + entry for entry in COVERED} == declared
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


def test_library_exports_and_binds_the_f16_entry_points():
    from mdir_amd import _lib
    _lib.build()
    h = _lib.lib()
    for name in NEW:
        fn = getattr(h, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    assert len(h.mdx_bn_act_f16.argtypes) == len(h.mdx_bn_act.argtypes)
    assert len(h.mdx_pool_l2n_f16.argtypes) == len(h.mdx_pool_l2n.argtypes)
    assert len(h.mdx_pool_multi_f16.argtypes) == len(h.mdx_pool_multi.argtypes)
    assert h.mdx_abi_version() == _lib.ABI_VERSION == 3


def test_refusals_before_any_device_work():
    from mdir_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(256)
    assert h.mdx_bn_act_f16(None, None, 1, 1, 8, None, None, None, None, 1e-5, 1, None) == -1 and b"mdx_bn_act_f16: NULL" in h.mdx_last_error()
    assert h.mdx_bn_act_f16(p, None, 1, 1, 8, p, None, None, None, 1e-5, 1, None) == -1 and b"mean and var" in h.mdx_last_error()
    assert h.mdx_bn_act_f16(p, None, 0, 1, 8, None, None, None, None, 1e-5, 1, None) == -1 and b"positive" in h.mdx_last_error()
    assert h.mdx_bn_act_f16(p, None, 1, 1, 1 << 31, None, None, None, None, 1e-5, 1, None) == -1 and b"too large" in h.mdx_last_error()
    assert h.mdx_bn_act_f16(p, None, 1, 1, 8, None, None, None, None, -1.0, 1, None) == -1 and b"eps" in h.mdx_last_error()
    assert h.mdx_pool_l2n_f16(None, 1, 1, 1, 1, 0, 3.0, 1e-6, 1e-6, None, None) == -1 and b"mdx_pool_l2n_f16: NULL" in h.mdx_last_error()
    assert h.mdx_pool_l2n_f16(p, 1, 1, 0, 1, 0, 3.0, 1e-6, 1e-6, p, None) == -1 and b"bad shape" in h.mdx_last_error()
    assert h.mdx_pool_l2n_f16(p, 1, 1, 1, 1, 0, -3.0, 1e-6, 1e-6, p, None) == -1 and b"gem needs" in h.mdx_last_error()
    assert h.mdx_pool_l2n_f16(p, 1, 1, 1, 1, 7, 3.0, 1e-6, 1e-6, p, None) == -1 and b"unknown pooling kind" in h.mdx_last_error()
    one = (ctypes.c_int * 1)(2)
    ptrs = (ctypes.c_void_p * 1)(256)
    none = (ctypes.c_void_p * 1)(None)
    assert h.mdx_pool_multi_f16(None, 1, 1, 1, one, one, 0, 3.0, 1e-6, p, None) == -1 and b"mdx_pool_multi_f16: NULL" in h.mdx_last_error()
    assert h.mdx_pool_multi_f16(ptrs, 9, 1, 1, one, one, 0, 3.0, 1e-6, p, None) == -1 and b"1..8" in h.mdx_last_error()
    assert h.mdx_pool_multi_f16(none, 1, 1, 1, one, one, 0, 3.0, 1e-6, p, None) == -1 and b"map 0 is NULL" in h.mdx_last_error()
    assert h.mdx_pool_multi_f16(ptrs, 1, 1, 1, one, one, 5, 3.0, 1e-6, p, None) == -1 and b"unknown pooling kind" in h.mdx_last_error()
    # the fp32 entry points still name themselves
    assert h.mdx_pool_l2n(None, 1, 1, 1, 1, 0, 3.0, 1e-6, 1e-6, None, None) == -1 and b"mdx_pool_l2n: NULL" in h.mdx_last_error()
    assert h.mdx_bn_act(None, None, 1, 1, 8, None, None, None, None, 1e-5, 1, None) == -1 and b"mdx_bn_act: NULL" in h.mdx_last_error()


def test_wrapper_checks_need_no_gpu(monkeypatch):
    import torch
    from mdir_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pool_l2n(torch.zeros(1, 2, 3, 3, dtype=torch.float16), "gem")
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.bn_act_(torch.zeros(1, 2, 3, 3, dtype=torch.float16), None, None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    half, full = torch.zeros(1, 2, 3, 3, dtype=torch.float16), torch.zeros(1, 2, 3, 3)
    for a, b in ((half, full), (full, half)):
        with pytest.raises(ValueError, match="share a dtype"):
            ops.pool_multi([a, b], "gem")
        with pytest.raises(ValueError, match="residual must be contiguous fp(16|32) and shaped like x"):
            ops.bn_act_(a, None, None, residual=b)
    stats16 = torch.zeros(2, dtype=torch.float16)
    with pytest.raises(ValueError, match="running_mean must be 2 contiguous fp32 values"):
        ops.bn_act_(half, stats16, stats16)
    with pytest.raises(ValueError, match="bias must be 2 contiguous fp32 values"):
        ops.bn_act_(half, None, None, None, stats16)
    with pytest.raises(ValueError, match="fp32 .or fp16."):
        ops.bn_act_(half.double(), None, None)
    with pytest.raises(TypeError, match="must be torch.float32"):
        ops.pool_l2n(half.double(), "gem")


# ------------------------------------------------------------------ the mode's host side

def test_init_network_records_the_precision_and_keeps_parameters_fp32():
    import torch
    from mdir_amd.networks import init_network
    base = {"architecture": "resnet18", "pooling": "gem", "whitening": True, "pretrained": False}
    assert init_network(dict(base)).meta["precision"] == "f32"                          # the default
    assert init_network(dict(base, precision="f32")).meta["precision"] == "f32"
    for arch in ("resnet18", "resnet50", "vgg11", "alexnet"):
        net = init_network(dict(base, architecture=arch, precision="f16"))
        assert net.meta["precision"] == "f16" and "precision: f16" in repr(net)
        assert all(t.dtype == torch.float32 for t in net.state_dict().values() if t.is_floating_point())
        assert all(p.dtype == torch.float32 for p in net.parameters())
    assert "precision: f32" in repr(init_network(dict(base)))
    torch.manual_seed(1)
    a = init_network(dict(base)).state_dict()
    torch.manual_seed(1)
    b = init_network(dict(base, precision="f16")).state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)                # the same checkpoint either way


def test_bad_precision_raises():
    from mdir_amd.networks import init_network
    for bad in ("fp16", "half", "bf16", 16, None, True, ""):
        with pytest.raises(ValueError, match="precision: 'f32' or 'f16'"):
            init_network({"architecture": "resnet18", "pretrained": False, "precision": bad})
    net = init_network({"architecture": "resnet18", "pretrained": False})
    with pytest.raises(ValueError, match="precision: 'f32' or 'f16'"):
        net.set_precision("f64")
    assert net.meta["precision"] == "f32" and net.set_precision("f16").meta["precision"] == "f16"


@pytest.mark.parametrize("arch", ["densenet121", "squeezenet1_1", "squeezenet1_0"])
def test_f16_is_limited_to_the_routed_architectures(arch):
    from mdir_amd.networks import init_network
    with pytest.raises(ValueError, match="precision 'f16' is limited to alexnet, resnet101.*'%s'" % arch):
        init_network({"architecture": arch, "pretrained": False, "precision": "f16"})
    net = init_network({"architecture": arch, "pretrained": False})                        # fp32 as before
    with pytest.raises(ValueError, match="limited to"):
        net.set_precision("f16")


def test_f16_convolution_uses_a_cached_half_copy_keyed_like_the_transposed_weights():
    """``backbones._conv`` on the host: fp32 input takes the module as it is; fp16 input meets an fp16 copy that is rebuilt when
    the parameter is modified in place or replaced; parameters stay fp32."""
    import torch
    from mdir_amd import backbones
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(3, 4, 3, padding=1)
    x = torch.randn(1, 3, 5, 5)
    with torch.no_grad():
        assert torch.equal(backbones._conv(conv, x), conv(x)) and not hasattr(conv, "_mdx_w16")
        assert torch.equal(backbones._conv(conv, x, with_bias=False), torch.nn.functional.conv2d(x, conv.weight, None, padding=1))
        y = backbones._conv(conv, x.half())
        first = conv._mdx_w16
        assert y.dtype == torch.float16 and first[1].dtype == torch.float16 and conv.weight.dtype == torch.float32
        assert torch.equal(first[1], conv.weight.half()) and torch.equal(first[2], conv.bias.half())
        backbones._conv(conv, x.half())
        assert conv._mdx_w16 is first                                                   # cached
        conv.weight.mul_(2.0)                                                           # in place: the version moves
        backbones._conv(conv, x.half())
        assert conv._mdx_w16 is not first and torch.equal(conv._mdx_w16[1], conv.weight.half())
        second = conv._mdx_w16
        conv.load_state_dict({"weight": torch.ones_like(conv.weight), "bias": torch.zeros_like(conv.bias)})
        backbones._conv(conv, x.half())
        assert conv._mdx_w16 is not second and bool((conv._mdx_w16[1] == 1).all())
        assert "_mdx_w16" not in conv.state_dict() and all(v.dtype == torch.float32 for v in conv.state_dict().values())


def test_cirnet_and_the_runtime_pass_the_precision_through():
    from mdir_amd.network import CirNetwork, SingleNetwork, init_cirnet
    params = {"cir_architecture": "alexnet", "local_whitening": False, "pooling": "gem", "regional": False, "whitening": False,
              "pretrained": False}
    assert init_cirnet(**dict(params)).meta["precision"] == "f32"
    assert init_cirnet(**dict(params, precision="f16")).meta["precision"] == "f16"
    with pytest.raises(ValueError, match="precision"):
        init_cirnet(**dict(params, precision="f8"))
    model = init_cirnet(**dict(params))
    net = CirNetwork(model, SingleNetwork.NetworkParams(dict(params), {"wrappers": "", "precision": "f16"}), "cpu", frozen=True)
    assert net.model.meta["precision"] == "f16"
    with pytest.raises(ValueError, match="precision"):
        CirNetwork(init_cirnet(**dict(params)), SingleNetwork.NetworkParams(dict(params), {"wrappers": "", "precision": "int8"}), "cpu", frozen=True)


def test_f16_trunk_overlay_parses():
    import yaml
    from mdir_amd.scenario import dict_deep_overlay
    with open(os.path.join(ROOT, "scenarios", "eval.yml")) as f:
        base = yaml.safe_load(f)
    with open(os.path.join(ROOT, "scenarios", "eval_f16_trunk.yml")) as f:
        overlay = yaml.safe_load(f)
    assert overlay == {"network": {"runtime": {"precision": "f16"}}}
    merged = dict_deep_overlay(base, overlay)
    assert merged["network"]["runtime"]["precision"] == "f16"
    assert set(merged["network"]["runtime"]["wrappers"]["eval"]) == {"0_cirwhiten", "1_cirmultiscale"}      # the rest of eval.yml stays
    assert set(merged["validation"]) >= {"roxford5k", "rparis6k", "247tokyo1k"}
