"""The U-Net generators (mdir_amd/unet.py), SequentialNetwork (mdir_amd/network.py) and the host side of mdx_bn_act_into
(include/mdx_unet.h), without a GPU:

  a. every label's state dict -- keys, order, shapes -- is the reference's (tests/golden/g21_unet.json, written by
     tests/golden/make_golden_unet.py from the reference itself), at the golden configurations and at the defaults;
  b. every label's CPU forward on the golden input equals the reference's output within 2e-5 * max|want| (the bound of
     test_fused_trunk_equals_module_calls: the two run the same torch convolutions, in the same order);
  c. a SequentialNetwork checkpoint in the golden's layout round-trips through load_network;
  d. the numpy restatement of the kernel (tests/unet_restatement.py) is the C statement oracle_bn_act(add_zero = 0) to the bit,
     lies within one ulp of the float64 evaluation (plus, where terms cancel, the statement's own rounding analysis), and is exact on -0, +-inf and NaN;
  e. census: every prototype of include/mdx_unet.h is exported, bound and covered by tests/test_gpu_unet_memcontract.py.
"""
import copy
import ctypes
import itertools
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

import fake_ops  # noqa: F401 (tests dir is on sys.path via conftest)
import unet_restatement as R
from conftest import GOLDEN, ROOT
from oracle import chain as OC

F32 = np.float32
NEW = ("mdx_bn_act_into",)
LABELS = sorted(R.CASES)


@pytest.fixture(scope="module")
def doc():
    with open(os.path.join(GOLDEN, "g21_unet.json")) as f:
        return json.load(f)


def build(label, params=None):
    from mdir_amd.network import initialize_model
    args = {} if label == "identity" else {"in_channels": 3, "out_channels": 3}
    return initialize_model({"architecture": label, **args, **(params or {})})


def keys_and_shapes(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


# ------------------------------------------------------------------------------------------------------------ a. state dicts

@pytest.mark.parametrize("label", LABELS)
def test_state_dict_is_the_references(label, doc):
    assert keys_and_shapes(build(label)) == doc["defaults"][label]
    for k, (params, _) in enumerate(R.CASES[label]):
        assert keys_and_shapes(build(label, params)) == doc["state_dicts"][label][R.case_key(label, k)]
    if label != "identity":
        assert build(label).meta == {"in_channels": 3, "out_channels": 3}


def test_registry_and_constructor_parameters():
    from mdir_amd import network, unet
    assert set(unet.MODEL_LABELS) == set(R.CASES) and set(unet.MODEL_LABELS) < set(network.MODEL_LABELS)
    assert "cirnet" in network.MODEL_LABELS
    with pytest.raises(TypeError, match="unexpected"):
        build("p2p_unet", {"min_channels": 4})
    # the reference's example names
    assert "outerblock.2.nested.0.weight" in build("p2p_unet").state_dict()
    assert "outerblock.downconv.conv1.weight" in build("orig_unet").state_dict()
    # dropout: pix2pix only below the fourth level, the others in every level
    drops = lambda m: sum(isinstance(x, torch.nn.Dropout) for x in m.modules())
    assert drops(build("p2p_unet", {"dropout": 0.5})) == 3 and drops(build("p2p_unet", {"dropout": 0.5, "nested_levels": 4})) == 0
    assert drops(build("outconv_unet", {"dropout": 0.5, "nested_levels": 3})) == 3
    assert drops(build("outconv_dynint_unet", {"dropout": 0.5, "nested_levels": 2})) == 2


# --------------------------------------------------------------------------------------------- b. forward against the reference

@pytest.mark.parametrize("label", LABELS)
def test_cpu_forward_equals_the_reference(label, golden):
    g = golden("g21_unet.npz")
    for k, (params, shape) in enumerate(R.CASES[label]):
        net = R.fill(build(label, params)).eval()
        x = g[R.case_key(label, k) + "_x"]
        want = g[R.case_key(label, k) + "_y"]
        np.testing.assert_array_equal(x, R.case_input(label, k))
        assert x.shape == tuple(shape)
        with torch.no_grad():
            got = net(torch.from_numpy(x)).numpy()
        err = float(np.abs(got - want).max())
        print("%s case %d: max |got - want| = %.3g, bound %.3g" % (label, k, err, 2e-5 * np.abs(want).max()))
        assert got.shape == want.shape and err <= 2e-5 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------- c. checkpoint round trip

UNET_PARAMS = {"architecture": "orig_unet", "in_channels": 3, "out_channels": 3, "nested_levels": 2, "min_channels": 4}
CIR_PARAMS = {"architecture": "cirnet", "cir_architecture": "alexnet", "local_whitening": False, "pooling": "gem", "regional": False,
              "whitening": False, "pretrained": False}


# the data section travels with the FIRST network: the images are normalised for the generator
DATA = {"transforms": "pil2np | totensor | normalize", "mean_std": [[0.485, 0.456, 0.406], [0.229, 0.224, 0.225]]}


def make_checkpoint(path, unet_params=UNET_PARAMS, seed=7):
    """A SequentialNetwork checkpoint file in the reference's layout: the top-level ``net`` entry with the member networks under
    ``_networks_included`` (what load_checkpoint unpacks).  Returns the member states."""
    from mdir_amd.network import initialize_model
    torch.manual_seed(seed)
    unet = R.fill(initialize_model(copy.deepcopy(unet_params)), seed)
    cir = initialize_model(copy.deepcopy(CIR_PARAMS))
    with torch.no_grad():
        cir.pool.p.fill_(2.85)
    members = {
        "unet": {"type": "SingleNetwork", "frozen": True, "model_state": unet.state_dict(),
                 "network_params": {"model": copy.deepcopy(unet_params),
                                    "runtime": {"wrappers": "", "data": copy.deepcopy(DATA)}}},
        "cirnet": {"type": "CirNetwork", "frozen": True, "model_state": cir.state_dict(),
                   "network_params": {"model": copy.deepcopy(CIR_PARAMS), "runtime": {"wrappers": "", "data": {}}}}}
    top = {"type": "SequentialNetwork", "frozen": True, "sequence": ["unet", "cirnet"],
           "network_hierarchy": {"unet": [], "cirnet": []}, "_networks_included": members}
    torch.save(top, path)
    return members


def whitening(path, d, seed=3):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    with open(path, "wb") as f:
        pickle.dump({"P": (q * rng.uniform(0.5, 2.0, (1, d))).T.copy(), "m": rng.normal(0, 0.01, (d, 1))}, f)


@pytest.fixture
def ops(monkeypatch):
    """The kernels of the wrapper chain and the descriptor tail replaced by the oracle (tests/fake_ops.py)."""
    fake_ops.install(monkeypatch)
    return fake_ops


def test_sequential_checkpoint_round_trip(tmp_path, doc, ops):
    from mdir_amd.network import SequentialNetwork, load_network
    from mdir_amd.wrapper import initialize_wrappers
    path, pkl = str(tmp_path / "seq.pth"), str(tmp_path / "whiten.pkl")
    members = make_checkpoint(path)
    whitening(pkl, 256)
    wrappers = {"0_cirwhiten": {"whitening": pkl, "dimensions": None}, "1_cirmultiscale": {"scales": True}}
    data = {"transforms": "pil2np | totensor", "mean_std": [[0, 0, 0], [1, 1, 1]]}
    net = load_network({"path": path, "runtime": {"wrappers": {"train": "", "eval": wrappers}, "data": data}}, "cpu").eval()
    assert isinstance(net, SequentialNetwork) and net.frozen and net.stage == "eval"
    # wrappers reach the last network, data the first; the last network's own chain is emptied
    assert net["cirnet"].network_params.runtime["wrappers"] == {"train": "", "eval": wrappers}
    assert net["unet"].network_params.runtime["data"] == data and net["unet"].network_params.runtime["wrappers"] == ""
    assert net.network_params.runtime == {"wrappers": {"train": "", "eval": wrappers}, "data": data}
    assert len(net.wrappers["eval"].wrappers) == 2 and not net["cirnet"].wrappers["eval"].wrappers
    assert net.model is net["cirnet"].model
    assert net.meta == {"in_channels": 3, "out_channels": net["cirnet"].meta["out_channels"]}
    # net(x) = cirnet(unet(x)) composed by hand through the same wrappers
    # (every level of the three-scale pyramid a multiple of 4: 80 x 136, 56 x 96, 40 x 68 -- two poolings must divide it)
    x = torch.from_numpy(np.random.default_rng(0).random((1, 3, 80, 136), dtype=F32))
    with torch.no_grad():
        got = net(x.clone())
        by_hand = initialize_wrappers(wrappers, "cpu")(x.clone(), lambda t: net["cirnet"].model(net["unet"].model(t)),
                                                        net["cirnet"].model)
    assert got.shape == (256,) and torch.equal(got, by_hand)
    with torch.no_grad():
        assert not torch.equal(got, initialize_wrappers(wrappers, "cpu")(x.clone(), net["cirnet"].model))   # the U-Net matters
    # state_dict(): the golden's structure
    state = net.state_dict()
    want = doc["sequential"]
    assert list(state) == want["keys"]
    assert state["net"] == want["net"]
    for name, entry in want["members"].items():
        assert list(state[name]) == entry["keys"] and state[name]["type"] == entry["type"] and state[name]["frozen"] == entry["frozen"]
        assert state[name]["network_params"].keys() == entry["network_params"].keys()
    assert list(state["unet"]["model_state"]) == want["members"]["unet"]["model_state_keys"]
    assert state["unet"]["network_params"]["model"] == want["members"]["unet"]["network_params"]["model"]
    for key, value in members["unet"]["model_state"].items():
        assert torch.equal(state["unet"]["model_state"][key], value)
    # ... and it loads again
    again = str(tmp_path / "again.pth")
    torch.save({**state.pop("net"), "_networks_included": state}, again)
    net2 = load_network({"path": again, "runtime": None}, "cpu").eval()
    with torch.no_grad():
        assert torch.equal(net2(x.clone()), got)
    # overlay_params swaps the wrappers of the last network only
    over = net.overlay_params({"unet": {}, "cirnet": {"runtime": {"wrappers": "", "data": {}}}}, "cpu")
    assert over is not net and over["unet"] is net["unet"] and over["cirnet"] is not net["cirnet"]
    assert not over.wrappers["eval"].wrappers and len(net.wrappers["eval"].wrappers) == 2 and over.frozen and over.stage == "eval"
    with torch.no_grad():
        assert torch.equal(over(x.clone()), net["cirnet"].model(net["unet"].model(x)))
    assert net.overlay_params(None, "cpu") is net
    kept = net.overlay_params({"unet": {}, "cirnet": {}}, "cpu")
    assert len(kept.wrappers["eval"].wrappers) == 2


def test_sequential_refusals(tmp_path, ops):
    from mdir_amd.network import initialize_network, load_network
    path = str(tmp_path / "seq.pth")
    make_checkpoint(path)
    with pytest.raises(NotImplementedError, match="precision"):
        load_network({"path": path, "runtime": {"precision": "f16"}}, "cpu")
    assert load_network({"path": path, "runtime": {"precision": "f32"}}, "cpu").meta["in_channels"] == 3     # what a sequence runs in
    with pytest.raises(NotImplementedError, match="not a complete SequentialNetwork checkpoint"):
        initialize_network({}, "cpu", state={"net": {"type": "SequentialNetwork"}})
    make_checkpoint(path, {**UNET_PARAMS, "out_channels": 1})
    with pytest.raises(AssertionError):                              # the U-Net answers 1 channel, the embedding takes 3
        load_network({"path": path, "runtime": None}, "cpu")
    make_checkpoint(path, {**UNET_PARAMS, "in_channels": 4})
    with pytest.raises(NotImplementedError, match="in_channels"):
        load_network({"path": path, "runtime": None}, "cpu")


# ------------------------------------------------------------------------------------------------------ d. the restatement

def _params(c, rng):
    return (rng.standard_normal(c).astype(F32), rng.uniform(0.2, 3.0, c).astype(F32),
            (rng.uniform(0.5, 1.5, c) * rng.choice([-1, 1], c)).astype(F32), rng.standard_normal(c).astype(F32))


@pytest.mark.parametrize("shape", [(2, 3, 33), (1, 5, 1024)])
def test_restatement_is_the_c_statement_and_within_one_ulp_of_float64(shape):
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(shape) * 3).astype(F32)
    mean, var, wt, bs = _params(shape[1], rng)
    for use_bn, use_w, use_b in itertools.product((False, True), repeat=3):
        kw = dict(mean=mean if use_bn else None, var=var if use_bn else None, weight=wt if use_w else None, bias=bs if use_b else None)
        for act, slope in ((R.ACT_NONE, 0.0), (R.ACT_RELU, 0.0), (R.ACT_LEAKY, 0.2), (R.ACT_LEAKY, 0.0)):
            got = R.bn_act_into(x, eps=1e-5, act=act, slope=slope, **kw)
            assert got.dtype == F32
            if act != R.ACT_LEAKY:          # oracle/chain.c states the fma and the ReLU in C: the same bits
                c_stmt = OC.bn_act_exact(x[..., None], eps=1e-5, relu=act == R.ACT_RELU, add_zero=False, **kw)[..., 0]
                np.testing.assert_array_equal(got.view(np.uint32), c_stmt.view(np.uint32))
            else:                           # one more multiplication on the non-positive values of the act = 0 result
                y = R.bn_act_into(x, eps=1e-5, act=R.ACT_NONE, **kw)
                np.testing.assert_array_equal(got, np.where(y > 0, y, y * F32(slope)))
            # float64.  One ulp of the result wherever no shift cancels the product (asserted for the combinations without mean
            # and bias); elsewhere the rounding analysis of tests/test_trunk_exact_host.py, u = 2^-24: `scale` carries 3.5 u, x - mean
            # adds u, the fma half an ulp of y:  |y - y64| <= ulp(y) + 6 u (|x - mean| |scale| + |bias|).  LeakyReLU multiplies the
            # error of a non-positive y by the slope and rounds once more.
            want = R.bn_act_into_f64(x, eps=1e-5, act=act, slope=slope, **kw)
            plain = R.bn_act_into_f64(x, eps=1e-5, act=R.ACT_NONE, **kw)
            per = lambda v: v.astype(np.float64)[None, :, None]
            scale = (1.0 / np.sqrt(per(var) + 1e-5) if use_bn else 1.0) * (per(wt) if use_w else 1.0)
            terms = np.abs((x - (per(mean) if use_bn else 0.0)) * scale) + (np.abs(per(bs)) if use_b else 0.0)
            ulp = lambda v: np.spacing(np.maximum(np.abs(v), np.finfo(F32).tiny).astype(F32)).astype(np.float64)
            factor = np.where(plain > 0, 1.0, slope) if act == R.ACT_LEAKY else 1.0
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= ulp(want) + factor * (ulp(plain) + 6 * 2.0 ** -24 * terms)).all(), (use_bn, use_w, use_b, act, slope)
            if not (use_bn or use_b):           # (the slope's product rounds a second time: the first half ulp, of y, is up to one of y * slope)
                assert (err <= ulp(want) * (2.0 if act == R.ACT_LEAKY else 1.0)).all(), (use_w, act, slope)


def test_fma32_rounds_once():
    """a * b = 1 + 2^-11 + 2^-24 lies exactly half way between two float32; a sliver c decides.  Rounding the float64 sum to float32
    (two roundings) would lose the sliver and go to even, 1 + 2^-11, both times."""
    a = b = np.array([1 + 2.0 ** -12], dtype=F32)
    c = np.array([2.0 ** -60], dtype=F32)
    assert R.fma32(a, b, c)[0] == F32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert R.fma32(a, b, -c)[0] == F32(1 + 2.0 ** -11)
    assert R.fma32(-a, b, -c)[0] == -F32(1 + 2.0 ** -11 + 2.0 ** -23)
    # against C's fmaf (oracle/chain.c: with a weight and a bias only, the statement is fmaf(x, weight, bias)) on values built to
    # land on and around ties: products of short mantissas plus tiny shifts
    rng = np.random.default_rng(1)
    x = (1 + rng.integers(0, 1 << 12, (1, 64, 256)) * 2.0 ** -12).astype(F32)
    wt = (1 + rng.integers(0, 1 << 12, 64) * 2.0 ** -12).astype(F32)
    bs = (rng.choice([-1.0, 1.0], 64) * 2.0 ** rng.integers(-70, -20, 64)).astype(F32)
    want = OC.bn_act_exact(x[..., None], weight=wt, bias=bs, eps=0.0, relu=False, add_zero=False)[..., 0]
    np.testing.assert_array_equal(R.fma32(x, wt[None, :, None], bs[None, :, None]), want)
    assert (R.fma32(x, wt[None, :, None], bs[None, :, None]) != (x.astype(np.float64) * wt[None, :, None] + bs[None, :, None]).astype(F32)).any()


def test_restatement_special_values():
    x = np.array([[[-0.0, 0.0, np.inf, -np.inf, np.nan, -1.0, 2.0]]], dtype=F32)
    # (without statistics y = fmaf(x - 0, 1, +0): IEEE gives -0 + +0 = +0, so an INPUT -0 leaves as +0; see below for a -0 result)
    for act, slope, want in ((R.ACT_NONE, 0.0, [0.0, 0.0, np.inf, -np.inf, np.nan, -1.0, 2.0]),
                             (R.ACT_RELU, 0.0, [0.0, 0.0, np.inf, 0.0, np.nan, 0.0, 2.0]),
                             (R.ACT_LEAKY, 0.2, [0.0, 0.0, np.inf, -np.inf, np.nan, F32(-1.0) * F32(0.2), 2.0]),
                             (R.ACT_LEAKY, 0.0, [0.0, 0.0, np.inf, np.nan, np.nan, -0.0, 2.0])):
        got = R.bn_act_into(x, act=act, slope=slope)
        want = np.array(want, dtype=F32).reshape(1, 1, -1)
        np.testing.assert_array_equal(got, want)                 # NaN where a NaN is due (its sign and payload are the platform's)
        np.testing.assert_array_equal(np.signbit(got)[~np.isnan(want)], np.signbit(want)[~np.isnan(want)])
    # a -0 OUT OF THE FMA stays: a negative product that underflows, or -0 * 1 + -0 -- mdx_bn_act's "+ 0" would lose the sign
    for act, slope in ((R.ACT_NONE, 0.0), (R.ACT_RELU, 0.0), (R.ACT_LEAKY, 0.2), (R.ACT_LEAKY, 0.0)):
        y = R.bn_act_into(np.full((1, 1, 1), -1e-30, F32), weight=np.array([1e-30], F32), act=act, slope=slope)
        assert y[0, 0, 0] == 0 and np.signbit(y[0, 0, 0]), (act, slope)
        y = R.bn_act_into(np.full((1, 1, 1), -0.0, F32), bias=np.array([-0.0], F32), act=act, slope=slope)
        assert y[0, 0, 0] == 0 and np.signbit(y[0, 0, 0]), (act, slope)
    # inf - inf is NaN
    assert np.isnan(R.bn_act_into(np.full((1, 1, 1), np.inf, F32), mean=np.array([np.inf], F32), var=np.ones(1, F32), act=R.ACT_RELU)).all()


# ------------------------------------------------------------------------------------------------------------- e. census

def _declared():
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_unet.h"$', text, flags=re.M) and "U-Net epilogue" in text
    assert text.index('#include "mdx_knn_reverse.h"') < text.index('#include "mdx_unet.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_unet.h")).read(), flags=re.S)


def test_every_unet_entry_point_is_covered():
    """Every prototype of include/mdx_unet.h is exported and bound (apart from mdx.h's own), none is a size function, and each
    has at least two memory-contract cases, one of them the stale pre-fill of the others."""
    from mdir_amd import _lib
    from test_gpu_unet_memcontract import CASES, COVERED
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", _declared()))
    assert declared == set(_lib.UNET_EXPORTS) == set(NEW)
    for other in ("EXPORTS", "KNN_JOIN_EXPORTS", "TRUNK_F16_EXPORTS", "KNN_REVERSE_EXPORTS"):
        assert not declared & set(getattr(_lib, other)), other
    assert not {n for n in declared if "_workspace" in n}
    assert {"mdx_" + entry for entry in COVERED} == declared
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry
    mdx_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    assert not re.search(r"\bmdx_bn_act_into\s*\(", mdx_h)
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bmdx_unet\.hip\b", makefile, flags=re.M) and "include/mdx_unet.h" in makefile
    assert '"mdx_unet.h"' in open(os.path.join(ROOT, "mdir_amd", "_lib.py")).read()


def test_library_exports_binds_and_refuses_before_any_device_work():
    from mdir_amd import _lib
    _lib.build()
    h = _lib.lib()
    fn = h.mdx_bn_act_into
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert h.mdx_abi_version() == _lib.ABI_VERSION == 3
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    err = lambda: h.mdx_last_error()
    assert fn(None, q, 1, 1, 8, 8, None, None, None, None, 0.0, 1, 0.0, None) == -1 and b"mdx_bn_act_into: NULL" in err()
    assert fn(p, None, 1, 1, 8, 8, None, None, None, None, 0.0, 1, 0.0, None) == -1 and b"NULL" in err()
    assert fn(p, q, 1, 1, 8, 8, p, None, None, None, 0.0, 1, 0.0, None) == -1 and b"mean and var" in err()
    assert fn(p, q, 0, 1, 8, 8, None, None, None, None, 0.0, 1, 0.0, None) == -1 and b"positive" in err()
    assert fn(p, q, 1, 1, 1 << 31, 1 << 31, None, None, None, None, 0.0, 1, 0.0, None) == -1 and b"too large" in err()
    assert fn(p, q, 1, 1, 8, 8, None, None, None, None, -1.0, 1, 0.0, None) == -1 and b"eps" in err()
    assert fn(p, q, 1, 1, 8, 8, None, None, None, None, 0.0, 3, 0.0, None) == -1 and b"act=3" in err()
    assert fn(p, q, 1, 1, 8, 8, None, None, None, None, 0.0, 2, float("inf"), None) == -1 and b"slope" in err()
    assert fn(p, q, 2, 3, 8, 23, None, None, None, None, 0.0, 1, 0.0, None) == -1 and b"out_batch_stride" in err()
    assert fn(p, q, 1 << 40, 1, 8, 1 << 30, None, None, None, None, 0.0, 1, 0.0, None) == -1 and b"too large" in err()
    # overlap: out one plane into x; x inside the span of a strided out; out == x with a wider stride
    assert fn(p, ctypes.c_void_p(4096 + 32), 1, 3, 8, 24, None, None, None, None, 0.0, 1, 0.0, None) == -1 and b"overlap" in err()
    assert fn(ctypes.c_void_p(4096 + 4 * 48), p, 2, 3, 8, 48, None, None, None, None, 0.0, 1, 0.0, None) == -1 and b"overlap" in err()
    assert fn(p, p, 2, 3, 8, 48, None, None, None, None, 0.0, 1, 0.0, None) == -1 and b"overlap" in err()


def test_wrapper_checks_need_no_gpu():
    from mdir_amd import ops
    x = torch.zeros((1, 2, 3, 4))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.bn_act_into(x, x)
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY) == (R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY) == (0, 1, 2)
    # CPU tensors take the module route whatever the switch says
    from mdir_amd.network import initialize_model
    net = initialize_model({"architecture": "shallow_p2p_unet", "in_channels": 3, "out_channels": 3, "nested_levels": 1}).eval()
    assert not net.fused(torch.zeros(1, 3, 8, 8))
