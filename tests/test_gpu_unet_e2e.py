"""The U-Net generators on the device (mdir_amd/unet.py) and a SequentialNetwork end to end (mdir_amd/network.py):

  a. every label at its golden configuration and at batch 2: the fused route (library convolutions + mdx_bn_act_into, no torch.cat)
     equals the module route (MDIR_AMD_FUSED_UNET=0) within 2e-5 * max|plain|, both equal the reference's output of
     tests/golden/g21_unet.npz within the same bound, and a NaN pixel makes NaN exactly where the module route has it;
  b. a tiny SequentialNetwork checkpoint (orig_unet + alexnet) through load_network and extract_vectors on JPEG files of two sizes,
     with the three-scale wrapper and a whitening: equal to the hand composition; graph replay equal to eager, bit for bit; and the
     scenario overlay through eval.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import unet_restatement as R
from conftest import ROOT
from test_unet_host import build, make_checkpoint, whitening

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
LABELS = sorted(R.CASES)


def both_routes(net, x, monkeypatch):
    with torch.no_grad():
        monkeypatch.setenv("MDIR_AMD_FUSED_UNET", "1")
        fused = net(x.clone())
        monkeypatch.setenv("MDIR_AMD_FUSED_UNET", "0")
        plain = net(x.clone())
        monkeypatch.delenv("MDIR_AMD_FUSED_UNET")
    return fused.cpu().numpy(), plain.cpu().numpy()


# ------------------------------------------------------------------------------------------------ a. fused against module route

@pytest.mark.parametrize("label", LABELS)
def test_fused_route_equals_module_route_and_the_reference(label, golden, monkeypatch):
    from mdir_amd import ops, unet
    g = golden("g21_unet.npz")
    calls = []
    real = ops.bn_act_into
    monkeypatch.setattr(ops, "bn_act_into", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(torch, "cat", lambda *a, **k: (calls.append("cat"), torch.concat(*a, **k))[1])
    for k, (params, _) in enumerate(R.CASES[label]):
        net = R.fill(build(label, params)).eval().to(DEV)
        x = g[R.case_key(label, k) + "_x"]
        want = g[R.case_key(label, k) + "_y"]
        for batch in (1, 2):
            xb = x if batch == 1 else np.concatenate([x, R.case_input(label, k)[:, :, ::-1, :].copy() * F32(0.5)], axis=0)
            xd = torch.from_numpy(xb).to(DEV)
            del calls[:]
            monkeypatch.setenv("MDIR_AMD_FUSED_UNET", "1")
            with torch.no_grad():
                fused = net(xd.clone()).cpu().numpy()
                assert label == "identity" or (isinstance(net, unet.UNet) and net.fused(xd))
            if label != "identity":
                # one epilogue per activation (the classic layout: one more per transposed convolution) and no concatenation
                acts = sum(isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU)) for m in net.modules())
                ups = sum(isinstance(m, torch.nn.ConvTranspose2d) for m in net.modules()) if label == "orig_unet" else 0
                assert "cat" not in calls and len(calls) == acts + ups, (label, len(calls), acts, ups)
            del calls[:]
            monkeypatch.setenv("MDIR_AMD_FUSED_UNET", "0")
            with torch.no_grad():
                plain = net(xd.clone()).cpu().numpy()
            assert 1 not in calls and (label == "identity" or "cat" in calls)
            bound = 2e-5 * np.abs(plain).max()
            err = float(np.abs(fused - plain).max())
            print("%s case %d batch %d: max |fused - plain| = %.3g, bound %.3g" % (label, k, batch, err, bound))
            assert fused.shape == plain.shape and err <= bound
            assert np.abs(plain[:1] - want).max() <= 2e-5 * np.abs(want).max() and np.abs(fused[:1] - want).max() <= 2e-5 * np.abs(want).max()


@pytest.mark.parametrize("label", [x for x in LABELS if x != "identity"])
def test_a_nan_pixel_spreads_as_in_the_module_route(label, monkeypatch):
    params, shape = R.CASES[label][-1]
    net = R.fill(build(label, params)).eval().to(DEV)
    x = np.concatenate([R.case_input(label, len(R.CASES[label]) - 1)] * 2, axis=0)
    x[1, 1, 5, 7] = np.nan
    fused, plain = both_routes(net, torch.from_numpy(x).to(DEV), monkeypatch)
    assert np.isnan(plain[1]).any() and not np.isnan(plain[0]).any()
    np.testing.assert_array_equal(np.isnan(fused), np.isnan(plain))
    ok = ~np.isnan(plain)
    assert np.abs(fused[ok] - plain[ok]).max() <= 2e-5 * np.abs(plain[ok]).max()


def test_training_and_autograd_take_the_module_route(monkeypatch):
    from mdir_amd import ops
    net = R.fill(build("outconv_unet", {"nested_levels": 2, "batchnorm": True})).to(DEV)
    monkeypatch.setattr(ops, "bn_act_into", lambda *a, **k: pytest.fail("the fused route ran"))
    x = torch.from_numpy(R.case_input("outconv_unet", 0)).to(DEV)
    net.eval()
    assert net(x).requires_grad                                   # autograd on
    net.train()
    with torch.no_grad():
        assert not net.fused(x) and net(x).shape == x.shape       # BatchNorm in training mode
        net.eval()
        assert net.fused(x)
        next(m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)).train()
        assert not net.fused(x) and net(x).shape == x.shape       # ... one submodule on its own is enough


# ------------------------------------------------------------------------------------------------------------ b. end to end

SIZES = ((136, 80), (136, 120))             # (w, h): every level of the three-scale pyramid is a multiple of 4 (two poolings)
WRAPPERS = lambda pkl: {"0_cirwhiten": {"whitening": pkl, "dimensions": None}, "1_cirmultiscale": {"scales": True}}


def _jpegs(folder, sizes, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    names = []
    for i, (w, h) in enumerate(sizes):
        pic = np.clip(np.kron(rng.integers(0, 255, (h // 8, w // 8, 3)), np.ones((8, 8, 1))) + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
        names.append(os.path.join(str(folder), "im%d.jpg" % i))
        Image.fromarray(pic).save(names[-1], quality=90)
    return names


def _load(tmp_path):
    from mdir_amd.network import load_network
    path, pkl = str(tmp_path / "seq.pth"), str(tmp_path / "whiten.pkl")
    make_checkpoint(path)
    whitening(pkl, 256)
    runtime = {"wrappers": {"train": "", "eval": WRAPPERS(pkl)}}
    return load_network({"path": path, "runtime": runtime}, torch.device(DEV)).eval(), pkl


def test_sequential_extraction_equals_the_hand_composition(tmp_path, monkeypatch):
    from PIL import Image
    from mdir_amd.datasets import initialize_transforms
    from mdir_amd.networks import extract_vectors
    from mdir_amd.wrapper import initialize_wrappers
    monkeypatch.setenv("MDIR_AMD_WORKERS", "2")
    # one image per network pass, as the hand composition runs them: the same kernels on the same shapes, so the same bits
    monkeypatch.setenv("MDIR_AMD_BATCH", "1")
    net, pkl = _load(tmp_path)
    names = _jpegs(tmp_path, (SIZES[0], SIZES[1], SIZES[0], SIZES[1], SIZES[0]), 8)
    mean_std = [net["cirnet"].model.meta["mean"], net["cirnet"].model.meta["std"]]
    tr = initialize_transforms("pil2np | totensor | normalize", mean_std)
    unet, cir = net["unet"].model, net["cirnet"].model
    assert next(unet.parameters()).is_cuda and next(cir.parameters()).is_cuda and net.supports_batches
    with torch.no_grad():
        got = extract_vectors(net, names, 256, tr, device=torch.device(DEV)).numpy()       # [D, N]
        chain = initialize_wrappers(WRAPPERS(pkl), DEV)
        for i, path in enumerate(names):
            x = tr(Image.open(path).convert("RGB"))[None].to(DEV)
            want = chain(x, lambda t: cir(unet(t)), cir).cpu().numpy().reshape(-1)
            print("image %d: max |extract_vectors - hand composition| = %.3g" % (i, float(np.abs(got[:, i] - want).max())))
            np.testing.assert_array_equal(got[:, i], want)
            assert np.abs(got[:, i] - chain(x, cir).cpu().numpy().reshape(-1)).max() > 1e-2          # the U-Net is in the path
    assert got.shape == (256, 5) and np.isfinite(got).all()


def test_graph_replay_of_the_sequence_equals_eager(tmp_path, monkeypatch):
    from mdir_amd.datasets import initialize_transforms
    from mdir_amd.graphs import ShapeGraphs
    from mdir_amd.networks import extract_vectors_device
    net, _ = _load(tmp_path)
    names = _jpegs(tmp_path, (SIZES[0],) * 6, 4)
    tr = initialize_transforms("pil2np | totensor | normalize", [net["cirnet"].model.meta["mean"], net["cirnet"].model.meta["std"]])
    made = []
    orig = ShapeGraphs.__init__

    def spy(self, *a, **k):
        orig(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(ShapeGraphs, "__init__", spy)
    monkeypatch.setattr(ShapeGraphs, "PAYOFF_IMAGES", 0)
    monkeypatch.setenv("MDIR_AMD_WORKERS", "0")
    monkeypatch.setenv("MDIR_AMD_BATCH", "1")
    graphed = extract_vectors_device(net, names, 256, tr, device=DEV).cpu().numpy()
    assert len(made) == 1 and made[0].replays == 5 and len(made[0].graphs) == 1 and not made[0].refused
    monkeypatch.setenv("MDIR_AMD_GRAPHS", "0")
    eager = extract_vectors_device(net, names, 256, tr, device=DEV).cpu().numpy()
    assert len(made) == 1
    assert np.isfinite(eager).all() and len(np.unique(eager.round(4), axis=0)) == 6
    assert graphed.tobytes() == eager.tobytes()


def test_composition_scenario_runs_through_eval_py(tmp_path):
    """scenarios/eval_composition.yml names the reference's remote files; here its keys are filled with a generated checkpoint and
    whitening and run as test_eval_py_end_to_end does.  The overlay parses, and eval.py prints a score per test set."""
    with open(os.path.join(ROOT, "scenarios", "eval_composition.yml")) as f:
        scenario = yaml.safe_load(f)
    assert scenario["network"].keys() == {"path", "runtime"} and scenario["network"]["path"].endswith(".pth")
    assert scenario["network"]["runtime"]["wrappers"]["eval"]["0_cirwhiten"]["whitening"].endswith(".pkl")
    root = str(tmp_path / "synth")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_eval.py"), root, "alexnet", "6"])
    make_checkpoint(os.path.join(root, "seq.pth"), {"architecture": "outconv_dynint_unet", "in_channels": 3, "out_channels": 3,
                                                     "nested_levels": 2, "outconv_channels": 8})
    scenario["network"]["path"] = os.path.join(root, "seq.pth")
    scenario["network"]["runtime"]["wrappers"]["eval"]["0_cirwhiten"]["whitening"] = os.path.join(root, "whiten.pkl")
    scenario["validation"] = {"roxford5k": {"criterion": {"image_size": 160}}, "247tokyo1k": {"criterion": {"image_size": 160}},
                              "rparis6k*": False}
    overlay = os.path.join(root, "eval_composition_synth.yml")
    with open(overlay, "w") as f:
        yaml.safe_dump(scenario, f)
    env = dict(os.environ, CIRTORCH_ROOT=root, MDIR_AMD_WORKERS="2")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "eval.yml", overlay], env=env, text=True,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert proc.returncode == 0, proc.stdout[-3000:]
    printed = {}
    for line in proc.stdout.splitlines():
        for label in ("roxford.5k medium", "247tokyo.1k"):
            if line.strip().startswith(label):
                printed[label] = float(line.split()[-1])
    assert set(printed) == {"roxford.5k medium", "247tokyo.1k"} and all(0 < v <= 100 for v in printed.values()), proc.stdout[-3000:]
