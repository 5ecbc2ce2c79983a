"""mdx_histmatch_u8_to_chw and mdx_gamma_u8_to_chw (include/mdx_photometric.h) on the MI355X against the reference's numpy / scipy
arithmetic (tests/photometric_restatement.py).  The Lab conversion is the CLAHE kernels' and carries their bound: the device's
float32 lightness may differ from numpy's in the last bits of powf / cbrtf.  GIVEN the device's own lightness plane everything up to
the mapped lightness is compared bit for bit (counts, the table fp, np.interp), gamma against a float64 bracketing root at the
reference solver's own tolerance, and the output against the rest of the chain at the Lab -> RGB code's 1e-4
(test_gpu_round3.test_clahe_kernels_vs_restatement).  The difference to a pure-numpy end-to-end run is printed, not asserted: `eq` has
slopes up to 255, which amplify the last bits of the lightness (profiles/r18_photometric.md records the maxima)."""
import functools

import numpy as np
import pytest
import torch

import photometric_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32

# (B, H, W) and the per-image `dark` factors
SHAPES = {"1x1x1": ((1, 1, 1), None), "1x9x7": ((1, 9, 7), None), "2x37x53 scalar": ((2, 37, 53), None), "1x64x96 vector": ((1, 64, 96), None),
          "3x60x96 dark": ((3, 60, 96), (1.0, 0.3, 0.05)), "1x240x320": ((1, 240, 320), None), "1x768x1024": ((1, 768, 1024), None),
          "constant 0 255 128": ((3, 12, 20), "constant")}


@functools.lru_cache(maxsize=None)
def case(name):
    """(uint8 images [B,H,W,3], their normalised Lab spaces in numpy): made once, shared by every test, never written to."""
    (b, h, w), dark = SHAPES[name]
    if dark == "constant":
        img = np.stack([np.full((h, w, 3), v, np.uint8) for v in (0, 255, 128)])
    else:
        img = R.images(b, h, w, dark)
    spaces = [R.normspace(im) for im in img]
    img.setflags(write=False)
    for s in spaces:
        s.setflags(write=False)
    return img, spaces


@functools.lru_cache(maxsize=None)
def target_cdf():
    cdf = np.cumsum(R.target_histogram())
    assert (np.diff(cdf) == 0).sum() >= 10 and cdf[4] == 0          # tied entries at both ends
    return cdf


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                # a copy: the shared cases are read-only


def bins_of(x):
    """np.histogram's bin of every value (the last bin closed on the right)."""
    return np.minimum(np.searchsorted(R.EDGES, x.astype(np.float64), side="right") - 1, 255)


def check_lightness(x_dev, x_np):
    """The device's float32 lightness against numpy's: four last-place units of [0.5, 1), and the bins they fall into."""
    assert np.abs(x_dev.astype(np.float64) - x_np.astype(np.float64)).max() <= 1e-6
    diff = bins_of(x_dev) - bins_of(x_np)
    assert np.abs(diff).max() <= 1 and (diff != 0).mean() < 1e-3


@pytest.mark.parametrize("form", ["eq", "named"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_histogram_matching_vs_numpy(name, form):
    from mdir_amd import ops
    img, spaces = case(name)
    cdf = None if form == "eq" else target_cdf()
    out, x, counts, fp, mapped = ops.histmatch_u8_to_chw(dev(img), R.MEAN, R.STD, None if cdf is None else dev(cdf), return_intermediates=True)
    out, x, counts, fp, mapped = out.cpu().numpy(), x.cpu().numpy(), counts.cpu().numpy(), fp.cpu().numpy(), mapped.cpu().numpy()
    assert x.dtype == F32 and counts.dtype == np.int32 and fp.dtype == np.float64 and mapped.dtype == F32
    assert np.isfinite(out).all()
    for i, spc in enumerate(spaces):
        check_lightness(x[i], spc[..., 0])
        np.testing.assert_array_equal(counts[i], np.histogram(x[i], R.EDGES)[0])
        want_fp = R.fp_table(counts[i], x[i].size, cdf)
        assert fp[i].tobytes() == want_fp.tobytes(), np.flatnonzero(fp[i] != want_fp)[:8]
        want_mapped = np.interp(x[i], R.CENTRES, fp[i]).astype(F32)
        assert mapped[i].tobytes() == want_mapped.tobytes(), int((mapped[i] != want_mapped).sum())
        np.testing.assert_allclose(out[i], R.finish(spc, mapped[i]), rtol=0, atol=1e-4)
        end_to_end = np.abs(out[i] - R.finish(spc, R.match(spc[..., 0], cdf)[2])).max()
        print("histmatch %s %s image %d: max |device - numpy end to end| = %.3g (max slope %.3g)"
              % (form, name, i, end_to_end, np.abs(np.diff(fp[i])).max() * 255))


def clipped_root(x, target):
    root = R.gamma_root(x, target)
    return None if root is None else float(np.clip(root, 0.1, 10))


@pytest.mark.parametrize("target", [0.3, 0.5, 0.7])
@pytest.mark.parametrize("name", list(SHAPES))
def test_gamma_equalisation_vs_scipy(name, target):
    from mdir_amd import ops
    img, spaces = case(name)
    out, x, gamma = ops.gamma_u8_to_chw(dev(img), target, R.MEAN, R.STD, return_intermediates=True)
    out, x, gamma = out.cpu().numpy(), x.cpu().numpy(), gamma.cpu().numpy()
    assert gamma.dtype == np.float64 and gamma.shape == (len(img),)
    assert np.isfinite(out).all() and np.isfinite(gamma).all() and (gamma >= 0.1).all() and (gamma <= 10).all()
    for i, spc in enumerate(spaces):
        check_lightness(x[i], spc[..., 0])
        want = clipped_root(x[i], target)                 # None: a plane of zeros or of ones, whose mean no gamma moves
        if want is not None:
            print("gamma %s target %g image %d: gamma %.9g, bracketing root %.9g" % (name, target, i, gamma[i], want))
            assert abs(gamma[i] - want) <= 1e-4
        else:
            assert SHAPES[name][1] == "constant" and i < 2
        np.testing.assert_allclose(out[i], R.finish(spc, R.gamma_map(x[i], gamma[i])), rtol=0, atol=1e-4)
        if SHAPES[name][1] == "constant" and i < 2:       # black and white come back as the plain conversion's Lab round trip
            np.testing.assert_allclose(out[i], R.finish(spc, spc[..., 0]), rtol=0, atol=1e-4)
        want_np = clipped_root(spc[..., 0], target)
        if want_np is not None:
            print("gamma %s target %g image %d: max |device - numpy end to end| = %.3g"
                  % (name, target, i, np.abs(out[i] - R.finish(spc, R.gamma_map(spc[..., 0], want_np))).max()))


@pytest.mark.parametrize("dark,plus,target,gamma,fallback", [(0.05, 0, 0.7, 0.1, 0), (1.0, 0, 0.02, 10.0, 0), (1.0, 150, 0.05, 10.0, 1)],
                         ids=["secant 0.082 clipped to 0.1", "secant 16.9 clipped to 10", "no convergence, fallback 10"])
def test_gamma_clip_and_fallback_rows(dark, plus, target, gamma, fallback):
    """The three rows checked on the CPU against the reference's own arithmetic (scipy.optimize.newton on the same plane)."""
    from mdir_amd import ops
    img = R.images(1, 64, 96, [dark], seed=5, plus=plus)
    out, x, g, info = ops.gamma_u8_to_chw(dev(img), target, R.MEAN, R.STD, return_intermediates="solver")
    print("gamma row dark %g plus %d target %g: gamma %r, secant steps %d, fallback %d" % (dark, plus, target, float(g[0]), int(info[0, 0]), int(info[0, 1])))
    assert float(g[0]) == gamma and int(info[0, 1]) == fallback and 1 <= int(info[0, 0]) <= 50
    spc = R.normspace(img[0])
    np.testing.assert_allclose(out[0].cpu().numpy(), R.finish(spc, R.gamma_map(x[0].cpu().numpy(), gamma)), rtol=0, atol=1e-4)


@pytest.mark.parametrize("name", ["2x37x53 scalar", "3x60x96 dark"])
def test_the_same_call_twice_gives_the_same_bits(name):
    from mdir_amd import ops
    u8 = dev(case(name)[0])
    cdf = dev(target_cdf())
    for call in (lambda: ops.histmatch_u8_to_chw(u8, R.MEAN, R.STD), lambda: ops.histmatch_u8_to_chw(u8, R.MEAN, R.STD, cdf),
                 lambda: ops.gamma_u8_to_chw(u8, 0.5, R.MEAN, R.STD)):
        first = call().cpu().numpy()
        scratch = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=DEV)         # whatever the allocator hands out next is dirty
        del scratch
        assert call().cpu().numpy().tobytes() == first.tobytes()


# ---------------------------------------------------------------- through the transform DSL and the extraction loop

CHAINS = {"match_histogram:eq": lambda ops, u8, mean, std: ops.histmatch_u8_to_chw(u8, mean, std),
          "gamma_equalize:0.5": lambda ops, u8, mean, std: ops.gamma_u8_to_chw(u8, 0.5, mean, std)}


def _jpegs(tmp_path, sizes, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    names = []
    for i, (w, h) in enumerate(sizes):
        pic = np.clip(np.kron(rng.integers(0, 255, (h // 16, w // 16, 3)), np.ones((16, 16, 1))) + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
        names.append(str(tmp_path / ("im%d.jpg" % i)))
        Image.fromarray(pic).save(names[-1], quality=90)
    return names


@pytest.mark.parametrize("middle", list(CHAINS))
def test_extraction_through_the_photometric_chains(tmp_path, monkeypatch, middle):
    """extract_vectors with `pil2np | <transform> | totensor | normalize`: file -> JPEG decode -> thumbnail -> the fused conversion
    (all on the device) -> network; equal to the same network fed the operator's tensor of the PIL thumbnail, one image at a time."""
    from PIL import Image
    from mdir_amd import ops
    from mdir_amd.datasets import initialize_transforms
    from mdir_amd.networks import extract_vectors, init_network
    monkeypatch.setenv("MDIR_AMD_WORKERS", "2")
    names = _jpegs(tmp_path, ((320, 240), (240, 320), (320, 240)), 8)
    torch.manual_seed(3)
    net = init_network({"architecture": "alexnet", "pooling": "gem", "whitening": False, "pretrained": False}).eval().to(DEV)
    tr = initialize_transforms("pil2np | %s | totensor | normalize" % middle, [net.meta["mean"], net.meta["std"]])
    assert tr.device_tail()[2]["op"] == middle.split(":")[0]
    with torch.no_grad():
        got = extract_vectors(net, names, 256, tr, device=torch.device(DEV)).numpy()       # [D, N]
        for i, path in enumerate(names):
            img = Image.open(path).convert("RGB")
            img.thumbnail((256, 256), Image.LANCZOS)
            x = CHAINS[middle](ops, dev(np.array(img)[None]), net.meta["mean"], net.meta["std"])
            np.testing.assert_allclose(got[:, i], net(x).cpu().numpy().reshape(-1), atol=2e-4)


@pytest.mark.parametrize("middle", list(CHAINS))
def test_graph_replay_of_the_photometric_chains_equals_eager(tmp_path, monkeypatch, middle):
    """Six images of one shape, one at a time: the conversion runs inside the hipGraph of the shape's `describe` closure from the
    second image on (memset node and kernels captured, nothing else): the descriptors are those of the eager run, bit for bit."""
    from mdir_amd.datasets import initialize_transforms
    from mdir_amd.graphs import ShapeGraphs
    from mdir_amd.networks import extract_vectors_device, init_network
    names = _jpegs(tmp_path, ((160, 128),) * 6, 4)
    torch.manual_seed(1)
    net = init_network({"architecture": "alexnet", "pooling": "gem", "whitening": False, "pretrained": False}).eval().to(DEV)
    tr = initialize_transforms("pil2np | %s | totensor | normalize" % middle, [net.meta["mean"], net.meta["std"]])
    made = []
    orig = ShapeGraphs.__init__

    def spy(self, *a, **k):
        orig(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(ShapeGraphs, "__init__", spy)
    monkeypatch.setattr(ShapeGraphs, "PAYOFF_IMAGES", 0)
    monkeypatch.setenv("MDIR_AMD_WORKERS", "0")
    monkeypatch.setenv("MDIR_AMD_BATCH", "1")
    graphed = extract_vectors_device(net, names, 160, tr, device=DEV).cpu().numpy()
    assert len(made) == 1 and made[0].replays == 5 and len(made[0].graphs) == 1 and not made[0].refused
    monkeypatch.setenv("MDIR_AMD_GRAPHS", "0")
    eager = extract_vectors_device(net, names, 160, tr, device=DEV).cpu().numpy()
    assert len(made) == 1
    assert np.isfinite(eager).all() and len(np.unique(eager.round(4), axis=0)) == 6
    assert graphed.tobytes() == eager.tobytes()
