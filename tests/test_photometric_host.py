"""Histogram matching and gamma equalisation (include/mdx_photometric.h; mdir_amd/datasets.py MatchHistogram / GammaEqualize) on a
CPU-only box: the census of include/mdx_photometric.h, the workspace formula, the bin edges and centres against numpy bit for bit,
every refusal of the C ABI with nothing launched, the transform DSL with its registry of named targets, the dispatch of
``device_convert`` (a numpy fake standing in for the device), and the two scenario overlays."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import photometric_restatement as R
from conftest import ROOT

NEW = ("mdx_photometric_workspace", "mdx_photometric_tables", "mdx_histmatch_u8_to_chw", "mdx_gamma_u8_to_chw")


def _declared():
    """The code of include/mdx_photometric.h, which mdx.h includes for its section "photometric normalisation"."""
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_photometric.h"$', text, flags=re.M) and "photometric normalisation" in text
    assert text.index('#include "mdx_groups.h"') < text.index('#include "mdx_krecip.h"') < text.index('#include "mdx_photometric.h"')
    assert re.search(r"#define MDX_ABI_VERSION 3\b", text)
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_photometric.h")).read(), flags=re.S)


def test_census_of_the_photometric_entry_points():
    from mdir_amd import _lib
    code = _declared()
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.PHOTOMETRIC_EXPORTS) == set(NEW)
    assert not declared & (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS) | set(_lib.GROUPS_EXPORTS)
                           | set(_lib.KRECIP_EXPORTS))
    assert re.search(r"int\s+mdx_histmatch_u8_to_chw\s*\(\s*const uint8_t \*rgb,\s*int64_t B,\s*int64_t H,\s*int64_t W,\s*const double \*target_cdf,"
                     r"\s*const float \*mean,\s*const float \*std,\s*void \*workspace,\s*int64_t workspace_bytes,\s*float \*out,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+mdx_gamma_u8_to_chw\s*\(\s*const uint8_t \*rgb,\s*int64_t B,\s*int64_t H,\s*int64_t W,\s*double target,"
                     r"\s*const float \*mean,\s*const float \*std,\s*void \*workspace,\s*int64_t workspace_bytes,\s*float \*out,\s*void \*stream\s*\)", code)
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert "mdx_photometric.hip" in makefile and "include/mdx_photometric.h" in makefile
    # the Lab code is shared, not restated: one definition, in the header both sources include
    csrc = os.path.join(ROOT, "mdir_amd", "csrc")
    for name in ("srgb_to_linear", "lab_f", "rgb8_to_lab_lut", "linear_to_srgb_fast", "mul_", "div_"):
        defined = [f for f in sorted(os.listdir(csrc)) if re.search(r"__forceinline__ \w+ %s\(" % name, open(os.path.join(csrc, f)).read())]
        assert defined == ["mdx_lab.h"], (name, defined)
    for f in ("mdx_clahe.hip", "mdx_photometric.hip"):
        assert '#include "mdx_lab.h"' in open(os.path.join(csrc, f)).read()
    assert "#pragma clang fp contract(off)" in open(os.path.join(csrc, "mdx_lab.h")).read()
    _lib.build()
    h = _lib.lib()
    for name in NEW:
        assert hasattr(h, name) and getattr(h, name).argtypes is not None
    assert h.mdx_abi_version() == 3 == _lib.ABI_VERSION


def test_workspace_formula():
    from mdir_amd import _lib
    h = _lib.lib()
    up = lambda n: -(-n // 256) * 256
    for b, hh, w in ((1, 1, 1), (2, 10, 10), (1, 9, 7), (3, 60, 96), (8, 768, 1024), (33, 5, 5), (65535, 1, 1), (1, 32768, 65535)):
        assert h.mdx_photometric_workspace(b, hh, w) == 4 * up(4 * b * hh * w) + 1024 * b + 2048 * b + 2 * up(8 * b), (b, hh, w)
    assert h.mdx_photometric_workspace(2, 10, 10) == 4 * 1024 + 2048 + 4096 + 512
    for b, hh, w in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, -2), (65536, 4, 4), (1, 1 << 24, 1), (1, 1, 1 << 24), (1, 1 << 16, 1 << 15)):
        assert h.mdx_photometric_workspace(b, hh, w) == 0, (b, hh, w)


def test_tables_are_numpys_linspaces_bit_for_bit():
    from mdir_amd import _lib
    h = _lib.lib()
    edges, centres = (ctypes.c_double * 257)(), (ctypes.c_double * 256)()
    assert h.mdx_photometric_tables(edges, centres) == 0
    want_e, want_c = np.linspace(-0.00196078431372549, 1.0019607843137255, 257), np.linspace(0, 1, 256)
    assert np.array(edges).tobytes() == want_e.tobytes() and np.array(centres).tobytes() == want_c.tobytes()
    assert (want_c != np.arange(256) / 255).any()         # k * (1 / 255), not k / 255: the two differ, and numpy's is the one kept
    assert h.mdx_photometric_tables(None, centres) == -1 and h.mdx_photometric_tables(edges, None) == -1
    assert h.mdx_last_error().startswith(b"mdx_photometric_tables:")


def test_refusals_before_any_device_work():
    """Every MDX_ERR_INVALID / MDX_ERR_WORKSPACE of the two conversions through the C ABI with pointers that are no memory: nothing
    is launched (there is no device here to launch on), and the error names the call."""
    from mdir_amd import _lib
    h = _lib.lib()
    p, mean = ctypes.c_void_p(4096), (ctypes.c_float * 3)(0, 0, 0)
    need = h.mdx_photometric_workspace(2, 8, 8)

    def hist(rgb=p, b=2, hh=8, w=8, cdf=None, m=mean, s=mean, ws=p, wsb=1 << 20, out=p):
        return h.mdx_histmatch_u8_to_chw(rgb, b, hh, w, cdf, m, s, ws, wsb, out, None)

    def gamma(rgb=p, b=2, hh=8, w=8, target=0.5, m=mean, s=mean, ws=p, wsb=1 << 20, out=p):
        return h.mdx_gamma_u8_to_chw(rgb, b, hh, w, target, m, s, ws, wsb, out, None)

    def refused(status, name, *words, code=-1):
        msg = h.mdx_last_error()
        assert status == code and msg.startswith(name.encode() + b":"), (status, msg)
        for w in words:
            assert w.encode() in msg, (w, msg)
    for fn, name in ((hist, "mdx_histmatch_u8_to_chw"), (gamma, "mdx_gamma_u8_to_chw")):
        for kw in ({"rgb": None}, {"out": None}, {"m": None}, {"s": None}):
            refused(fn(**kw), name, "NULL")
        for kw in ({"b": 0}, {"b": -1}, {"hh": 0}, {"w": 0}, {"b": 65536}, {"hh": 1 << 24}, {"w": 1 << 24}, {"hh": 1 << 16, "w": 1 << 15}):
            refused(fn(**kw), name, "bad sizes")
        refused(fn(ws=None), name, "workspace", code=-4)
        refused(fn(wsb=need - 1), name, "workspace", code=-4)
        refused(fn(wsb=0), name, "workspace", code=-4)
        refused(fn(ws=ctypes.c_void_p(4096 + 8)), name, "16-byte aligned")
    refused(hist(cdf=ctypes.c_void_p(4096 + 4)), "mdx_histmatch_u8_to_chw", "8-byte aligned")
    for target in (0.0, 1.0, 1.5, -0.2, float("nan"), float("inf")):
        refused(gamma(target=target), "mdx_gamma_u8_to_chw", "0 < target < 1")


# ------------------------------------------------------------------ the transform DSL

def _chain(middle, mean=R.MEAN, std=R.STD):
    from mdir_amd.datasets import initialize_transforms
    return initialize_transforms("pil2np | %s | totensor | normalize" % middle, [mean, std])


def test_dsl_parses_the_two_transforms():
    from mdir_amd.datasets import TRANSFORMS, GammaEqualize, MatchHistogram, initialize_transforms
    assert TRANSFORMS["match_histogram"] is MatchHistogram and TRANSFORMS["gamma_equalize"] is GammaEqualize
    t = _chain("match_histogram:eq").transforms[1]
    assert isinstance(t, MatchHistogram) and (t.histogram, t.colorspace, t.cdf) == ("eq", "lab", None)
    assert _chain("match_histogram:eq").device_tail() == (R.MEAN, R.STD, {"op": "match_histogram", "histogram": "eq", "cdf": None})
    assert _chain("match_histogram:eq:lab").device_tail() == _chain("match_histogram:eq").device_tail()
    g = _chain("gamma_equalize:0.3").transforms[1]
    assert isinstance(g, GammaEqualize) and (g.target, g.colorspace) == (0.3, "lab")
    assert _chain("gamma_equalize:0.3").device_tail() == (R.MEAN, R.STD, {"op": "gamma_equalize", "target": 0.3})
    assert _chain("gamma_equalize:0.5:lab").device_tail()[2] == {"op": "gamma_equalize", "target": 0.5}
    # the CLAHE dictionary keeps its two keys
    assert _chain("apply_clahe").device_tail()[2] == {"clip_limit": 4, "grid": (8, 8)}
    for bad in ("match_histogram:eq:luv", "gamma_equalize:0.5:luv"):
        with pytest.raises(NotImplementedError):
            _chain(bad)
    for bad in ("0", "1", "1.5", "-0.1", "nan"):
        with pytest.raises(ValueError, match="gamma_equalize: target"):
            _chain("gamma_equalize:" + bad)
    with pytest.raises(ValueError):
        _chain("gamma_equalize:half")                     # float() of the DSL's string
    with pytest.raises(TypeError):
        _chain("gamma_equalize")                          # the reference's transform has no default target either
    for t in (MatchHistogram("eq"), GammaEqualize(0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            t(np.zeros((4, 4, 3), np.float32))
    # an incomplete chain is not a device chain
    for text in ("pil2np | match_histogram:eq | totensor", "pil2np | gamma_equalize:0.5 | totensor", "match_histogram:eq | totensor | normalize",
                 "pil2np | gamma_equalize:0.5 | apply_clahe | totensor | normalize"):
        assert initialize_transforms(text, [R.MEAN, R.STD]).device_tail() is None, text


def test_named_targets_registry_and_npy_lookup(tmp_path, monkeypatch):
    from mdir_amd import datasets
    from mdir_amd.datasets import MatchHistogram, initialize_transforms, register_histogram
    monkeypatch.setattr(datasets, "HISTOGRAM_CDF", {})
    monkeypatch.setenv("MDIR_AMD_MODELS", str(tmp_path / "none") + ":" + str(tmp_path / "models"))
    with pytest.raises(KeyError, match="f3d_lab"):
        MatchHistogram("f3d_lab")
    with pytest.raises(KeyError):
        initialize_transforms("pil2np | match_histogram:f3d_lab", None)
    hist = R.target_histogram()
    register_histogram("mine", hist.astype(np.float32).tolist())
    want = np.cumsum(hist.astype(np.float32).astype(np.float64))
    t = MatchHistogram("mine")
    assert t.cdf.dtype == np.float64 and t.cdf.tobytes() == want.tobytes() and t.cdf[-1] > 1     # unnormalised, as the reference keeps it
    assert (np.diff(t.cdf) == 0).sum() >= 10                                                     # ties and all
    for bad in (hist[:255], np.append(hist, 1.0), -hist, np.where(np.arange(256) == 7, np.nan, hist), np.where(np.arange(256) == 7, np.inf, hist)):
        with pytest.raises(ValueError, match="256 non-negative finite values"):
            register_histogram("bad", bad)
    with pytest.raises(ValueError):
        register_histogram("eq", hist)
    assert "bad" not in datasets.HISTOGRAM_CDF
    # <name>.npy in the model directories
    os.makedirs(tmp_path / "models")
    np.save(tmp_path / "models" / "fromfile.npy", hist)
    f = MatchHistogram("fromfile")
    assert f.cdf.tobytes() == np.cumsum(hist).tobytes()
    np.save(tmp_path / "models" / "short.npy", hist[:100])
    with pytest.raises(ValueError, match="256 non-negative finite values"):
        MatchHistogram("short")
    tail = initialize_transforms("pil2np | match_histogram:fromfile | totensor | normalize", [R.MEAN, R.STD]).device_tail()
    assert tail[2]["op"] == "match_histogram" and tail[2]["histogram"] == "fromfile" and callable(tail[2]["cdf"])
    on_cpu = tail[2]["cdf"](torch.device("cpu"))
    assert on_cpu.dtype == torch.float64 and on_cpu.numpy().tobytes() == np.cumsum(hist).tobytes()
    assert tail[2]["cdf"](torch.device("cpu")) is on_cpu                                         # put there once per transform and device


def test_device_convert_dispatches_on_op(monkeypatch):
    """``device_convert`` with ``ops`` replaced by the numpy restatement: each chain reaches its operator with its parameters, the
    target CDF as ONE float64 tensor however often the conversion is called."""
    from mdir_amd import datasets, ops
    from mdir_amd.datasets import device_convert, register_histogram
    monkeypatch.setattr(datasets, "HISTOGRAM_CDF", {})
    register_histogram("mine", R.target_histogram())
    calls = []

    def fake_hist(images, mean, std, target_cdf=None, return_intermediates=False):
        calls.append(("hist", target_cdf))
        cdf = None if target_cdf is None else target_cdf.numpy()
        out = [R.finish(R.normspace(im), R.match(R.normspace(im)[..., 0], cdf)[2], mean, std) for im in images.numpy()]
        return torch.from_numpy(np.stack(out))

    def fake_gamma(images, target, mean, std, return_intermediates=False):
        calls.append(("gamma", target))
        out = []
        for im in images.numpy():
            spc = R.normspace(im)
            out.append(R.finish(spc, R.gamma_map(spc[..., 0], np.clip(R.gamma_root(spc[..., 0], target), 0.1, 10)), mean, std))
        return torch.from_numpy(np.stack(out))

    def no_clahe(*a, **k):
        raise AssertionError("the CLAHE operator was called")
    monkeypatch.setattr(ops, "histmatch_u8_to_chw", fake_hist)
    monkeypatch.setattr(ops, "gamma_u8_to_chw", fake_gamma)
    monkeypatch.setattr(ops, "clahe_u8_to_chw", no_clahe)
    monkeypatch.setattr(ops, "u8_to_chw", no_clahe)
    img = R.images(2, 24, 40, dark=[1.0, 0.3])
    u8 = torch.from_numpy(img)
    mean, std = [0.5, 0.4, 0.3], [0.25, 0.5, 1.0]
    got = device_convert(_chain("match_histogram:eq", mean, std).device_tail())(u8).numpy()
    assert calls == [("hist", None)] and got.shape == (2, 3, 24, 40)
    spc = R.normspace(img[1])
    want = R.finish(spc, np.interp(spc[..., 0], R.CENTRES, np.cumsum(np.histogram(spc[..., 0], R.EDGES)[0]) / spc[..., 0].size).astype(np.float32), mean, std)
    np.testing.assert_array_equal(got[1], want)
    convert = device_convert(_chain("match_histogram:mine", mean, std).device_tail())
    named = convert(u8).numpy()
    convert(u8)
    assert [c[0] for c in calls[1:]] == ["hist", "hist"] and calls[1][1] is calls[2][1] and calls[1][1].dtype == torch.float64
    assert calls[1][1].numpy().tobytes() == np.cumsum(R.target_histogram()).tobytes()
    assert not np.array_equal(named, got)
    del calls[:]
    gam = device_convert(_chain("gamma_equalize:0.3", mean, std).device_tail())(u8).numpy()
    assert calls == [("gamma", 0.3)]
    for i in range(2):                                    # the fake did move the mean lightness to the target
        back = R.normspace(np.clip(np.rint((gam[i].transpose(1, 2, 0) * np.float32(std) + np.float32(mean)) * 255), 0, 255).astype(np.uint8))[..., 0]
        assert abs(float(back.mean()) - 0.3) < 0.02
    with pytest.raises(KeyError, match="no device operator"):
        device_convert((mean, std, {"op": "tospace"}))


def test_overlays_load_and_merge_onto_eval_yml():
    import eval as evalcli
    from mdir_amd.datasets import initialize_transforms
    base = evalcli.load_scenarios(["eval.yml"])
    for overlay, chain, op in (("eval_histeq.yml", "pil2np | match_histogram:eq | totensor | normalize", "match_histogram"),
                               ("eval_gamma.yml", "pil2np | gamma_equalize:0.5 | totensor | normalize", "gamma_equalize")):
        import yaml
        alone = yaml.safe_load(open(os.path.join(ROOT, "scenarios", overlay)))
        assert alone == {"network": {"runtime": {"data": {"transforms": chain}}}}                 # nothing but the transform chain
        sc = evalcli.load_scenarios(["eval.yml", overlay])
        assert sc["network"]["runtime"]["data"] == {"transforms": chain}
        assert sc["network"]["runtime"]["wrappers"] == base["network"]["runtime"]["wrappers"] and sc["validation"] == base["validation"]
        assert initialize_transforms(sc["network"]["runtime"]["data"]["transforms"], [R.MEAN, R.STD]).device_tail()[2]["op"] == op
