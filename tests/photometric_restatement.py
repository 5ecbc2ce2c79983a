"""The reference's histogram matching and gamma equalisation of the Lab lightness (mdir/components/data/transform/functional.py:55-102)
restated in numpy / scipy for the tests of include/mdx_photometric.h (a helper module, imported by test_photometric_host.py,
test_gpu_photometric.py and test_gpu_photometric_memcontract.py).  The Lab halves are oracle.rgb_to_lab / oracle.lab_to_rgb, the
restatement of OpenCV the CLAHE tests use; everything between them is numpy's own np.histogram / np.cumsum / np.interp / np.power."""
import numpy as np
import scipy.optimize

from oracle import oracle as O

F32 = np.float32
EDGES = np.linspace(-0.00196078431372549, 1.0019607843137255, 257)
CENTRES = np.linspace(0, 1, 256)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
_OFFSET, _SCALE = np.array([0, 128, 128], F32), np.array([100, 255, 255], F32)


def images(b, h, w, dark=None, seed=None, plus=0):
    """The generator of test_gpu_round3.test_clahe_kernels_vs_restatement (8 x 8 blocks plus N(0, 12) noise), every image scaled
    by its ``dark`` factor (and shifted by ``plus``) before clipping."""
    rng = np.random.default_rng(h * w + b if seed is None else seed)
    base = rng.integers(0, 256, (b, h // 8 + 1, w // 8 + 1, 3))
    img = np.kron(base, np.ones((1, 8, 8, 1)))[:, :h, :w] + rng.normal(0, 12, (b, h, w, 3))
    if dark is not None:
        img = img * np.asarray(dark, np.float64).reshape(-1, 1, 1, 1)
    return np.clip(img + plus, 0, 255).astype(np.uint8)


def target_histogram(seed=11):
    """A target with ties in its CDF: random squares, the first 5 and the last 6 bins empty."""
    h = np.random.default_rng(seed).random(256) ** 2
    h[:5] = 0
    h[-6:] = 0
    return h


def normspace(img):
    """rgb2normspace(pil2np(img), "lab"): float32 [H,W,3], lightness in [0, 1] first."""
    lab = O.rgb_to_lab(img.astype(F32) / F32(255))
    return ((lab + _OFFSET) / _SCALE).astype(F32)


def finish(spc, lightness, mean=MEAN, std=STD):
    """normspace2rgb with the lightness replaced, then totensor | normalize: float32 [3,H,W]."""
    spc = spc.copy()
    spc[..., 0] = lightness
    rgb = O.lab_to_rgb(((spc * _SCALE).astype(F32) - _OFFSET).astype(F32))
    return ((rgb - F32(mean)) / F32(std)).transpose(2, 0, 1)


def fp_table(counts, size, target_cdf=None):
    """The table np.interp maps the lightness through, from the 256 bin counts of one image of ``size`` pixels."""
    cdf0 = np.cumsum(counts.astype(np.int64)) / int(size)
    if target_cdf is None:
        return cdf0 * CENTRES[-1]
    return np.interp(cdf0, target_cdf, CENTRES)


def match(x, target_cdf=None):
    """channel_histogram_matching on a float32 lightness plane: (counts, fp, mapped float32)."""
    counts = np.histogram(x, EDGES)[0]
    fp = fp_table(counts, x.size, target_cdf)
    return counts, fp, np.interp(x, CENTRES, fp).astype(F32)


def gamma_root(x, target):
    """The gamma with mean(x ** gamma) = target in float64 by bracketing (None when the mean does not move: a constant 0 / 1 plane)."""
    xd = x.astype(np.float64).reshape(-1)
    f = lambda g: float(np.mean(np.power(xd, g))) - target
    lo, hi = 1e-9, 200.0
    if not f(lo) * f(hi) < 0:
        return None
    return scipy.optimize.brentq(f, lo, hi, xtol=1e-13, rtol=1e-15)


def gamma_map(x, gamma):
    """np.power(float32 plane, float64 gamma) assigned into the float32 space, as the reference does under numpy 2."""
    return np.power(x.astype(np.float64), np.float64(gamma)).astype(F32)
