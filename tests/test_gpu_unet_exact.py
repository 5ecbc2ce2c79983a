"""mdx_bn_act_into, bit for bit (include/mdx_unet.h): every element is the restatement of tests/unet_restatement.py -- which
tests/test_unet_host.py holds to the C statement ``oracle_bn_act(add_zero = 0)`` and to within one ulp of float64 -- for the three
activations x {batch-norm + affine, bias only, nothing}; on the vector path across the 1024-vector block boundary, the scalar path,
the alignment fallback, both halves of a two-image concat buffer with the other half poisoned, in place, on both sides of the
65 535-plane launch split, with NaN / +-inf / -0 in single elements, and the refusals."""
import itertools

import numpy as np
import pytest
import torch

import unet_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
STATS = ("bn", "bias", "none")
ACTS = ((R.ACT_NONE, 0.0), (R.ACT_RELU, 0.0), (R.ACT_LEAKY, 0.2), (R.ACT_LEAKY, 0.0))
POISON = 0x7FC0BEEF


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def params(c, stats, seed=0):
    rng = np.random.default_rng(seed + c)
    mean, var = rng.standard_normal(c).astype(F32), rng.uniform(0.2, 3.0, c).astype(F32)
    wt, bs = rng.uniform(0.5, 1.5, c).astype(F32) * rng.choice([-1, 1], c).astype(F32), rng.standard_normal(c).astype(F32)
    return {"bn": dict(mean=mean, var=var, weight=wt, bias=bs, eps=1e-5), "bias": dict(bias=bs), "none": {}}[stats]


def call(x, out_view, kw, act, slope):
    from mdir_amd import ops
    return ops.bn_act_into(x, out_view, dev(kw.get("mean")), dev(kw.get("var")), dev(kw.get("weight")), dev(kw.get("bias")),
                           kw.get("eps", 0.0), act, slope)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(shape, ctot=None, c0=0, x=None, offset=0):
    """All activations x statistics for ``x [N,C,H,W]`` into channels [c0, c0 + C) of a poisoned [N,ctot,H,W] buffer that starts
    ``offset`` floats into its allocation; the rest of the buffer must keep its poison."""
    n, c, h, w = shape
    ctot = c if ctot is None else ctot
    if x is None:
        x = (np.random.default_rng(n + c + h * w).standard_normal(shape) * 2).astype(F32)
    xd = dev(x)
    for stats, (act, slope) in itertools.product(STATS, ACTS):
        kw = params(c, stats)
        raw = torch.from_numpy(np.full(offset + n * ctot * h * w, POISON, dtype=np.uint32).view(F32)).to(DEV)
        buf = raw[offset:].view(n, ctot, h, w)
        call(xd, buf[:, c0:c0 + c], kw, act, slope)
        want = np.full((n, ctot, h, w), POISON, dtype=np.uint32).view(F32)
        want[:, c0:c0 + c] = R.bn_act_into(x.reshape(n, c, h * w), act=act, slope=slope, **kw).reshape(shape)
        np.testing.assert_array_equal(bits(buf.cpu().numpy()), bits(want), err_msg="%s %s act=%d slope=%g" % (shape, stats, act, slope))
        assert (bits(raw[:offset].cpu().numpy()) == POISON).all()
    np.testing.assert_array_equal(bits(xd.cpu().numpy()), bits(x))          # x is read only


@pytest.mark.parametrize("hw", [4096 + 4, 4096, 4096 - 4])
def test_vector_path_across_the_block_boundary(hw):
    check((1, 3, 1, hw))


@pytest.mark.parametrize("hw", [15, 1])
def test_scalar_path(hw):
    check((1, 3, 1, hw))
    check((2, 2, 1, hw), ctot=5, c0=2)


def test_alignment_fallback_for_a_slice_off_the_16_byte_grid():
    # C * HW odd and c0 > 0: the slice starts an odd number of floats into a 512-byte-aligned buffer
    check((1, 3, 1, 5), ctot=6, c0=3)
    # HW % 4 == 0 but the buffer itself starts off the grid, for one image and for two
    check((1, 3, 2, 8), ctot=6, c0=3, offset=1)
    check((2, 3, 2, 8), ctot=6, c0=0, offset=3)


@pytest.mark.parametrize("c0", [0, 3])
def test_two_images_into_one_half_of_the_concat_buffer(c0):
    check((2, 3, 4, 8), ctot=6, c0=c0)          # vector path
    check((2, 3, 3, 5), ctot=6, c0=c0)          # scalar path


def test_in_place_form():
    x = (np.random.default_rng(5).standard_normal((2, 3, 4, 6)) * 2).astype(F32)
    for stats, (act, slope) in itertools.product(STATS, ACTS):
        kw = params(3, stats)
        xd = dev(x)
        got = call(xd, xd, kw, act, slope)
        assert got.data_ptr() == xd.data_ptr()
        np.testing.assert_array_equal(bits(xd.cpu().numpy()), bits(R.bn_act_into(x.reshape(2, 3, 24), act=act, slope=slope, **kw).reshape(x.shape)))


@pytest.mark.parametrize("planes", [65535, 65536, 65537])
def test_both_sides_of_the_launch_split(planes):
    # N * C = planes at HW = 4: the planes beyond 65 535 go to a second launch, with their own image and channel index
    n = 3 if planes % 3 == 0 else 1
    c = planes // n
    assert n * c == planes
    x = (np.random.default_rng(planes).standard_normal((n, c, 2, 2)) * 2).astype(F32)
    xd = dev(x)
    for stats, (act, slope) in (("bn", (R.ACT_LEAKY, 0.2)), ("bias", (R.ACT_RELU, 0.0)), ("none", (R.ACT_NONE, 0.0))):
        kw = params(c, stats)
        buf = torch.from_numpy(np.full((n, c + 1, 2, 2), POISON, dtype=np.uint32).view(F32)).to(DEV)
        call(xd, buf[:, 1:], kw, act, slope)
        want = np.full((n, c + 1, 2, 2), POISON, dtype=np.uint32).view(F32)
        want[:, 1:] = R.bn_act_into(x.reshape(n, c, 4), act=act, slope=slope, **kw).reshape(x.shape)
        np.testing.assert_array_equal(bits(buf.cpu().numpy()), bits(want))


@pytest.mark.parametrize("hw", [8, 5])
def test_special_values_stay_in_their_own_element(hw):
    x = (np.random.default_rng(hw).standard_normal((2, 3, 1, hw)) * 2).astype(F32)
    x[0, 0, 0, 1], x[0, 1, 0, 2], x[1, 2, 0, 3], x[1, 0, 0, 0], x[0, 2, 0, 4] = np.nan, np.inf, -np.inf, -0.0, 0.0
    check(x.shape, ctot=6, c0=3, x=x)
    from mdir_amd import ops
    xd = dev(x)
    for act, slope in ACTS:
        out = torch.empty_like(xd)
        ops.bn_act_into(xd, out, None, None, None, None, 0.0, act, slope)
        got = out.cpu().numpy()
        # (-inf * 0 is NaN: a zero slope turns the -inf into one, as torch's leaky_relu does)
        assert np.isnan(got[0, 0, 0, 1]) and np.isnan(got).sum() == 1 + (act == R.ACT_LEAKY and slope == 0.0), (act, slope)
        assert got[0, 1, 0, 2] == np.inf
        # nothing is added after the fma, so a -0 out of it stays -0 through every activation: a negative product that underflows,
        # and -0 * 1 + -0 (an input -0 with a +0 shift is +0 by IEEE, and is in `check` above)
        tiny = torch.full((1, 1, 1, hw), -1e-30, device=DEV)
        got = ops.bn_act_into(tiny, torch.empty_like(tiny), None, None, torch.full((1,), 1e-30, device=DEV), None, 0.0, act, slope).cpu().numpy()
        assert (got == 0).all() and np.signbit(got).all(), (act, slope)
        zero = torch.full((1, 1, 1, hw), -0.0, device=DEV)
        got = ops.bn_act_into(zero, torch.empty_like(zero), None, None, None, torch.full((1,), -0.0, device=DEV), 0.0, act, slope).cpu().numpy()
        assert (got == 0).all() and np.signbit(got).all(), (act, slope)


def test_refusals():
    from mdir_amd import ops
    x = torch.zeros((2, 3, 2, 4), device=DEV)
    buf = torch.zeros((2, 6, 2, 4), device=DEV)
    flat = torch.zeros(2 * 3 * 2 * 4 + 8, device=DEV)
    with pytest.raises(ValueError, match="overlap"):               # shifted by one plane: a partial overlap
        ops.bn_act_into(flat[:48].view(2, 3, 2, 4), flat[8:56].view(2, 3, 2, 4))
    with pytest.raises(ValueError, match="overlap"):               # x is itself the lower half of the buffer it is sent into
        ops.bn_act_into(buf.view(-1)[:24].view(1, 3, 2, 4), buf[:1, 1:4])
    with pytest.raises(ValueError, match="channel slice"):         # a batch stride below C * HW
        ops.bn_act_into(x, torch.as_strided(flat, (2, 3, 2, 4), (16, 8, 4, 1)))
    with pytest.raises(ValueError, match="channel slice"):         # every other channel
        ops.bn_act_into(x, buf[:, ::2])
    with pytest.raises(ValueError, match="channel slice"):         # a spatial crop
        ops.bn_act_into(x[:, :, :, :2].contiguous(), buf[:, :3, :, :2])
    with pytest.raises(ValueError, match="shaped like x"):
        ops.bn_act_into(x, buf)
    with pytest.raises(ValueError, match="act="):
        ops.bn_act_into(x, buf[:, :3], act=3)
    with pytest.raises(ValueError, match="slope"):
        ops.bn_act_into(x, buf[:, :3], act=ops.ACT_LEAKY, slope=float("nan"))
    with pytest.raises(ValueError, match="both"):
        ops.bn_act_into(x, buf[:, :3], running_mean=torch.zeros(3, device=DEV))
    assert float(buf.abs().sum()) == 0 and float(flat.abs().sum()) == 0
