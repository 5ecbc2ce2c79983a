"""mdx_bn_act_f16, bit for bit (include/mdx.h, "fp16 trunk"): every element is ``oracle_bn_act(add_zero = 1)`` of oracle/chain.c
on the input converted to fp32, then ONE conversion to fp16 to nearest even (numpy's ``astype(float16)``; overflow to +-inf).

No tolerance: the fp16 bits must be equal wherever the result is a number (signed zeros included), and NaN must stand in the same
places (the sign and payload of a NaN are not compared: x86 and the GPU make different default NaNs).  ``x`` and the residual lie
inside longer buffers whose other elements must come back untouched.

  a. H*W = 1, 7, 8, 9, 12, 8184, 8192, 8200 with C = 1 and 3: the scalar path, the 8-half vector path (12 is a multiple of 4 but
     not of 8: the fp32 kernel's vector rule would be wrong here), and both sides of one workgroup's 256 x 4 vectors of 8 halves
  b. x and the residual 1..7 elements off the 16-byte grid (the alignment fallback)
  c. 65 535 and 65 536 planes at H*W = 8: both sides of the launch split
  d. all 2^5 combinations of {statistics, weight, bias, residual, relu}
  e. planted values: NaN, +-inf and -0 with and without a residual, fp16 subnormals, a finite input whose result overflows fp16,
     results exactly halfway between two fp16 values with the even neighbour below and above (scale 1, the fp32 result exact)
"""
import itertools

import numpy as np
import pytest
import torch

from oracle import chain as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16 = np.float32, np.float16
PAD = 16                  # elements around x / the residual inside their buffers
SENTINEL = 0x5A5A


def _place(a, off):
    """``a`` (fp16 host array) as a contiguous device view that starts ``off`` elements past a 16-byte boundary, inside a buffer
    filled with a sentinel; returns (view, whole buffer)."""
    buf = torch.full((a.size + 2 * PAD + 8,), SENTINEL, dtype=torch.int16, device=DEV).view(torch.float16)
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + off:PAD + off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    assert view.data_ptr() % 16 == (2 * off) % 16 and view.is_contiguous()
    return view, buf


def _untouched(buf, a, off):
    raw = buf.view(torch.int16).cpu().numpy()
    assert (raw[:PAD + off] == SENTINEL).all() and (raw[PAD + off + a.size:] == SENTINEL).all(), "a write outside the tensor"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bn_act16(x, mean=None, var=None, weight=None, bias=None, eps=1e-5, residual=None, relu=False, x_off=0, res_off=0):
    """``ops.bn_act_`` in place on an fp16 device copy of ``x`` (and of the residual) at the given element offsets."""
    from mdir_amd import ops
    xd, xbuf = _place(x, x_off)
    rd, rbuf = (None, None) if residual is None else _place(residual, res_off)
    got = ops.bn_act_(xd, dev(mean), dev(var), dev(weight), dev(bias), eps, rd, relu)
    assert got is xd and got.dtype == torch.float16
    torch.cuda.synchronize()
    _untouched(xbuf, x, x_off)
    if residual is not None:
        _untouched(rbuf, residual, res_off)
        assert np.array_equal(rd.cpu().numpy().view(np.uint16), residual.view(np.uint16)), "the residual was modified"
    return got.cpu().numpy()


def want16(x, mean=None, var=None, weight=None, bias=None, eps=1e-5, residual=None, relu=False):
    y = OC.bn_act_exact(x.astype(F32), mean, var, weight, bias, eps, None if residual is None else residual.astype(F32), relu, add_zero=True)
    with np.errstate(over="ignore"):
        return y.astype(F16)


def same_bits(got, want, what=""):
    assert got.dtype == F16 and want.dtype == F16 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg="NaN mask %s" % (what,))
    np.testing.assert_array_equal(got.view(np.uint16)[~nan], want.view(np.uint16)[~nan], err_msg=str(what))


def check(x, what="", x_off=0, res_off=0, **kw):
    same_bits(bn_act16(x, x_off=x_off, res_off=res_off, **kw), want16(x, **kw), what)


def bn_params(c, seed=0):
    rng = np.random.default_rng(seed + c)
    return dict(mean=rng.standard_normal(c).astype(F32), var=rng.uniform(0.2, 3.0, c).astype(F32),
                weight=rng.uniform(0.5, 1.5, c).astype(F32) * rng.choice([-1, 1], c).astype(F32), bias=rng.standard_normal(c).astype(F32))


def maps(shape, seed=0):
    rng = np.random.default_rng(seed + sum(shape))
    return (rng.standard_normal(shape) * 3).astype(F16), rng.standard_normal(shape).astype(F16)


# ------------------------------------------------------------------------------------------------ a. plane sizes

@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", [1, 7, 8, 9, 12, 8184, 8192, 8200])
def test_plane_sizes(hw, c):
    x, res = maps((2, c, 1, hw))
    check(x, (hw, c, "residual + relu"), residual=res, relu=True, **bn_params(c))
    check(x, (hw, c, "plain"), **bn_params(c, 1))


# ------------------------------------------------------------------------------------------------ b. alignment

@pytest.mark.parametrize("off", range(1, 8))
def test_off_the_16_byte_grid(off):
    """H*W = 16 and 8200 take the vector path when aligned; ``off`` elements (2 * off bytes) past the grid they must not."""
    for hw in (16, 8200):
        x, res = maps((2, 3, 1, hw), off)
        p = bn_params(3, off)
        aligned = bn_act16(x, residual=res, relu=True, **p)
        for xo, ro in ((off, 0), (0, off), (off, off), (off, 8 - off)):
            got = bn_act16(x, residual=res, relu=True, x_off=xo, res_off=ro, **p)
            same_bits(got, want16(x, residual=res, relu=True, **p), (hw, xo, ro))
            same_bits(got, aligned, (hw, xo, ro, "against the aligned call"))
        check(x, (hw, off, "no residual"), x_off=off, relu=True, **p)


# ------------------------------------------------------------------------------------------------ c. the launch split

@pytest.mark.parametrize("n,c", [(65535, 1), (65536, 1), (21845, 3), (21846, 3)])
def test_both_sides_of_the_launch_split(n, c):
    """65 535, 65 536, 65 535 and 65 538 planes of H*W = 8: the second launch starts at plane 65 535, channel 65 535 % C."""
    rng = np.random.default_rng(n + c)
    x = rng.integers(-2048, 2049, (n, c, 2, 4)).astype(F16)
    res = rng.integers(-64, 65, (n, c, 2, 4)).astype(F16)
    check(x, (n, c), residual=res, relu=True, **bn_params(c, n))


# ------------------------------------------------------------------------------------------------ d. options

def test_all_option_combinations():
    for hw in (8, 9, 12):
        x, res = maps((2, 3, 1, hw), 5)
        p = bn_params(3, 5)
        for stats, weight, bias, residual, relu in itertools.product((False, True), repeat=5):
            kw = dict(mean=p["mean"] if stats else None, var=p["var"] if stats else None, weight=p["weight"] if weight else None,
                      bias=p["bias"] if bias else None, residual=res if residual else None, relu=relu)
            check(x, (hw, stats, weight, bias, residual, relu), **kw)


# ------------------------------------------------------------------------------------------------ e. planted values

def _planted(hw):
    """[1, 1, 1, hw] random maps with special values at fixed places of x and of the residual."""
    x, res = maps((1, 1, 1, hw), 9)
    x, res = x.reshape(-1), res.reshape(-1)
    x[0], x[1], x[2], x[3] = np.nan, np.inf, -np.inf, -0.0
    res[4], res[5], res[6] = np.nan, np.inf, -np.inf
    x[7], res[7] = np.inf, -np.inf                                   # inf - inf
    x[8], res[8] = -0.0, -0.0
    x[9], res[9] = -0.0, 0.0
    sub = np.array([1, 2, 3, 1023, -1, -1023], np.float64) * 2.0 ** -24
    x[10:16] = sub.astype(F16)                                       # fp16 subnormals
    assert (np.abs(x[10:16].astype(np.float64)) < 2.0 ** -14).all() and (x[10:16] != 0).all()
    return x.reshape(1, 1, 1, hw), res.reshape(1, 1, 1, hw)


@pytest.mark.parametrize("hw", [16, 24, 19])
def test_non_finite_values_signed_zeros_and_subnormals(hw):
    """Vector path (16, 24) and scalar path (19)."""
    x, res = _planted(hw)
    one = dict(mean=None, var=None, weight=None, bias=None)
    for relu in (False, True):
        for residual in (None, res):
            check(x, (hw, relu, residual is not None, "scale 1"), residual=residual, relu=relu, **one)
            check(x, (hw, relu, residual is not None, "bn"), residual=residual, relu=relu, **bn_params(1, 2))
    # read off directly, without the oracle: identity epilogue (scale 1, no shift)
    got = bn_act16(x, relu=False).reshape(-1)
    assert np.isnan(got[0]) and got[1] == np.inf and got[2] == -np.inf
    assert got[3] == 0 and not np.signbit(got[3])                                       # -0 + 0 = +0 without a residual
    np.testing.assert_array_equal(got[10:16].view(np.uint16), x.reshape(-1)[10:16].view(np.uint16))    # subnormals pass through
    got = bn_act16(x, relu=True).reshape(-1)
    assert np.isnan(got[0]) and got[1] == np.inf and got[2] == 0 and not np.signbit(got[2])        # NaN stays NaN through the ReLU
    got = bn_act16(x, residual=res, relu=False).reshape(-1)
    assert np.isnan(got[[0, 4, 7]]).all() and got[5] == np.inf and got[6] == -np.inf
    # fmaf(-0 - 0, 1, +0) is +0 (the absent bias is +0), so even a -0 residual cannot bring the sign back: +0 + -0 = +0
    assert got[8] == 0 and not np.signbit(got[8]) and got[9] == 0 and not np.signbit(got[9])
    got = bn_act16(x, residual=res, relu=True).reshape(-1)
    assert np.isnan(got[[0, 4, 7]]).all() and got[6] == 0


@pytest.mark.parametrize("hw", [8, 5])
def test_overflow_and_ties_to_even(hw):
    """Scale 1 (no statistics, no weight), so the fp32 result x + shift (+ residual) is exact.  Channel shifts 1, -1, 2^-25, 60000:
      2048 + 1 = 2049 lies halfway between 2048 (even) and 2050: down;  2050 + 1 = 2051 between 2050 and 2052 (even): up
      the same mirrored with shift -1;  0 + 2^-25 halfway between 0 (even) and the smallest subnormal: down;
      2^-24 + 2^-25 halfway between 2^-24 and 2^-23 (even): up;  60000 + 60000 is finite in fp32 and overflows fp16: +inf"""
    x = np.zeros((1, 4, 1, hw), F16)
    x[0, 0, 0, :4] = [2048, 2050, 4096, 4100]                        # spacing 2, then 4: 4097 -> 4096, 4101 -> 4100 (not ties)
    x[0, 1, 0, :4] = [-2048, -2050, -2052, -2054]
    x[0, 2, 0, :4] = [0, 2.0 ** -24, 2.0 ** -23, -(2.0 ** -24)]
    x[0, 3, 0, :4] = [60000, -60000, 5504, 5536]                     # 65504 = the largest fp16; 65536 is past the halfway 65520: inf
    bias = np.array([1, -1, 2.0 ** -25, 60000], F32)
    got = bn_act16(x, bias=bias)
    same_bits(got, want16(x, bias=bias), hw)
    np.testing.assert_array_equal(got[0, 0, 0, :4].astype(F32), [2048, 2052, 4096, 4100])
    np.testing.assert_array_equal(got[0, 1, 0, :4].astype(F32), [-2048, -2052, -2052, -2056])
    np.testing.assert_array_equal(got[0, 2, 0, :4].astype(np.float64), [0, 2.0 ** -23, 2.0 ** -23, -0.0])   # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0
    assert np.signbit(got[0, 2, 0, 3])
    np.testing.assert_array_equal(got[0, 3, 0, :4].astype(F32), [np.inf, 0, 65504, np.inf])
    # the same ties made by the residual, through the ReLU
    res = np.zeros_like(x)
    res[0, 0, 0, :2] = 1
    res[0, 2, 0, :2] = F16(2.0 ** -24)                               # 0 + 2^-25 + 2^-24 = 1.5, 2^-24 + 2^-25 + 2^-24 = 2.5 (x 2^-24): ties
    shift = np.array([0, -1, 2.0 ** -25, 60000], F32)
    got = bn_act16(x, bias=shift, residual=res, relu=True)
    same_bits(got, want16(x, bias=shift, residual=res, relu=True), (hw, "residual"))
    np.testing.assert_array_equal(got[0, 0, 0, :4].astype(F32), [2048, 2052, 4096, 4100])
    np.testing.assert_array_equal(got[0, 1, 0, :4].astype(F32), [0, 0, 0, 0])
    np.testing.assert_array_equal(got[0, 2, 0, :2].astype(np.float64), [2.0 ** -23, 2.0 ** -23])     # 1.5 -> 2, 2.5 -> 2 (x 2^-24)
