"""The trunk kernels, bit for bit: mdx_conv1x1_bn_act and mdx_bn_act against their host statements (oracle/chain.c:
``oracle_gemm_nt_chain`` for the accumulators, ``oracle_bn_act`` for the epilogue; the statements themselves are checked on the
CPU in tests/test_trunk_exact_host.py).

All comparisons are ``np.testing.assert_array_equal`` on the float values (-0 == +0, NaN required in the same places): no
tolerance.  Every output the wrappers allocate is taken from a ``memguard.Arena`` pre-filled with 0xFF (NaN) between guard bands,
so a tile that is not written cannot hide behind the equal bytes of an earlier call.

  a. the convolution's accumulators are the k-ascending fmaf chain (v_mfma_f32_32x32x2_f32), on real-valued data and on
     order-free integer data (there a failure is an indexing defect, not an ordering one): nk = Cin / 16 = 1..5 (the
     double-buffered loop left through its `break` and through its end, the two-fetch prologue), 1 and 3 channel tiles, pixel-tile
     counts with only a partial group, one full group and full + partial groups of the XCD remap, rows off the 16-byte grid, empty
     32-column MFMA tiles; the same contract from the similarity kernel (DescriptorIndex.scores)
  b. the convolution's epilogue: all 2^5 option combinations = ``bn_act_exact(accumulators, add_zero=False)`` = mdx_bn_act
     applied to the plain convolution output
  c. mdx_bn_act = ``bn_act_exact(add_zero=True)``: across the 1024-vector block boundary, the scalar path, the alignment
     fallback, both sides of the 65 535-plane launch split
  d. the 128-pixel-tile instantiation (MDX_CONV_NT=128, read once per process: a child process)
  e. non-finite values: a NaN makes NaN exactly the outputs the reference makes NaN (include/mdx.h, "extraction")
"""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import memguard
from conftest import ROOT
from oracle import chain as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def conv(x, w, mean=None, var=None, weight=None, bias=None, eps=1e-5, residual=None, relu=False):
    """``ops.conv1x1_bn_act`` on host arrays (``w [Cout,Cin]``), its outputs -- the transposed weights too -- in guarded memory
    pre-filled with NaN."""
    from mdir_amd import ops
    arena = memguard.Arena(DEV)
    with memguard.guarded(ops, arena, fill_out=0xFF):
        wt = ops.conv1x1_transpose_weights(dev(w))
        out = ops.conv1x1_bn_act(dev(x), wt, dev(mean), dev(var), dev(weight), dev(bias), eps, dev(residual), relu)
    arena.check()
    assert len(arena.names(("output",))) == 2
    return host(out)


def bn_act(x, mean=None, var=None, weight=None, bias=None, eps=1e-5, residual=None, relu=False, x_align=256, res_align=256):
    """``ops.bn_act_`` in place on a guarded copy of ``x`` (and a guarded residual) at the given address alignments."""
    from mdir_amd import ops
    arena = memguard.Arena(DEV)
    xd = arena.put(x, align=x_align, name="x")
    rd = None if residual is None else arena.put(residual, align=res_align, name="residual")
    assert xd.data_ptr() % 16 == x_align % 16 and (rd is None or rd.data_ptr() % 16 == res_align % 16)
    got = ops.bn_act_(xd, dev(mean), dev(var), dev(weight), dev(bias), eps, rd, relu)
    arena.check()
    arena.check_inputs(except_for=("x",))
    return host(got)


def real_operands(n, cin, cout, hw, seed=0):
    rng = np.random.default_rng(seed + 1000 * n + 7 * cin + 3 * cout + hw)
    return rng.standard_normal((n, cin, 1, hw)).astype(F32), (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(F32)


def integer_operands(n, cin, cout, hw, seed=0):
    """Integers in [-8, 8]: every partial sum is an integer below 64 * Cin <= 2^16 -- exact in any order."""
    rng = np.random.default_rng(seed + 1000 * n + 7 * cin + 3 * cout + hw)
    return rng.integers(-8, 9, (n, cin, 1, hw)).astype(F32), rng.integers(-8, 9, (cout, cin)).astype(F32)


def integer_product(x, w):
    want = np.einsum("oc,nchw->nohw", w.astype(np.float64), x.astype(np.float64))
    assert np.abs(want).max() < 2 ** 24
    return want.astype(F32)


def bn_params(c, seed=0):
    rng = np.random.default_rng(seed + c)
    return dict(mean=rng.standard_normal(c).astype(F32), var=rng.uniform(0.2, 3.0, c).astype(F32),
                weight=rng.uniform(0.5, 1.5, c).astype(F32) * rng.choice([-1, 1], c).astype(F32), bias=rng.standard_normal(c).astype(F32))


# ------------------------------------------------------------------------------------------------ a. the convolution is the chain

CINS, COUTS = (16, 32, 48, 64, 80), (64, 192)
PIXELS = [(1, 1), (1, 31), (1, 33), (1, 63), (1, 64), (1, 65), (2, 127), (3, 200), (1, 512), (5, 250)]


def check_conv_is_the_chain(n, hw, cins=CINS, couts=COUTS, real=True):
    for cin, cout in itertools.product(cins, couts):
        x, w = integer_operands(n, cin, cout, hw)
        np.testing.assert_array_equal(conv(x, w), integer_product(x, w), err_msg="order-free data: an indexing defect %s" % ((n, cin, cout, hw),))
        if real:
            x, w = real_operands(n, cin, cout, hw)
            np.testing.assert_array_equal(conv(x, w), OC.conv1x1_chain(x, w), err_msg="real-valued data: the accumulation order %s" % ((n, cin, cout, hw),))


@pytest.mark.parametrize("n,hw", PIXELS)
def test_conv1x1_accumulators_are_the_fmaf_chain(n, hw):
    """Pixel-tile counts N * ceil(HW / 64) = 1, 1, 1, 1, 1, 2, 4, 12, 8, 20 against Cin = 16..80 (nk = 1..5) and 1 / 3 channel
    tiles."""
    check_conv_is_the_chain(n, hw)


def test_conv1x1_long_loop_is_the_fmaf_chain():
    check_conv_is_the_chain(1, 70, cins=(1024,), couts=(64,))


@pytest.mark.parametrize("cin", [64, 128])
def test_conv1x1_and_the_similarity_kernel_keep_one_contract(cin):
    """Two independent kernels (32x32x2 MFMA tiles here, 16x16x4 there), one stated order: out[b] = scores of the weight rows
    against the pixels of image b as dimension-major queries."""
    from mdir_amd import ops
    for (n, hw), cout in itertools.product([(2, 127), (1, 65)], COUTS):
        x, w = real_operands(n, cin, cout, hw, seed=5)
        got = conv(x, w)
        ix = ops.DescriptorIndex(dev(w), "ND")
        try:
            for b in range(n):
                sc = host(ix.scores(dev(x[b].reshape(cin, hw)), "DN"))                 # [HW, Cout]
                np.testing.assert_array_equal(got[b].reshape(cout, hw), sc.T, err_msg=str((n, cin, cout, hw, b)))
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------ b. the epilogue

@pytest.mark.parametrize("n,cin,cout,hw", [(2, 80, 192, 65), (1, 16, 64, 7)])
def test_conv1x1_epilogue_is_the_statement(n, cin, cout, hw):
    from mdir_amd import ops
    x, w = real_operands(n, cin, cout, hw, seed=3)
    acc = OC.conv1x1_chain(x, w)
    plain = conv(x, w)
    np.testing.assert_array_equal(plain, acc)
    p = bn_params(cout, seed=1)
    res = np.random.default_rng(cout).standard_normal(acc.shape).astype(F32)
    for use_bn, use_w, use_b, use_res, relu in itertools.product((False, True), repeat=5):
        kw = dict(mean=p["mean"] if use_bn else None, var=p["var"] if use_bn else None, weight=p["weight"] if use_w else None,
                  bias=p["bias"] if use_b else None, residual=res if use_res else None, relu=relu)
        what = str((n, cin, cout, hw, use_bn, use_w, use_b, use_res, relu))
        got = conv(x, w, eps=1e-5, **kw)
        np.testing.assert_array_equal(got, OC.bn_act_exact(acc, eps=1e-5, add_zero=False, **kw), err_msg=what)
        # include/mdx.h: "the arithmetic of mdx_bn_act applied to the accumulators"
        np.testing.assert_array_equal(bn_act(plain, eps=1e-5, **kw), got, err_msg=what)


# ------------------------------------------------------------------------------------------------ c. mdx_bn_act

def param_forms(c):
    p = bn_params(c, seed=2)
    return [("full", p), ("no affine", dict(mean=p["mean"], var=p["var"])), ("bias only", dict(bias=p["bias"])), ("nothing", {})]


def check_bn_act(shape, x_align=256, res_align=256):
    rng = np.random.default_rng(shape[1] + shape[3])
    x = (rng.standard_normal(shape) * 2).astype(F32)
    res = rng.standard_normal(shape).astype(F32)
    for (form, p), use_res, relu in itertools.product(param_forms(shape[1]), (False, True), (False, True)):
        if res_align != 256 and not use_res:
            continue
        got = bn_act(x, eps=1e-5, residual=res if use_res else None, relu=relu, x_align=x_align, res_align=res_align, **p)
        want = OC.bn_act_exact(x, eps=1e-5, residual=res if use_res else None, relu=relu, add_zero=True, **p)
        np.testing.assert_array_equal(got, want, err_msg=str((shape, form, use_res, relu, x_align, res_align)))


@pytest.mark.parametrize("hw", [4, 1020, 1024, 1028, 4092, 4096, 4100])
def test_bn_act_vector_path_across_the_block_boundary(hw):
    """H*W % 4 == 0: float4 accesses, 1024 of them per workgroup -- one short of, at, and one past one and four blocks."""
    check_bn_act((1, 3, 1, hw))


@pytest.mark.parametrize("hw", [1, 3, 1023, 1025, 4099])
def test_bn_act_scalar_path(hw):
    check_bn_act((1, 3, 1, hw))


def test_bn_act_alignment_fallback():
    """H*W % 4 == 0 but x (then only the residual) 4 bytes past a 16-byte boundary: the scalar kernel, the same values."""
    check_bn_act((1, 3, 1, 1024), x_align=4)
    check_bn_act((1, 3, 1, 1024), res_align=4)


@pytest.mark.parametrize("hw", [4, 3])
def test_bn_act_on_both_sides_of_the_launch_split(hw):
    """3 x 21 846 = 65 538 planes: the second launch starts at plane 65 535 = image 2, channel 21 843, and its channel index
    wraps inside it."""
    check_bn_act((3, 21846, 1, hw))


# ------------------------------------------------------------------------------------------------ d. 128-pixel tiles

NT128_PIXELS, NT128_CINS = [(1, 65), (3, 200), (1, 129)], (16, 48)


def conv_nt128_table():
    """The order-free half of (a) on the shapes of the <128, 16> instantiation (the child process of the test below)."""
    assert os.environ.get("MDX_CONV_NT") == "128"
    for n, hw in NT128_PIXELS:
        check_conv_is_the_chain(n, hw, cins=NT128_CINS, real=False)


def test_conv1x1_128_pixel_tiles():
    """MDX_CONV_NT is read once per process: a child runs the order-free table on the 128-pixel-tile kernel."""
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_trunk_exact as T; T.conv_nt128_table(); print('CONV-NT128-OK')"
            % (ROOT, os.path.join(ROOT, "tests")))
    proc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MDX_CONV_NT="128"), text=True, capture_output=True, timeout=300)
    assert proc.returncode == 0 and "CONV-NT128-OK" in proc.stdout, (proc.stdout[-2000:], proc.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ e. non-finite values

@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("where", ["x", "residual"])
def test_bn_act_keeps_nan_and_inf_in_their_element(where, relu):
    """One NaN and one +inf in x (in the residual): NaN exactly where the statement and torch on the CPU have it -- the element
    itself -- and every other element bit-exact.  (fmaxf(NaN, 0) = 0 made a damaged activation a plausible one.)"""
    import torch.nn.functional as F
    for shape in [(2, 5, 1, 1028), (2, 5, 1, 67)]:                          # the float4 and the scalar kernel
        rng = np.random.default_rng(shape[3])
        x = (rng.standard_normal(shape) * 2).astype(F32)
        res = rng.standard_normal(shape).astype(F32)
        bad = x if where == "x" else res
        bad[1, 3, 0, shape[3] - 2], bad[0, 4, 0, 5] = np.nan, np.inf
        p = bn_params(5, seed=4)
        got = bn_act(x, eps=1e-5, residual=res, relu=relu, **p)
        want = OC.bn_act_exact(x, eps=1e-5, residual=res, relu=relu, add_zero=True, **p)
        np.testing.assert_array_equal(got, want)
        t = F.batch_norm(torch.from_numpy(x), *(torch.from_numpy(p[k]) for k in ("mean", "var", "weight", "bias")), False, 0.0, 1e-5) \
            + torch.from_numpy(res)
        t = torch.relu(t) if relu else t
        np.testing.assert_array_equal(np.isnan(got), np.isnan(t.numpy()))
        mask = np.zeros(shape, dtype=bool)
        mask[1, 3, 0, shape[3] - 2] = True
        np.testing.assert_array_equal(np.isnan(got), mask)
        assert np.isinf(got[0, 4, 0, 5]) or (relu and got[0, 4, 0, 5] == 0 and t.numpy()[0, 4, 0, 5] == 0)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("where", ["x", "residual"])
def test_conv1x1_keeps_nan_in_its_pixel_column(where, relu):
    """A NaN input element: its pixel column, every output channel, no other pixel; a NaN residual element: that element.  The
    +inf follows IEEE arithmetic (the chain's and the statement's)."""
    import torch.nn.functional as F
    n, cin, cout, hw = 2, 48, 192, 65
    x, w = real_operands(n, cin, cout, hw, seed=8)
    res = np.random.default_rng(8).standard_normal((n, cout, 1, hw)).astype(F32)
    p = bn_params(cout, seed=6)
    mask = np.zeros((n, cout, 1, hw), dtype=bool)
    if where == "x":
        x[1, 17, 0, 64], x[0, 3, 0, 31] = np.nan, np.inf
        mask[1, :, 0, 64] = True
    else:
        res[1, 100, 0, 64], res[0, 7, 0, 31] = np.nan, np.inf
        mask[1, 100, 0, 64] = True
    got = conv(x, w, eps=1e-5, residual=res, relu=relu, **p)
    want = OC.bn_act_exact(OC.conv1x1_chain(x, w), eps=1e-5, residual=res, relu=relu, add_zero=False, **p)
    np.testing.assert_array_equal(np.isnan(want), mask)
    np.testing.assert_array_equal(got, want)
    t = F.batch_norm(F.conv2d(torch.from_numpy(x), torch.from_numpy(w).reshape(cout, cin, 1, 1)),
                     *(torch.from_numpy(p[k]) for k in ("mean", "var", "weight", "bias")), False, 0.0, 1e-5) + torch.from_numpy(res)
    t = torch.relu(t) if relu else t
    np.testing.assert_array_equal(np.isnan(got), np.isnan(t.numpy()))
    np.testing.assert_array_equal(np.isinf(got), np.isinf(t.numpy()))


def test_fused_trunk_and_module_calls_agree_on_where_nan_is(monkeypatch):
    """ResNet50 at 1 x 3 x 67 x 59 with one NaN input pixel: MDIR_AMD_FUSED_TRUNK=1 and =0 give the same NaN mask."""
    from mdir_amd.backbones import TrunkSequential, build_features
    torch.manual_seed(5)
    feats = TrunkSequential(*build_features("resnet50")).eval()
    for m in feats.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.5, 1.2); m.bias.data.normal_(0, 0.1)
    feats = feats.to(DEV)
    x = torch.randn(1, 3, 67, 59, device=DEV)
    x[0, 1, 40, 20] = float("nan")
    with torch.no_grad():
        monkeypatch.setenv("MDIR_AMD_FUSED_TRUNK", "1")
        fused = feats(x)
        monkeypatch.setenv("MDIR_AMD_FUSED_TRUNK", "0")
        plain = feats(x)
    assert fused.shape == plain.shape
    assert bool(torch.isnan(plain).any())
    np.testing.assert_array_equal(host(torch.isnan(fused)), host(torch.isnan(plain)))
