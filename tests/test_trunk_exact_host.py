"""The host statements behind tests/test_gpu_trunk_exact.py and tests/test_gpu_tail_exact.py, checked on the CPU:

  a. ``oracle_bn_act`` (oracle/chain.c), the trunk epilogue in single IEEE fp32 operations, lies within one fp32 ulp of the
     float64 ``oracle.bn_act`` for every option combination, keeps NaN and +-inf, and its ReLU returns 0 for negative values;
     ``conv1x1_chain`` is ``gemm_nt_chain`` per image
  b. the order-free generators of tests/tail_data.py really are order-free: three permutations summed in float64 and the
     sequential fp32 sum give one value
  c. the non-finite rule of include/mdx.h ("extraction") is what torch does on the CPU -- taken from the reference, not from
     the kernels.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_data as TD
from oracle import chain as OC
from oracle import oracle as O

F32 = np.float32


def _params(rng, c):
    return (rng.standard_normal(c).astype(F32), rng.uniform(0.2, 3.0, c).astype(F32), rng.uniform(0.5, 1.5, c).astype(F32),
            rng.standard_normal(c).astype(F32))


# ------------------------------------------------------------------------------------------------ a. the epilogue statement

@pytest.mark.parametrize("shape", [(2, 5, 3, 7), (1, 67, 1, 1), (3, 1, 4, 4), (2, 64, 16, 16)])
def test_bn_act_exact_is_within_one_ulp_of_float64(shape):
    """Every option combination on random data against the float64 ``oracle.bn_act``.

    "One ulp of the result" holds as it stands wherever no shift of the other sign cancels the product (asserted below for the
    combinations without mean, bias and residual).  Where terms cancel, the result can be arbitrarily smaller than the terms
    whose roundings it inherits, so no fp32 statement in ANY operation order is within an ulp of a small result (measured on
    these data: up to 2e5 ulps of the result in 4 % of the elements).  The bound there is the statement's own rounding analysis,
    u = 2^-24:  var + eps, sqrtf, 1 / ., . * weight round ``scale`` by at most (1/2 + 1 + 1 + 1) u; x - mean adds u; so the
    product term |x - mean| |scale| carries 4.5 u (+ second order), the fma and the residual add round the result (half an ulp
    each, the first one relative to y = result - residual):
        |got - want| <= ulp(result) + 6 u (|x - mean| |scale| + |bias| + |residual|)."""
    rng = np.random.default_rng(sum(shape))
    c = shape[1]
    x = (rng.standard_normal(shape) * 2).astype(F32)
    res = rng.standard_normal(shape).astype(F32)
    mean, var, wt, bs = _params(rng, c)
    per = lambda v: v.astype(np.float64).reshape(1, c, 1, 1)
    for use_bn, use_w, use_b, use_res, relu, add_zero in itertools.product((False, True), repeat=6):
        kw = dict(mean=mean if use_bn else None, var=var if use_bn else None, weight=wt if use_w else None,
                  bias=bs if use_b else None, residual=res if use_res else None, relu=relu)
        got = OC.bn_act_exact(x, eps=1e-5, add_zero=add_zero, **kw)
        want = O.bn_act(x, mean if use_bn else np.zeros(c, F32), var if use_bn else np.ones(c, F32), kw["weight"], kw["bias"],
                        1e-5 if use_bn else 0.0, kw["residual"], relu)
        scale = (1.0 / np.sqrt(per(var) + 1e-5) if use_bn else 1.0) * (per(wt) if use_w else 1.0)
        terms = np.abs((x - (per(mean) if use_bn else 0.0)) * scale) + (np.abs(per(bs)) if use_b else 0.0) + (np.abs(res) if use_res else 0.0)
        ulp = np.spacing(np.maximum(np.abs(want), np.finfo(F32).tiny)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        bound = ulp + 6 * 2.0 ** -24 * terms
        assert (err <= bound).all(), (sorted(k for k, v in kw.items() if v is not None and v is not False), float((err / bound).max()))
        if not (use_bn or use_b or use_res):
            assert (err <= ulp).all()


def test_bn_act_exact_single_operations():
    """Every line of the statement against numpy's fp32 scalars (each a correctly rounded IEEE operation)."""
    rng = np.random.default_rng(5)
    shape = (2, 6, 5, 3)
    x, res = (rng.standard_normal(shape) * 3).astype(F32), rng.standard_normal(shape).astype(F32)
    mean, var, wt, bs = _params(rng, 6)
    eps = F32(1e-5)
    invstd = (F32(1) / np.sqrt(var + eps, dtype=F32)).astype(F32)
    scale = (invstd * wt).astype(F32)
    d = (x - mean.reshape(1, -1, 1, 1)).astype(F32)
    fma = (d.astype(np.float64) * scale.astype(np.float64).reshape(1, -1, 1, 1) + bs.astype(np.float64).reshape(1, -1, 1, 1))
    # float64 holds the product of two fp32 values exactly and the sum with an fp32 value to 53 bits: its rounding to fp32 is
    # the fma's except in a double-rounding tie, which these data do not hit (asserted: no value half way between two floats)
    y = fma.astype(F32)
    half_way = np.abs(np.abs(fma - y.astype(np.float64)) - np.spacing(np.abs(y)).astype(np.float64) / 2) < np.spacing(np.abs(fma))
    assert not half_way.any()
    want = np.maximum((y + res).astype(F32), F32(0))
    np.testing.assert_array_equal(OC.bn_act_exact(x, mean, var, wt, bs, 1e-5, res, True, add_zero=False), want)
    np.testing.assert_array_equal(OC.bn_act_exact(x, mean, var, wt, bs, 1e-5, None, False, add_zero=True), y)


def test_bn_act_exact_non_finite_and_negative_values():
    x = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 0.0, 2.5, -1e-30], dtype=F32).reshape(1, 1, 2, 4)
    for add_zero in (False, True):
        plain = OC.bn_act_exact(x, relu=False, add_zero=add_zero)
        np.testing.assert_array_equal(plain, x)
        got = OC.bn_act_exact(x, relu=True, add_zero=add_zero).reshape(-1)
        assert np.isnan(got[0]) and got[1] == np.inf
        np.testing.assert_array_equal(got[2:], np.array([0, 0, 0, 0, 2.5, 0], dtype=F32))
    # what mdx_bn_act's "+ 0" changes: a -0 out of the fma (bias -0, or a negative product that underflows) becomes +0
    tiny = np.full((1, 1, 1, 1), -1e-30, F32)
    for add_zero in (False, True):
        y = OC.bn_act_exact(tiny, weight=np.array([1e-30], F32), relu=False, add_zero=add_zero)
        assert y[0, 0, 0, 0] == 0 and np.signbit(y[0, 0, 0, 0]) == (not add_zero)
    res = np.zeros_like(x)
    res.reshape(-1)[6] = np.nan
    got = OC.bn_act_exact(x, residual=res, relu=True).reshape(-1)
    assert np.isnan(got[[0, 6]]).all() and got[1] == np.inf and (got[[2, 3, 4, 5, 7]] == 0).all()
    # inf - inf and 0 * inf follow IEEE
    got = OC.bn_act_exact(np.full((1, 1, 1, 2), np.inf, F32), mean=np.array([np.inf], F32), var=np.ones(1, F32), relu=True)
    assert np.isnan(got).all()
    with pytest.raises(ValueError):
        OC.bn_act_exact(x, mean=np.zeros(1, F32))


def test_conv1x1_chain_is_the_gemm_chain_per_image():
    rng = np.random.default_rng(9)
    x, w = rng.standard_normal((3, 48, 5, 7)).astype(F32), rng.standard_normal((64, 48)).astype(F32)
    got = OC.conv1x1_chain(x, w)
    assert got.shape == (3, 64, 5, 7) and got.dtype == F32
    for b in range(3):
        np.testing.assert_array_equal(got[b].reshape(64, 35), OC.gemm_nt_chain(w, x[b].reshape(48, 35).T))
    np.testing.assert_allclose(got, np.einsum("oc,nchw->nohw", w.astype(np.float64), x.astype(np.float64)), rtol=0, atol=2e-5)
    xi, wi = rng.integers(-8, 9, (2, 80, 1, 33)).astype(F32), rng.integers(-8, 9, (64, 80)).astype(F32)
    np.testing.assert_array_equal(OC.conv1x1_chain(xi, wi), np.einsum("oc,nchw->nohw", wi.astype(np.float64), xi.astype(np.float64)))


# ------------------------------------------------------------------------------------------------ b. order-free data

def _sums_agree(rows):
    """float64 sums of three permutations and the sequential fp32 sum of every row: one value."""
    rows = np.asarray(rows, dtype=F32)
    rows = rows.reshape(-1, rows.shape[-1])
    rng = np.random.default_rng(rows.shape[-1])
    seq = np.add.accumulate(rows, axis=1, dtype=F32)[:, -1]                  # one fp32 addition per element, in order
    for _ in range(3):
        perm = rng.permutation(rows.shape[1])
        np.testing.assert_array_equal(rows[:, perm].astype(np.float64).sum(axis=1), seq.astype(np.float64))
        np.testing.assert_array_equal(np.add.accumulate(rows[:, perm], axis=1, dtype=F32)[:, -1], seq)


def test_tail_generators_are_order_free():
    sizes = TD.plane_sizes()
    assert sizes[:132] == list(range(1, 133)) and {64, 65, 256, 257, 260, 1024, 1028} <= set(sizes) and len(sizes) == 159
    for hw in sizes:
        h, w = TD.factor(hw)
        assert h * w == hw and (w > 1 or hw == 1)
        if hw > 3 and any(hw % k == 0 for k in range(2, hw)):
            assert h > 1
        hot = TD.one_hot_maps(2 if hw % 7 == 0 else 1, hw + (hw % 7 == 0), hw)
        flat = hot.reshape(hot.shape[0], hot.shape[1], hw)
        assert ((flat != 0).sum(axis=2) == 1).all()
        assert set(np.argmax(flat[0], axis=1)) == set(range(hw))             # every position is some channel's hot one
        dense = TD.dense_maps(1, 3, hw)
        assert dense.min() >= 1 and dense.max() <= 8
        for data in (flat, np.maximum(flat, F32(TD.GEM_EPS)), dense.reshape(1, 3, hw)):
            TD.assert_order_free(data)
            _sums_agree(data)
    for d in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 4097):
        rows = TD.int_rows(3, d, seed=1) + TD.int_rows(1, d, seed=2)          # rows with a bias added: |v| <= 8
        TD.assert_order_free(rows, squares=True)
        _sums_agree(rows.astype(np.float64) ** 2)
        eight = TD.int_rows(8, d, seed=3)
        TD.assert_order_free(np.add.accumulate(eight, axis=0), squares=True)  # the sums over 1..8 scales
    # the region vectors of R-MAC on the one-hot map: squares up to 2^14, 143 of them
    TD.assert_order_free(np.exp2(np.arange(143) % 8)[None, :], squares=True)
    with pytest.raises(AssertionError):
        TD.assert_order_free(np.array([[1.0, 2.0 ** -24, 1.0]]))
    with pytest.raises(AssertionError):
        TD.assert_order_free(np.full((1, 5000), 4097.0), squares=True)


def test_tail_restatements_agree_with_the_float64_oracle():
    x = TD.dense_maps(2, 5, 35)
    np.testing.assert_allclose(TD.spoc(x), O.spoc(x), rtol=1e-6)
    np.testing.assert_array_equal(TD.mac(x), O.mac(x))
    np.testing.assert_allclose(TD.gem1(x), O.gem(x, 1.0, TD.GEM_EPS), rtol=1e-6)
    rows = TD.int_rows(4, 257)
    np.testing.assert_allclose(TD.l2n_rows(rows), O.l2n(rows), rtol=1e-6)
    np.testing.assert_allclose(TD.ms_aggregate(rows), O.ms_aggregate(rows, 1.0), rtol=1e-6)
    regions = [(0, 0, 5, 7), (1, 2, 3, 3), (4, 6, 1, 1)]
    want = sum(O.l2n(x[:, :, i:i + h, j:j + w].reshape(2, 5, -1).max(axis=2)) for i, j, h, w in regions)
    np.testing.assert_allclose(TD.rmac(x, regions), want, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ c. the rule is torch's

def test_the_non_finite_rule_is_what_torch_does():
    nan, inf = float("nan"), float("inf")
    t = torch.tensor([nan, inf, -inf, -1.0, 2.0])
    r = torch.relu(t)
    assert torch.isnan(r[0]) and r[1] == inf and r[2] == 0 and r[3] == 0 and r[4] == 2
    c = t.clamp(min=1e-6)
    assert torch.isnan(c[0]) and c[1] == inf and abs(float(c[2]) - 1e-6) < 1e-12 and c[4] == 2
    x = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5) / 7
    x[1, 2, 3, 4] = nan
    x[0, 1, 0, 0] = inf
    for pooled in (F.adaptive_max_pool2d(x, 1), F.max_pool2d(x, (4, 5)), x.mean(dim=(2, 3), keepdim=True),
                   F.avg_pool2d(x.clamp(min=1e-6).pow(3), (4, 5)).pow(1 / 3)):
        mask = torch.isnan(pooled.reshape(2, 3))
        assert mask[1, 2] and int(mask.sum()) == 1                           # its plane, no other
        assert pooled.reshape(2, 3)[0, 1] == inf
    o = F.adaptive_max_pool2d(x, 1).reshape(2, 3)
    o = o / (torch.norm(o, p=2, dim=1, keepdim=True) + 1e-6)                 # LF.l2n: the descriptor of that image, no other
    assert torch.isnan(o[1]).all() and not torch.isnan(o[0, [0, 2]]).any()
    # batch-norm + residual + relu: the element itself, no other; the same mask as the statement
    rng = np.random.default_rng(1)
    a = rng.standard_normal((2, 3, 4, 5)).astype(F32)
    res = rng.standard_normal((2, 3, 4, 5)).astype(F32)
    a[1, 0, 2, 2], a[0, 2, 1, 1], res[0, 0, 0, 3] = nan, inf, nan
    mean, var, wt, bs = _params(rng, 3)
    for relu in (False, True):
        y = F.batch_norm(torch.from_numpy(a), torch.from_numpy(mean), torch.from_numpy(var), torch.from_numpy(wt), torch.from_numpy(bs),
                         False, 0.0, 1e-5) + torch.from_numpy(res)
        y = torch.relu(y) if relu else y
        want = OC.bn_act_exact(a, mean, var, wt, bs, 1e-5, res, relu)
        np.testing.assert_array_equal(np.isnan(y.numpy()), np.isnan(want))
        assert int(np.isnan(want).sum()) == 2 and np.isnan(want[1, 0, 2, 2]) and np.isnan(want[0, 0, 0, 3])
        assert want[0, 2, 1, 1] == np.sign(wt[2]) * np.inf or (relu and want[0, 2, 1, 1] == 0)
        fin = np.isfinite(want)
        np.testing.assert_allclose(y.numpy()[fin], want[fin], rtol=2e-6, atol=2e-6)
    # a 1x1 convolution: the pixel column of the NaN, every output channel
    xx = torch.from_numpy(rng.standard_normal((1, 16, 3, 3)).astype(F32))
    xx[0, 5, 1, 2] = nan
    ww = torch.from_numpy(rng.standard_normal((64, 16, 1, 1)).astype(F32))
    got = torch.isnan(F.conv2d(xx, ww)).numpy()
    want = np.isnan(OC.conv1x1_chain(xx.numpy(), ww.numpy().reshape(64, 16)))
    np.testing.assert_array_equal(got, want)
    assert want[0, :, 1, 2].all() and int(want.sum()) == 64
