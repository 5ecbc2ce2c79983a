"""What the U-Net tests share: a numpy restatement of ``mdx_bn_act_into`` (include/mdx_unet.h), one float32 operation per line; the
configurations the goldens of tests/golden/make_golden_unet.py were made at; and the rule that fills a network's parameters, which
the generator and the tests both run (the golden stores no weights)."""
import numpy as np

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
f32 = np.float32


def fma32(a, b, c):
    """fmaf on float32 arrays: the float64 product of two float32 is exact, the float64 sum rounds once, and rounding that to
    float32 is the fused result except where the double rounding meets a tie -- which ``fix`` detects and repairs by the exact
    residual (the sum's error is recovered with two-sum)."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                   # exact
        s = p + c                                   # one rounding, to float64
        bb = s - p
        err = (p - (s - bb)) + (c - bb)             # two-sum: p + c == s + err exactly
        r = s.astype(np.float32)
        # r is wrong only if s sat exactly half way between two float32 and err says the true sum lies on the other side
        back = r.astype(np.float64)
        up = np.nextafter(r, f32(np.inf)).astype(np.float64)
        down = np.nextafter(r, f32(-np.inf)).astype(np.float64)
        half_up = (s - back == (up - back) / 2) & (err > 0) & np.isfinite(up)
        half_down = (s - back == (down - back) / 2) & (err < 0) & np.isfinite(down)
        r = np.where(half_up, up.astype(np.float32), np.where(half_down, down.astype(np.float32), r))
    return r


def bn_act_into(x, mean=None, var=None, weight=None, bias=None, eps=0.0, act=ACT_NONE, slope=0.0):
    """x float32 [N, C, HW] -> float32 [N, C, HW]: the value of every element ``mdx_bn_act_into`` writes."""
    x = np.asarray(x, dtype=np.float32)
    c = x.shape[1]
    one = np.ones(c, dtype=np.float32)
    with np.errstate(all="ignore"):
        if var is not None:
            t = (np.asarray(var, dtype=np.float32) + f32(eps)).astype(np.float32)
            root = np.sqrt(t).astype(np.float32)
            invstd = (one / root).astype(np.float32)
        else:
            invstd = one
        scale = (invstd * np.asarray(weight, dtype=np.float32)).astype(np.float32) if weight is not None else invstd
        m = np.asarray(mean, dtype=np.float32) if mean is not None else np.zeros(c, dtype=np.float32)
        shift = np.asarray(bias, dtype=np.float32) if bias is not None else np.zeros(c, dtype=np.float32)
        d = (x - m[None, :, None]).astype(np.float32)
        y = fma32(d, scale[None, :, None], shift[None, :, None])
        if act == ACT_RELU:
            y = np.where(y < 0, f32(0), y)
        elif act == ACT_LEAKY:
            leak = (y * f32(slope)).astype(np.float32)
            y = np.where(y > 0, y, leak)
    return y.astype(np.float32)


def bn_act_into_f64(x, mean=None, var=None, weight=None, bias=None, eps=0.0, act=ACT_NONE, slope=0.0):
    """The same function evaluated in float64 throughout: what the restatement is held to within one ulp of."""
    x = np.asarray(x, dtype=np.float64)
    c = x.shape[1]
    with np.errstate(all="ignore"):
        invstd = 1.0 / np.sqrt(np.asarray(var, dtype=np.float64) + np.float64(f32(eps))) if var is not None else np.ones(c)
        scale = invstd * np.asarray(weight, dtype=np.float64) if weight is not None else invstd
        m = np.asarray(mean, dtype=np.float64) if mean is not None else np.zeros(c)
        shift = np.asarray(bias, dtype=np.float64) if bias is not None else np.zeros(c)
        y = (x - m[None, :, None]) * scale[None, :, None] + shift[None, :, None]
        if act == ACT_RELU:
            y = np.where(y < 0, 0.0, y)
        elif act == ACT_LEAKY:
            y = np.where(y > 0, y, y * np.float64(f32(slope)))
    return y


# ------------------------------------------------------------------------------------------------ the golden configurations

# label -> [(constructor parameters, input shape)].  Small widths are not possible (the channel widths are the reference's), small
# depths and images are.  orig_unet: the reference fixes the input width of its last 1x1 convolution at 64, so its forward runs
# with min_channels = 64 only -- the one value the reference can give an output for.
CASES = {
    "identity": [({}, (1, 3, 8, 8))],
    "orig_unet": [({"nested_levels": 2, "min_channels": 64}, (1, 3, 32, 32))],
    "p2p_unet": [({"nested_levels": 3}, (1, 3, 32, 32))],
    "outconv_unet": [({"nested_levels": 2, "batchnorm": True, "dropout": 0.5, "outconv_channels": 8}, (1, 3, 24, 40))],
    "outconv_dynint_unet": [({"nested_levels": 3, "batchnorm": True, "outconv_channels": 8}, (1, 3, 24, 40)),
                            ({"nested_levels": 3, "batchnorm": True, "outconv_channels": 8}, (1, 3, 27, 35))],
    "shallow_p2p_unet": [({"nested_levels": 2}, (1, 3, 32, 32))],
    "inconv_p2p_unet": [({"nested_levels": 2}, (1, 3, 24, 40))],
    "aligned_p2p_unet": [({"nested_levels": 2}, (1, 3, 32, 32))],
}
SEED = 2100


def case_key(label, k):
    return "%s_%d" % (label, k)


def case_input(label, k):
    shape = CASES[label][k][1]
    return np.random.default_rng(SEED + 17 * k + len(label)).standard_normal(shape).astype(np.float32)


def fill(module, seed=SEED):
    """Every parameter and BatchNorm buffer of ``module`` from one seeded rule, in sorted key order: weights N(0, 2 / fan-in) with
    fan-in = the product of all dimensions but the first, BatchNorm scales around 1, biases and running means small, running
    variances in [0.5, 1.5].  Returns the module."""
    import torch
    rng = np.random.default_rng(seed)
    state = module.state_dict()
    new = {}
    for key in sorted(state):
        shape = tuple(state[key].shape)
        if key.endswith("num_batches_tracked"):
            new[key] = state[key]
            continue
        if key.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif key.endswith("running_mean") or key.endswith("bias"):
            v = 0.1 * rng.standard_normal(shape)
        elif len(shape) == 1:
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape) * np.sqrt(2.0 / np.prod(shape[1:]))
        new[key] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    module.load_state_dict(new)
    return module
