"""The descriptor tail, bit for bit, on order-free data (tests/tail_data.py: every partial sum is exact in fp32, so a reduction
has one right answer in any order; the generators are checked on the CPU in tests/test_trunk_exact_host.py).

All exact comparisons are ``np.testing.assert_array_equal`` against the numpy fp32 restatement of tail_data (one correctly
rounded division / square root at the end); outputs come from a ``memguard.Arena`` pre-filled with 0xFF (NaN) between guard
bands.

  a. plane reductions (mdx_pool_l2n, mdx_pool_multi): MAC, SPoC and GeM p = 1 at every H*W in 1..132 and around 256, 512, 1024
     -- the 16-byte path changes where H*W / 4 crosses 64, the scalar path where H*W crosses 64 -- on one-hot planes (a dropped
     and a doubled position both change the value) and on dense ones; GeM p = 2, 3, 2.92 ends in the library powf and keeps
     rtol 1e-5 against float64, at the same sizes
  b. regions (mdx_roipool, mdx_rmac, mdx_region_sum): 1 x 1, one row, one column, the whole map, 63 / 64 / 65 elements,
     regions that touch the last row and column
  c. rows (mdx_l2n_rows, mdx_ms_aggregate(_batch), mdx_l2n_aggregate) with D next to the 256- and 1024-thread strides
  d. non-finite values: a NaN makes NaN its plane (pooling) and its descriptor (after L2N), and changes no other output
"""
import numpy as np
import pytest
import torch

import memguard
import tail_data as TD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32

SIZES = TD.plane_sizes()
DIMS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 4097]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def guarded(fn, *args, **kw):
    """``fn(*args)`` of mdir_amd.ops with its outputs and workspaces in guarded memory pre-filled with NaN; host arrays back."""
    from mdir_amd import ops
    arena = memguard.Arena(DEV)
    with memguard.guarded(ops, arena, fill_out=0xFF, fill_ws=0xFF):
        out = getattr(ops, fn)(*args, **kw)
    arena.check()
    assert arena.names(("output",))
    return host(out)


def pool(x, kind, p=1.0, eps=TD.GEM_EPS):
    return guarded("pool_l2n", dev(x), kind, p, pool_eps=eps, l2n_eps=None)


RESTATED = {"mac": TD.mac, "spoc": TD.spoc, "gem": TD.gem1}


# ------------------------------------------------------------------------------------------------ a. plane reductions

def plane_maps(hw):
    """The calls of one plane size: C = H*W one-hot channels; every seventh size also two images of H*W + 1 channels (the last
    workgroup of four planes is partial there, or elsewhere, as C runs through every residue); one dense set."""
    maps = [TD.one_hot_maps(1, hw, hw), TD.dense_maps(2, 5, hw)]
    if hw % 7 == 0:
        maps.append(TD.one_hot_maps(2, hw + 1, hw))
    return maps


@pytest.mark.parametrize("kind", ["mac", "spoc", "gem"])
def test_plane_reductions_are_exact_at_every_size(kind):
    for hw in SIZES:
        for x in plane_maps(hw):
            np.testing.assert_array_equal(pool(x, kind), RESTATED[kind](x), err_msg="%s H*W=%d %s" % (kind, hw, x.shape))


@pytest.mark.parametrize("kind", ["mac", "spoc", "gem"])
def test_pool_multi_is_exact_on_three_maps_per_call(kind):
    """Three consecutive sizes per launch, so the scalar and the 16-byte path share a grid; C = the largest size + 1."""
    for i in range(0, len(SIZES), 3):
        hws = SIZES[i:i + 3]
        c = max(hws) + 1
        maps = [TD.one_hot_maps(2, c, hw) for hw in hws]
        got = guarded("pool_multi", [dev(m) for m in maps], kind, 1.0, TD.GEM_EPS)
        assert got.shape == (len(hws), 2, c)
        for s, m in enumerate(maps):
            np.testing.assert_array_equal(got[s], RESTATED[kind](m), err_msg="%s sizes %s map %d" % (kind, hws, s))


@pytest.mark.parametrize("p", [2.0, 3.0, 2.92])
def test_gem_with_a_power_at_every_size(p):
    """The result goes through the library powf: not bit-specifiable.  rtol 1e-5 against float64 (the tolerance of
    test_gpu_kernels.test_pool_l2n_golden) on strictly positive planes, so the clamp does not act."""
    p32 = float(F32(p))
    for hw in SIZES:
        x = TD.dense_maps(2, 5, hw, seed=1)
        want = (x.astype(np.float64).reshape(2, 5, hw) ** p32).mean(axis=2) ** (1.0 / p32)
        np.testing.assert_allclose(pool(x, "gem", p, eps=1e-6), want, rtol=1e-5, atol=0, err_msg="p=%s H*W=%d" % (p, hw))


# ------------------------------------------------------------------------------------------------ b. regions

def region_table(h, w):
    """(row0, col0, height, width): the whole map first; 1 x 1 at the four corners and inside; one row (first, last), one column
    (first, last); 63, 64 and 65 elements, placed at the origin and against the last row and column."""
    regs = [(0, 0, h, w), (0, 0, 1, 1), (h - 1, w - 1, 1, 1), (0, w - 1, 1, 1), (h - 1, 0, 1, 1), (h // 2, w // 3, 1, 1),
            (0, 0, 1, w), (h - 1, 0, 1, w), (0, 0, h, 1), (0, w - 1, h, 1)]
    for area in (63, 64, 65):
        fits = [(a, area // a) for a in range(1, h + 1) if area % a == 0 and area // a <= w]
        assert fits, (h, w, area)
        for rh, rw in (fits[0], fits[-1]):
            regs += [(0, 0, rh, rw), (h - rh, w - rw, rh, rw)]
    assert len(regs) <= 64 and all(i + a <= h and j + b <= w for i, j, a, b in regs)
    return regs


def region_maps(h, w):
    hw = h * w
    return [TD.one_hot_maps(1, hw, hw).reshape(1, hw, h, w), TD.dense_maps(2, 261, hw, seed=2).reshape(2, 261, h, w)]


@pytest.mark.parametrize("h,w", [(13, 11), (9, 16)])
def test_regional_pooling_is_exact(h, w):
    regs = region_table(h, w)
    assert {63, 64, 65} <= {a * b for _, _, a, b in regs}
    for x in region_maps(h, w):
        xd = dev(x)
        for kind in ("mac", "spoc"):
            np.testing.assert_array_equal(guarded("roipool", xd, regs, kind, 1.0), TD.roipool(x, regs, kind), err_msg="%s %s" % (kind, x.shape))
        np.testing.assert_array_equal(guarded("roipool", xd, regs, "gem", 1.0, TD.GEM_EPS),
                                      TD.roipool(np.maximum(x, F32(TD.GEM_EPS)), regs, "spoc"), err_msg="gem %s" % (x.shape,))
        maxima = TD.roipool(x, regs, "mac")
        np.testing.assert_array_equal(guarded("rmac", xd, regs, 1e-6), TD.region_sum(maxima, 1e-6), err_msg="rmac %s" % (x.shape,))
        np.testing.assert_array_equal(guarded("region_sum", dev(maxima), 1e-6), TD.region_sum(maxima, 1e-6))
        np.testing.assert_array_equal(guarded("region_sum", dev(maxima), None), TD.region_sum(maxima, None))


# ------------------------------------------------------------------------------------------------ c. rows

@pytest.mark.parametrize("d", DIMS)
def test_l2n_rows_is_exact(d):
    from mdir_amd import ops
    rows, bias = TD.int_rows(3, d, seed=1), TD.int_rows(1, d, seed=2)[0]
    rows[2] = 0                                                     # an all-zero row: 0 / (0 + eps) = 0
    for b in (None, bias):
        arena = memguard.Arena(DEV)
        got = ops.l2n_rows_(arena.put(rows, name="x"), None if b is None else dev(b), 1e-6)
        arena.check()
        np.testing.assert_array_equal(host(got), TD.l2n_rows(rows, b, 1e-6), err_msg="D=%d bias=%s" % (d, b is not None))


@pytest.mark.parametrize("d", DIMS)
def test_ms_aggregate_entry_points_agree(d):
    """msp = 1, S = 1, 2, 4, 8: the single-descriptor and the batched entry point return the same bits; the mean over a power
    of two of scales and the sum of squares are exact, so both equal ``a / sqrtf(ss)``; against float64 rtol 1e-5 / atol 1e-7
    (the tolerance of test_gpu_kernels.test_pool_multi_l2n_aggregate_two_launch_tail)."""
    for s in (1, 2, 4, 8):
        vecs = np.stack([TD.int_rows(3, d, seed=10 + k) for k in range(s)])                    # [S, B=3, D]
        batch = guarded("ms_aggregate_batch", [dev(v) for v in vecs], 1.0)
        for b in range(3):
            one = guarded("ms_aggregate", [dev(v[b]) for v in vecs], 1.0)
            np.testing.assert_array_equal(one, batch[b], err_msg="D=%d S=%d image %d" % (d, s, b))
        np.testing.assert_array_equal(batch, TD.ms_aggregate(vecs), err_msg="D=%d S=%d" % (d, s))
        a = vecs.astype(np.float64).mean(axis=0)
        np.testing.assert_allclose(batch, a / np.sqrt((a * a).sum(axis=1, keepdims=True)), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("d", DIMS)
def test_l2n_aggregate_is_its_two_kernels(d):
    """mdx_l2n_aggregate == mdx_l2n_rows per scale followed by mdx_ms_aggregate_batch, bit for bit (include/mdx.h)."""
    from mdir_amd import ops
    for s in (1, 3, 8):
        pooled = np.abs(np.stack([TD.int_rows(2, d, seed=20 + k) for k in range(s)]))          # [S, B, D], non-negative as pooled maps
        for msp in (1.0, 2.92):
            got = guarded("l2n_aggregate", dev(pooled), 1e-6, msp)
            rows = [ops.l2n_rows_(dev(pooled[k]), None, 1e-6) for k in range(s)]
            np.testing.assert_array_equal(got, guarded("ms_aggregate_batch", rows, msp), err_msg="D=%d S=%d msp=%s" % (d, s, msp))
            if msp == 1.0:
                np.testing.assert_array_equal(np.stack([host(r) for r in rows]), np.stack([TD.l2n_rows(pooled[k]) for k in range(s)]))


# ------------------------------------------------------------------------------------------------ d. non-finite values

NAN_SIZES = [7, 64, 65, 260, 1023, 1028]


def positions(hw):
    return sorted({0, hw // 2, hw - 1})


@pytest.mark.parametrize("kind,p", [("gem", 3.0), ("gem", 2.92), ("mac", 1.0), ("spoc", 1.0)])
def test_pooling_keeps_nan_in_its_plane(kind, p):
    """One NaN element: its plane is NaN (F.adaptive_max_pool2d, mean and clamp(min=eps).pow(p) all keep it; fmaxf dropped it)
    and no other plane changes a bit; after L2N the descriptor of its image is NaN and no other image changes."""
    from mdir_amd import ops
    for hw in NAN_SIZES:
        clean = TD.dense_maps(3, 6, hw, seed=3)
        want = host(ops.pool_l2n(dev(clean), kind, p, 1e-6, None))
        want_l2n = host(ops.pool_l2n(dev(clean), kind, p, 1e-6, 1e-6))
        for pos in positions(hw):
            x = clean.copy()
            x.reshape(3, 6, hw)[1, 4, pos] = np.nan
            x.reshape(3, 6, hw)[2, 0, pos] = np.inf
            expect = want.copy()
            expect[1, 4], expect[2, 0] = np.nan, np.inf
            np.testing.assert_array_equal(guarded("pool_l2n", dev(x), kind, p, 1e-6, None), expect, err_msg="%s H*W=%d at %d" % (kind, hw, pos))
            got = guarded("pool_l2n", dev(x), kind, p, 1e-6, 1e-6)
            assert np.isnan(got[1]).all(), (kind, hw, pos)
            np.testing.assert_array_equal(got[0], want_l2n[0])
            multi = guarded("pool_multi", [dev(x), dev(clean)], kind, p, 1e-6)
            np.testing.assert_array_equal(multi, np.stack([expect, want]), err_msg="pool_multi %s H*W=%d at %d" % (kind, hw, pos))


def test_regional_pooling_keeps_nan_in_its_regions():
    """roipool: NaN for the regions that hold the element, in its channel; rmac: the descriptor of its image."""
    from mdir_amd import ops
    h, w = 13, 11
    regs = region_table(h, w)
    clean = TD.dense_maps(2, 70, h * w, seed=4).reshape(2, 70, h, w)
    for i, j in ((0, 0), (h - 1, w - 1), (6, 4)):
        x = clean.copy()
        x[1, 33, i, j] = np.nan
        inside = np.array([r0 <= i < r0 + a and c0 <= j < c0 + b for r0, c0, a, b in regs])
        assert inside[0] and not inside.all()
        for kind, p in (("mac", 1.0), ("spoc", 1.0), ("gem", 3.0), ("gem", 2.92)):
            expect = host(ops.roipool(dev(clean), regs, kind, p, 1e-6))
            expect[1, inside, 33] = np.nan
            np.testing.assert_array_equal(guarded("roipool", dev(x), regs, kind, p, 1e-6), expect, err_msg="%s NaN at %s" % (kind, (i, j)))
        got = guarded("rmac", dev(x), regs, 1e-6)
        assert np.isnan(got[1]).all()
        np.testing.assert_array_equal(got[0], host(ops.rmac(dev(clean), regs, 1e-6))[0])
