"""mdx_pool_l2n_f16 and mdx_pool_multi_f16 (include/mdx.h, "fp16 trunk"): BIT FOR BIT the value the fp32 entry point returns on the
same maps converted to fp32 -- ``torch.equal``, no tolerance; the fp32 entry points are themselves pinned by the golden files and
tests/test_gpu_tail_exact.py.  Random data (not only summation-exact), so a lane that took its elements in another order, or
pieces of another size, shows.

  H*W = 1, 2, 3, 4, 5, 7, 8 (below one piece, one piece, two), 255, 256, 257, 260 (around the 64 lanes x 4 elements of one
  sweep), 768, 1000;  1, 3, 4, 5 planes (four share a workgroup);  GeM with p = 1, 2, 3, 2.5, MAC, SPoC;  maps sliced off the
  8- and 16-byte grids;  pool_multi with S = 1, 2, 3, 8 and another H*W per scale;  a NaN in a MAC plane and in a GeM plane.
One comparison against the float64 oracle (oracle.gem + l2n on the upcast maps) at the suite's rtol 1e-5."""
import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32

HWS = [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 260, 768, 1000]
KINDS = [("gem", 1.0), ("gem", 2.0), ("gem", 3.0), ("gem", 2.5), ("mac", 1.0), ("spoc", 1.0)]


def half_map(shape, seed):
    """ReLU-like random fp16 map: about a third zeros, the rest positive with a few large values."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g).clamp_(min=0) * (1 + 9 * (torch.rand(shape, generator=g) > 0.9))
    return x.half().to(DEV)


def offset_copy(t, off):
    """A contiguous copy of fp16 ``t`` that starts ``off`` elements (2 * off bytes) past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (2 * off) % 16
    return view


def equal_bits(a, b, what):
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, what
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, float((a - b).abs().max()))


@pytest.mark.parametrize("hw", HWS)
def test_pool_l2n_f16_equals_fp32_on_the_upcast_maps(hw):
    from mdir_amd import ops
    for planes in (1, 3, 4, 5):
        x = half_map((1, planes, 1, hw), 100 * hw + planes)
        up = x.float()
        for kind, p in KINDS:
            for l2n_eps in (1e-6, None):
                got = ops.pool_l2n(x, kind, p, 1e-6, l2n_eps)
                equal_bits(got, ops.pool_l2n(up, kind, p, 1e-6, l2n_eps), (hw, planes, kind, p, l2n_eps))
    x = half_map((2, 3, 1, hw), hw)                                  # a batch: [B, C] rows normalised separately
    equal_bits(ops.pool_l2n(x, "gem", 3.0), ops.pool_l2n(x.float(), "gem", 3.0), (hw, "batch"))


@pytest.mark.parametrize("off", [1, 2, 3, 4, 5, 6, 7])
def test_maps_off_the_8_and_16_byte_grids(off):
    """The plane start is any multiple of 2 bytes: odd H*W moves every later plane too.  The bits must not depend on it."""
    from mdir_amd import ops
    for hw in (4, 8, 260, 257, 7):
        x = half_map((2, 5, 1, hw), hw + off)
        moved = offset_copy(x, off)
        for kind, p in KINDS:
            want = ops.pool_l2n(x.float(), kind, p)
            equal_bits(ops.pool_l2n(moved, kind, p), want, (hw, off, kind, p))
            equal_bits(ops.pool_l2n(x, kind, p), want, (hw, 0, kind, p))


@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_pool_multi_f16_equals_fp32_on_the_upcast_maps(S):
    from mdir_amd import ops
    sizes = [(16, 16), (11, 11), (8, 8), (5, 52), (1, 1), (3, 1), (2, 2), (25, 40)][:S]       # H*W = 256, 121, 64, 260, 1, 3, 4, 1000
    for B, C in ((1, 5), (2, 3)):
        maps = [half_map((B, C, h, w), 7 * i + B) for i, (h, w) in enumerate(sizes)]
        ups = [m.float() for m in maps]
        for kind, p in KINDS:
            got = ops.pool_multi(maps, kind, p)
            assert got.shape == (S, B, C)
            equal_bits(got, ops.pool_multi(ups, kind, p), (S, B, C, kind, p))
            for s in range(S):                                       # and the single-map entry point, plane for plane
                equal_bits(got[s], ops.pool_l2n(maps[s], kind, p, 1e-6, None), (S, s, kind, p, "pool_l2n_f16"))
        moved = [offset_copy(m, 1 + i % 7) for i, m in enumerate(maps)]
        equal_bits(ops.pool_multi(moved, "gem", 2.5), ops.pool_multi(ups, "gem", 2.5), (S, "sliced"))


@pytest.mark.parametrize("hw", [8, 7, 260])
def test_nan_in_a_plane(hw):
    """One NaN in one plane: that plane pools to NaN for every kind (MAC's flag, GeM's clamp keeps it), no other plane changes
    -- exactly as the fp32 entry point answers (compared as bits where it is a number, as a NaN mask where not)."""
    from mdir_amd import ops
    x = half_map((1, 6, 1, hw), hw)
    x[0, 2, 0, hw // 2] = float("nan")
    clean = x.clone()
    clean[0, 2] = 0
    for kind, p in KINDS:
        got = ops.pool_l2n(x, kind, p, 1e-6, None)
        want = ops.pool_l2n(x.float(), kind, p, 1e-6, None)
        assert bool(torch.isnan(got[0, 2])) and int(torch.isnan(got).sum()) == 1, (kind, p, got)
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        keep = ~torch.isnan(want)
        assert torch.equal(got[keep].view(torch.int32), want[keep].view(torch.int32))
        other = ops.pool_l2n(clean, kind, p, 1e-6, None)
        assert torch.equal(got[keep].view(torch.int32), other[keep].view(torch.int32)), (kind, p, "another plane changed")
        multi = ops.pool_multi([x, clean], kind, p)
        assert bool(torch.isnan(multi[0, 0, 2])) and int(torch.isnan(multi).sum()) == 1


def test_against_the_float64_oracle():
    from mdir_amd import ops
    x = half_map((2, 7, 9, 13), 3)
    up = x.float().cpu().numpy()
    got = ops.pool_l2n(x, "gem", 2.92).cpu().numpy()
    np.testing.assert_allclose(got, O.l2n(O.gem(up, 2.92)), rtol=1e-5, atol=1e-7)


def test_mixed_and_wrong_dtypes_are_refused():
    from mdir_amd import ops
    a, b = half_map((1, 2, 2, 2), 0), half_map((1, 2, 3, 3), 1)
    for maps in ([a, b.float()], [a.float(), b]):
        with pytest.raises(ValueError, match="share a dtype"):
            ops.pool_multi(maps, "gem")
    with pytest.raises(TypeError):
        ops.pool_l2n(a.to(torch.bfloat16), "gem")
    stats = torch.ones(2, device=DEV)
    with pytest.raises(ValueError, match="residual must be contiguous fp16"):
        ops.bn_act_(a.clone(), stats, stats, residual=a.float())
    with pytest.raises(ValueError, match="residual must be contiguous fp32"):
        ops.bn_act_(a.float(), stats, stats, residual=a)
    with pytest.raises(ValueError, match="contiguous fp32 values"):
        ops.bn_act_(a.clone(), stats.half(), stats.half())
