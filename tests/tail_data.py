"""Order-free data for the descriptor tail (a helper module, imported by test_trunk_exact_host.py and
test_gpu_tail_exact.py), and the tail restated in numpy fp32.

The tolerance tests of the pooling / L2N / aggregation kernels allow for the rounding of an fp32 sum whose order (lanes,
16-byte pieces, wave shuffles, workgroup partials) they do not know.  Here every value is a small integer times a power of two
and every partial sum -- of a plane, of a region, of the squares of a row -- is an integer below 2^24 on that grid: an fp32
value.  No sum ever rounds, in any order or grouping, so a reduction has ONE right answer and the only rounded operations left
are the single correctly rounded division / square root at the end, which numpy's fp32 scalars restate.  A dropped element and
a doubled element both change the value: a mismatch is an indexing defect, never rounding noise.

``assert_order_free`` is the condition; tests/test_trunk_exact_host.py checks it for every generator on the CPU.
"""
import numpy as np

F32 = np.float32
LIMIT = 1 << 24

GEM_EPS = 2.0 ** -10            # a clamp on the grid: the zeros of a one-hot plane become 2^-10 and the sum stays exact


def plane_sizes():
    """Every H*W the plane reductions are run at: 1..132 (the lane stride of 64 elements and of 64 16-byte pieces is crossed
    at 64 / 65 and 256 / 260) and the neighbourhoods of 256, 512 and 1024."""
    return list(range(1, 133)) + list(range(252, 261)) + list(range(508, 517)) + list(range(1020, 1029))


def factor(hw):
    """(H, W) with H * W = hw, W > 1 where hw has such a factorisation (H <= W; a prime is 1 x hw)."""
    for h in range(int(np.sqrt(hw)), 0, -1):
        if hw % h == 0:
            return h, hw // h
    raise AssertionError(hw)


def one_hot_maps(b, c, hw):
    """fp32 [b, c, H, W]: plane ``ch`` of image ``i`` is zero except for ``2^((ch + i) % 8)`` at position ``(ch + 3 i) % hw``;
    with ``c >= hw`` every position of the plane is the hot one of some channel."""
    h, w = factor(hw)
    x = np.zeros((b, c, hw), dtype=F32)
    ch = np.arange(c)
    for i in range(b):
        x[i, ch, (ch + 3 * i) % hw] = np.exp2((ch + i) % 8).astype(F32)
    return x.reshape(b, c, h, w)


def dense_maps(b, c, hw, seed=0):
    """fp32 [b, c, H, W] of integers 1..8 (strictly positive: GeM's clamp does not act)."""
    h, w = factor(hw)
    rng = np.random.default_rng(1000 * seed + hw + 7 * c + b)
    return rng.integers(1, 9, (b, c, h, w)).astype(F32)


def int_rows(r, d, seed=0, lo=-4, hi=4):
    """fp32 [r, d] of integers in [lo, hi]; element 0 of every row is nonzero (no all-zero row)."""
    rng = np.random.default_rng(77 * seed + d + 3 * r)
    x = rng.integers(lo, hi + 1, (r, d)).astype(F32)
    x[:, 0] = hi
    return x


def assert_order_free(rows, squares=False):
    """``rows`` [..., n]: every partial sum of the values (``squares``: of their squares) of a row, in any order, is an fp32
    value -- all values are multiples of one power of two u and sum |v| / u < 2^24."""
    v = np.asarray(rows, dtype=np.float64)
    v = v.reshape(-1, v.shape[-1])
    assert np.isfinite(v).all()
    if squares:
        v = v * v
    nz = np.abs(v[v != 0])
    if nz.size == 0:
        return
    mant, ex = np.frexp(nz)
    # the grid: the lowest set bit of any value.  53-bit significands as integers, their trailing zeros counted
    m = (mant * 2.0 ** 53).astype(np.int64)
    low = (m & -m).astype(np.float64)
    u = float(np.min(np.ldexp(low, ex - 53)))
    ints = v / u
    assert (ints == np.rint(ints)).all()
    assert np.abs(ints).sum(axis=1).max() < LIMIT, "a partial sum could round"


# ------------------------------------------------------------------------------------------------ the tail in numpy fp32

def _exact_sum(x, axis):
    """The sum along ``axis`` as fp32.  Computed in float64, where it is exact for order-free data; refuses a sum that is not
    an fp32 value."""
    s = np.asarray(x, dtype=np.float64).sum(axis=axis)
    s32 = s.astype(F32)
    assert np.array_equal(s32.astype(np.float64), s), "the exact sum is not an fp32 value"
    return s32


def mac(x):
    """[B,C,H,W] -> [B,C]: the maximum (no rounding anywhere)."""
    return x.reshape(x.shape[0], x.shape[1], -1).max(axis=2)


def spoc(x):
    """[B,C,H,W] -> [B,C]: the exact sum, then ONE fp32 division by H*W."""
    flat = x.reshape(x.shape[0], x.shape[1], -1)
    return (_exact_sum(flat, 2) / F32(flat.shape[2])).astype(F32)


def gem1(x, eps=GEM_EPS):
    """GeM with p = 1: the mean of ``max(x, eps)``; ``eps`` on the data's grid."""
    return spoc(np.maximum(x, F32(eps)))


def region(x, reg):
    i0, j0, h, w = reg
    return np.ascontiguousarray(x[:, :, i0:i0 + h, j0:j0 + w])


def roipool(x, regions, kind):
    """[B,C,H,W] -> [B,R,C]: ``mac`` / ``spoc`` of every region ``(row0, col0, height, width)``."""
    pool = {"mac": mac, "spoc": spoc}[kind]
    return np.stack([pool(region(x, r)) for r in regions], axis=1).astype(F32)


def l2n_rows(v, bias=None, eps=1e-6):
    """[R,D]: ``(v + bias) / (sqrtf(ss) + eps)`` in fp32 -- the sum of squares is exact, so the square root, the addition of
    eps and the division are the only rounded operations, one each."""
    v = np.asarray(v, dtype=F32)
    if bias is not None:
        v = (v + np.asarray(bias, dtype=F32)).astype(F32)
    ss = _exact_sum(v.astype(np.float64) ** 2, 1)
    den = (np.sqrt(ss, dtype=F32) + F32(eps)).astype(F32)
    return (v / den[:, None]).astype(F32)


def region_sum(m, eps=None):
    """[B,R,C] -> [B,C]: the region vectors (``eps`` not None: L2-normalised as ``l2n_rows``) summed in region order, one
    fp32 addition per region -- a thread of the kernel owns its channels, so the order is the regions'."""
    m = np.asarray(m, dtype=F32)
    out = None
    for r in range(m.shape[1]):
        v = m[:, r] if eps is None else l2n_rows(m[:, r], None, eps)
        out = v.copy() if out is None else (out + v).astype(F32)
    return out


def rmac(x, regions, eps=1e-6):
    return region_sum(roipool(x, regions, "mac"), eps)


def ms_aggregate(vecs):
    """[S,...,D] with S a power of two, msp = 1: the mean over the scales (exact), then ``a / sqrtf(ss)`` with an exact ss."""
    v = np.asarray(vecs, dtype=np.float64)
    a = _exact_sum(v, 0) / F32(v.shape[0])
    a2 = a.reshape(-1, a.shape[-1])
    ss = _exact_sum(a2.astype(np.float64) ** 2, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (a2 / np.sqrt(ss, dtype=F32)[:, None]).astype(F32).reshape(a.shape)
