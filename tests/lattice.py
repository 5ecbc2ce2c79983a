"""Exactly representable data for the similarity paths (a helper module, imported by test_lattice_host.py and
test_gpu_lattice.py).

The tolerance tests of the similarity kernels compare with a float64 product and allow for the rounding of an fp32
accumulation whose order they do not know.  Here the data leave nothing to round: every operand lies on one power-of-two
grid ``u`` (small integers times ``u``) and, for every (query, row) pair,

    sum_k |q_k| |x_k|  <  2^24  (in units of the product grid)

so every partial sum of every subset of the products, in any order and any grouping -- inside an MFMA, across accumulators,
across the pieces of a split-precision operand -- is an integer below 2^24 times the grid: an fp32 value.  Nothing is ever
rounded, and EVERY correct path returns the integer dot product bit for bit: the fp32 chain, the row-major route, both fp16
kernels, split3, split2, the int8 shard, the rescore and the join resolve.  The expected matrix is an integer matrix
product; no oracle of a kernel's internal order is needed.

``Lattice`` is what a generator returns:
    db       fp32 [n, d]   the database rows as handed to the library
    queries  fp32 [nq, d]  the queries as handed to the library (with a centre: the effective queries PLUS the centre)
    center   fp32 [d] or None
    xi, qi   int64         the operands on their grids as the path under test sees them (qi after centring; for the fp16
                           grids after rounding to fp16)
    ux, uq   float         the two grids (powers of two): value = integer * grid
``expected(qi, xi, u)`` with ``u = uq * ux`` is the exact result.  ``assert_exact_in_any_order`` is the condition above; it
is a condition on the DATA, checked for every shape on the CPU (test_lattice_host.py), never a reason to skip or relax a
case: a generator chooses its value range per ``d`` so that it holds.

A zero score is +0 on every path: the chain starts from +0 and adds products (+0 + -0 = +0, x + -x = +0 under round to
nearest; oracle/chain.c gives the same), the MFMA accumulators start from +0, and the int8 epilogue multiplies (float)0 by a
non-negative scale product.  ``expected`` therefore holds +0 and the comparisons are on the bit patterns.
"""
from collections import namedtuple

import numpy as np

LIMIT = 1 << 24                 # integers below 2^24 in magnitude are fp32 values

Lattice = namedtuple("Lattice", ["db", "queries", "center", "xi", "qi", "ux", "uq"])


# ------------------------------------------------------------------------------------------------ the condition, the result

def to_grid(values):
    """(int64 array, u): finite dyadic ``values`` (any float dtype) as integers times the largest power of two ``u`` that
    divides all of them (u = 1 for an all-zero array).  Exact: float64 holds every fp32 / fp16 / bf16 value."""
    v = np.asarray(values, dtype=np.float64)
    assert np.isfinite(v).all(), "to_grid: non-finite value"
    if v.size and np.abs(v).max() < 2.0 ** 52:                      # the usual case, without the bit work: integers, one of them odd
        ints = v.astype(np.int64)
        if (ints == v).all() and (ints & 1).any():
            return ints, 1.0
    nz = v[v != 0]
    if nz.size == 0:
        return np.zeros(v.shape, np.int64), 1.0
    b = np.ascontiguousarray(nz).view(np.int64)                     # the bit patterns: sign | 11-bit exponent | 52-bit fraction
    e = (b >> 52) & 0x7FF
    assert (e > 0).all()                                             # no float64 subnormals (every fp32 value is a float64 normal)
    mant = (b & ((1 << 52) - 1)) | (1 << 52)                         # nz = +-mant * 2^(e - 1075)
    low = mant & -mant                                               # lowest set bit of the significand ...
    tz = (low.astype(np.float64).view(np.int64) >> 52) - 1023        # ... and its position
    ex = int((e - 1075 + tz).min())
    scaled = np.ldexp(v, -ex)
    ints = scaled.astype(np.int64)
    assert (ints.astype(np.float64) == scaled).all() and np.abs(scaled).max() < 2.0 ** 62
    return ints, float(np.ldexp(1.0, ex))


def _int_matmul(a, b_t):
    """int64 ``a @ b_t.T`` of integer matrices through the float64 BLAS: exact, because every partial sum is an integer
    below 2^53 (asserted from the magnitudes); a plain int64 matmul of the 32 k-row shapes takes numpy seconds."""
    a64, b64 = a.astype(np.float64), b_t.astype(np.float64)
    bound = float(np.abs(a64).sum(axis=1).max(initial=0.0)) * float(np.abs(b64).max(initial=0.0))
    assert bound < 2.0 ** 53, "integer product outside float64's exact range"
    return (a64 @ b64.T).astype(np.int64)


def expected(qi, xi, u):
    """fp32 [nq, n]: the exact scores ``(qi @ xi.T) * u`` (int64 operands, ``u`` the product grid).  Refuses a result that is
    not an fp32 value."""
    acc = _int_matmul(qi, xi)
    assert np.abs(acc).max(initial=0) < LIMIT, "the exact result is not an fp32 value"
    out = acc.astype(np.float64) * u
    res = out.astype(np.float32)
    assert (res.astype(np.float64) == out).all(), "the exact result leaves fp32's range"
    return res


def pair_magnitude(q_pieces, x_pieces):
    """max over (query, row) pairs of ``sum_k (sum_p |q_p,k|)(sum_p |x_p,k|)`` in units of the product grid, as a Python int.
    ``q_pieces`` / ``x_pieces``: one array, or a sequence of the pieces a split-precision path makes of the operand (float
    dyadic values or integers): every piece product of every pair is then a multiple of the product grid, and their
    magnitudes add up to what this returns."""
    def total(pieces):
        if isinstance(pieces, np.ndarray):
            pieces = [pieces]
        stack = np.stack([np.asarray(p, dtype=np.float64) for p in pieces])
        ints, _ = to_grid(stack)
        return np.abs(ints).sum(axis=0)
    tq, tx = total(q_pieces), total(x_pieces)
    if tq.size == 0 or tx.size == 0:
        return 0
    return int(_int_matmul(tq, tx).max())


def assert_exact_in_any_order(q_pieces, x_pieces):
    """The condition of this module: below 2^24, so that no order or grouping of the products can round.  Returns the value."""
    worst = pair_magnitude(q_pieces, x_pieces)
    assert worst < LIMIT, "sum_k |q_k||x_k| = %d >= 2^24: some order of the products may round" % worst
    return worst


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ generators

def _special_rows(rng, ints, hot, period=7):
    """Zero rows, one-hot rows and duplicate rows mixed into integer rows (in place): one of each in every ``period`` rows.
    ``hot``: the value of a one-hot row's entry.  Row 0 stays an ordinary row."""
    n, d = ints.shape
    for i in range(1, n):
        kind = i % period
        if kind == 3:
            ints[i] = 0
        elif kind == 5:
            ints[i] = 0
            ints[i, rng.integers(0, d)] = hot if i % 2 else -hot
        elif kind == 6:
            ints[i] = ints[i // 2]
    if n > 20:                                               # a few more, at random places
        for i in rng.integers(1, n, size=max(1, n // 50)):
            ints[i] = ints[rng.integers(0, i)]
    return ints


def _negative_zeros(rng, a32):
    """-0 in place of about a quarter of the zero elements of an fp32 array (in place): the value is the same, the bits differ."""
    mask = (a32 == 0) & (rng.random(a32.shape) < 0.25)
    a32[mask] = np.float32(-0.0)
    return a32


def _common_ints(rng, rows, d, amp, period):
    ints = rng.integers(-amp, amp + 1, size=(rows, d), dtype=np.int64)
    ints[rng.random((rows, d)) < 0.3] = 0
    hot = rng.integers(0, d, size=rows)                      # every nonzero row: one entry of exactly +-127
    ints[np.arange(rows), hot] = np.where(rng.random(rows) < 0.5, 127, -127)
    return _special_rows(rng, ints, 127, period)             # zero, one-hot (+-127) and duplicate rows keep the rule


def common(n, d, nq, seed=0, centred=False, amp=15, period=7):
    """The grid every path shares: integers, |x| <= ``amp`` <= 15, and one entry of exactly +-127 in every nonzero row, so that
    the int8 scale of the row is 127 / 127 = 1 and its codes are its values (include/mdx.h, MDX_I8).  ``centred``: an integer
    centre with |c| <= 3 is added to the queries; the effective queries (``qi``) keep the +-127 rule.  ``amp=1`` leaves about a
    hundred distinct scores (the ranking tests); ``period``: one zero, one one-hot and one duplicate row in every so many."""
    rng = np.random.default_rng([seed, n, d, nq, int(centred), amp, period])
    xi = _common_ints(rng, n, d, amp, period)
    qi = _common_ints(rng, nq, d, amp, period)
    db = _negative_zeros(rng, xi.astype(np.float32))
    if centred:
        ci = rng.integers(-3, 4, size=d, dtype=np.int64)
        center = ci.astype(np.float32)
        queries = (qi + ci[None, :]).astype(np.float32)
    else:
        center = None
        queries = _negative_zeros(rng, qi.astype(np.float32))
    return Lattice(db, queries, center, xi, qi, 1.0, 1.0)


def _f16_lattice(db, queries):
    """The Lattice of fp32 operands as an fp16 shard sees them: rounded to fp16 (nearest even), then put on their grids."""
    with np.errstate(over="ignore"):
        xi, ux = to_grid(db.astype(np.float16).astype(np.float64))
        qi, uq = to_grid(queries.astype(np.float16).astype(np.float64))
    return Lattice(np.ascontiguousarray(db, np.float32), np.ascontiguousarray(queries, np.float32), None, xi, qi, ux, uq)


def f16_wide(n, d, nq, seed=0, swap=False, db_exp=0, q_exp=0, top=False):
    """fp16's whole significand: the database holds integers |x| <= 2047 (11 bits) times 2^``db_exp``, the queries integers
    |q| <= 3 times 2^``q_exp``; ``swap`` exchanges the roles.  2^-24 puts an operand on fp16's subnormal grid (the products stay
    fp32 normals); 2^-34 puts it BELOW that grid, so the shard holds its rounding to 0, 2^-24 or 2^-23 (ties to even); ``top``
    with ``db_exp=5`` plants +-65504, fp16's largest value.  ``xi`` / ``qi`` are the fp16 values of the operands."""
    rng = np.random.default_rng([seed, n, d, nq, int(swap), db_exp + 64, q_exp + 64, int(top)])
    rows_w, rows_s = (nq, n) if swap else (n, nq)
    wide = rng.integers(-2047, 2048, size=(rows_w, d), dtype=np.int64)
    wide[rng.random((rows_w, d)) < 0.2] = 0
    _special_rows(rng, wide, 2047)
    if top:
        wide[0, rng.integers(0, d)] = 2047
        wide[rows_w - 1, rng.integers(0, d)] = -2047
    small = rng.integers(-3, 4, size=(rows_s, d), dtype=np.int64)
    _special_rows(rng, small, 3)
    we, se = (q_exp, db_exp) if swap else (db_exp, q_exp)
    wide32 = _negative_zeros(rng, np.ldexp(wide.astype(np.float64), we).astype(np.float32))
    small32 = _negative_zeros(rng, np.ldexp(small.astype(np.float64), se).astype(np.float32))
    return _f16_lattice(small32, wide32) if swap else _f16_lattice(wide32, small32)


F16_ROUND_BANDS = ("halfway", "overflow", "tiny")


def _f16_round_values(band):
    """fp32 values that are NOT fp16 values, for one band of fp16's range (one band = one grid after rounding)."""
    f32 = np.float32
    vals = []
    if band == "halfway":
        # fp16's binade [1024, 2048): ulp 1.  k + 0.5 is exactly half way; k even and odd: both parities of the lower neighbour
        for k in (1024, 1025, 1026, 1531, 1532, 2045, 2046, 2047):
            half = f32(k + 0.5)
            vals += [half, np.nextafter(half, f32(0)), np.nextafter(half, f32(4096))]
        for k in (512, 513, 700, 701, 1023):                 # binade [512, 1024): ulp 1/2, half way at k + 0.25
            half = f32(k + 0.25)
            vals += [half, np.nextafter(half, f32(0)), np.nextafter(half, f32(4096))]
    elif band == "overflow":
        # the last binade, ulp 32: 65519.996 is the largest fp32 value that still rounds to 65504 (65520 rounds to infinity:
        # that side is the non-finite test's); half-way points with an even and an odd lower neighbour
        vals += [np.nextafter(f32(65520.0), f32(0)), f32(65504.0), f32(65505.0), f32(65488.0), np.nextafter(f32(65488.0), f32(0)),
                 np.nextafter(f32(65488.0), f32(70000)), f32(65456.0), np.nextafter(f32(65456.0), f32(0)),
                 np.nextafter(f32(65456.0), f32(70000)), f32(32784.0), f32(32816.0)]
    else:
        # under fp16's subnormal grid 2^-24: 2^-25 is half way between 0 and 2^-24 (to even: 0), anything above it rounds up
        t = 2.0 ** -24
        vals += [f32(t / 2), np.nextafter(f32(t / 2), f32(1)), np.nextafter(f32(t / 2), f32(0)), f32(t / 4), f32(t / 1024), f32(1.5 * t),
                 np.nextafter(f32(1.5 * t), f32(0)), np.nextafter(f32(1.5 * t), f32(1)), f32(2.5 * t), f32(3.5 * t), f32(1022.5 * t),
                 f32(1023.5 * t), f32(2.0 ** -126), f32(1e-41)]
    vals = np.array(vals, dtype=np.float32)
    return np.concatenate([vals, -vals])


def f16_round(n, d, nq, band, seed=0, swap=False):
    """fp32 inputs that an fp16 shard has to ROUND: exact half-way cases with both parities of the lower neighbour and both
    signs, the fp32 neighbours of a half-way point on either side, the largest value under the overflow threshold, values
    below 2^-25.  The other operand holds integers |q| <= 3.  Expected: the integer product of ``astype(np.float16)`` of the
    operands (IEEE round to nearest even), which is what ``xi`` / ``qi`` hold."""
    assert band in F16_ROUND_BANDS
    rng = np.random.default_rng([seed, n, d, nq, F16_ROUND_BANDS.index(band), int(swap)])
    rows_w, rows_s = (nq, n) if swap else (n, nq)
    table = _f16_round_values(band)
    wide32 = table[rng.integers(0, table.size, size=(rows_w, d))]
    wide32[rng.random((rows_w, d)) < 0.2] = 0
    flat = wide32.reshape(-1)
    flat[:min(table.size, flat.size)] = table[:flat.size]     # every value of the table occurs (where the matrix has room)
    small = rng.integers(-3, 4, size=(rows_s, d), dtype=np.int64)
    _special_rows(rng, small, 3)
    small32 = _negative_zeros(rng, small.astype(np.float32))
    return _f16_lattice(small32, wide32) if swap else _f16_lattice(wide32, small32)


def _two_piece(n, d, nq, seed, swap, shift, tag):
    """One operand ``a + b * 2^-shift`` (|a| <= amax with at least one |a| = amax, |b| <= 7), the other small integers |q| <= 3."""
    rng = np.random.default_rng([seed, n, d, nq, int(swap), shift, tag])
    amax = 15 if d << shift <= 1 << 19 else 3                 # keeps sum (|h| + |m|)(|q|) below 2^24 up to d = 2048
    rows_w, rows_s = (nq, n) if swap else (n, nq)
    a = rng.integers(-amax, amax + 1, size=(rows_w, d), dtype=np.int64)
    b = rng.integers(-7, 8, size=(rows_w, d), dtype=np.int64)
    mask = rng.random((rows_w, d)) < 0.25
    a[mask], b[mask] = 0, 0
    wide = a * (1 << shift) + b
    _special_rows(rng, wide, amax * (1 << shift) + 5)
    wide[0, rng.integers(0, d)] = amax * (1 << shift) + 3      # the matrix' largest magnitude lies in amax's binade
    small = rng.integers(-3, 4, size=(rows_s, d), dtype=np.int64)
    _special_rows(rng, small, 3)
    small[0, rng.integers(0, d)] = 3
    wide32 = _negative_zeros(rng, np.ldexp(wide.astype(np.float64), -shift).astype(np.float32))
    small32 = _negative_zeros(rng, small.astype(np.float32))
    if swap:
        return Lattice(small32, wide32, None, small, wide, 1.0, 2.0 ** -shift)
    return Lattice(wide32, small32, None, wide, small, 2.0 ** -shift, 1.0)


def split3_two_piece(n, d, nq, seed=0, swap=False):
    """MDX_F32_SPLIT3 with two live pieces: database ``x = a + b * 2^-8`` (up to 12 significant bits: the bf16 pieces h and m
    hold all of it, l = 0; wherever a and b are both nonzero, h and m both are), queries small integers (one piece).  Every
    piece product is kept by the mode, so the exact result is the integer product.  ``swap``: the queries are the two-piece
    operand."""
    return _two_piece(n, d, nq, seed, swap, 8, 3)


def split2_two_piece(n, d, nq, seed=0, swap=False):
    """MDX_F32_SPLIT2 with two live pieces: ``x = a + b * 2^-11``: after the block scaling the fp16 piece h holds the leading
    11 bits and m the rest, exactly.  The other operand is small integers -- one piece, so the ``mm`` product the mode drops by
    definition is zero and the exact result is the integer product."""
    return _two_piece(n, d, nq, seed, swap, 11, 2)


def split3_pieces(a32):
    """The bf16 pieces (h, m, l) of the host restatement (oracle.oracle.split3_bf16), float64."""
    from oracle import oracle as O
    return [p.astype(np.float64) for p in O.split3_bf16(a32)]


def split2_pieces(a32):
    """The fp16 pieces of the host restatement of MDX_F32_SPLIT2 (oracle.oracle.scores_split2: block scale, round toward
    zero) as VALUES of the unscaled operand: (h / S, m / (2048 S)), float64."""
    from oracle import oracle as O
    s = O.split2_scale(a32)
    X = np.asarray(a32, dtype=np.float32).astype(np.float64) * s
    h = O._fp16_toward_zero(X)
    m = O._fp16_toward_zero((X - h) * 2048.0)
    return [h / s, m / (2048.0 * s)]


# ------------------------------------------------------------------------------------------------ the shapes of the GPU table

# (n, d, nq).  Branches of mdir_amd/csrc/mdx_index.hip reached (RT = round_up(ceil(n / 16), 8) row tiles; QT = ceil(nq / 16)):
#   RT < 2048 (n <= 32 640): 64-row workgroups (R = 1); above: 128-row workgroups (R = 2) -- 32 640 / 32 641 is the switch
#   of an index, 32 752 / 32 753 that of the row-major route (its RT is not rounded up); the issue's 32 767 .. 32 895 lie above both
#   fp32, R = 1, 1 < QT <= 8 and RT / 4 * QT <= 1024: one query tile per workgroup (launch_scores_lc<1, 1> with grid.y = QT);
#   above that product (8192 / 8193 rows at QT = 8): launch_group -> launch_tiles<QT, 1>
#   fp32, R = 2, QT >= 2 and <= 8 queries in the last tile: launch_group takes launch_scores_lc<QT - 1, 2, MmaF32, 1> (the
#   leftover tile); else launch_tiles<QT, 2>
#   QT = 9: a launch of 8 tiles and one of 1; QT = 17: two full groups in ONE launch (grid.y = 2) and a launch of 1 (for_query_groups)
#   fp16: round_up(d, 64) % 128 == 0 -> register-streaming kernel, == 64 -> ring kernel; int8: launch_stream<QT, R, true>, R as above
#   split3 / split2: up to 5 query tiles per workgroup, more = passes; 128-row consumers below 65 536 rows (SPLIT_TRIPLES has the other)
TRIPLES = [
    # 64-row workgroups, every tail of rows, queries and k
    (1, 1, 1), (15, 8, 8), (16, 63, 9), (17, 64, 16), (63, 65, 17), (64, 100, 112), (65, 128, 113), (127, 129, 128),
    (128, 192, 129), (129, 256, 257), (129, 2048, 17), (1, 2048, 129), (127, 2048, 113), (17, 1, 257), (64, 8, 128),
    (128, 64, 1), (65, 63, 16), (8192, 64, 128), (8193, 64, 128), (16401, 65, 50),
    # the switch to 128-row workgroups and its tail; every query-tile count with and without the <= 8-query leftover tile
    (32640, 64, 128), (32641, 100, 112), (32752, 64, 17), (32753, 64, 17),
    (32767, 64, 17), (32768, 128, 113), (32769, 65, 9), (32895, 192, 129), (32768, 63, 257), (32769, 129, 16),
    (32767, 8, 1), (32895, 1, 8), (32768, 192, 40), (32769, 128, 57), (32767, 100, 72), (32768, 64, 89), (32895, 128, 104),
    (32767, 128, 25), (32768, 100, 41), (32769, 64, 56), (32895, 65, 73), (32768, 8, 88),
]
R2_TRIPLES = [t for t in TRIPLES if t[0] > 32640]
# the split modes switch their consumers at RT = 4096 (65 536 rows)
SPLIT_TRIPLES = TRIPLES + [(65521, 64, 17), (65537, 100, 129)]
# the tail shapes of the fp16 contract: both kernels (d_pad % 128 == 0 / == 64), both workgroup sizes, tails everywhere
F16_TRIPLES = [(17, 63, 9), (65, 100, 17), (127, 192, 113), (129, 256, 129), (63, 2048, 16), (32769, 100, 17), (32895, 192, 9)]
