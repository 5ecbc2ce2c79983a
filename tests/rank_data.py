"""The ranking order restated in numpy, rows built in KEY space, and the tables of cases that pin every route of
mdir_amd/csrc/mdx_rank.hip at its size boundaries (a helper module, imported by test_rank_data_host.py and
test_gpu_rank_boundaries.py).  No GPU, no project kernel and no code of oracle/chain.c is used here: the host test holds this
reference against the oracle, two independent statements of one order.

The order (include/mdx.h, mdx_rank_full): larger score first, -0 == +0, every NaN -- either sign, any payload -- last as ONE
tie class, ties by ascending id.  ``desc_key`` maps a float's bit pattern to a uint32 that ascends in that order; the radix
sorts of the library work on the four bytes of that key, so rows that must exercise a byte (or the skipping of a byte) are
built from keys with ``key_to_float``.

Every table row names the route it is meant to pin.  The GPU test asserts that name against ``ops.rank_route`` /
``ops.topk_route`` before it looks at the result: a threshold that moves fails the row instead of silently changing what the
row covers.  The thresholds restated here (the ``*_EDGE`` constants) are therefore checked, not trusted.
"""
import collections
import zlib

import numpy as np

F32 = np.float32
U32 = np.uint32

NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)        # quiet and signalling, both signs, small and full payloads
NAN_KEY = 0xFFFFFFFF

# the thresholds of the dispatch, as the tables assume them (asserted row by row through the route queries)
SMALL_EDGES = (2048, 4096, 6144, 8192)          # the four instantiations of the one-workgroup sort; 8192 | 8193: SMALL | tiled
SORT_TILE = 4096                                # elements per workgroup of the tiled passes
SEL_CAP = 4096                                  # SELECT: 4 (k + SEL_CAP) <= n; its candidate list has k + SEL_CAP entries
TKS_CAP = 16384                                 # SAMPLED: n >= 16384, k <= 1024, 256 k <= n; at most TKS_CAP candidates in LDS
TKS_SAMPLES = 4096
CNT_TILE = 4096                                 # rows per tile of the counting kernel; 256 labelled items per sweep
RP_ROWS_PER_BLOCK = 16384                       # ranking entries per workgroup of mdx_rank_positions


# ------------------------------------------------------------------------------------------------ the reference

def desc_key(sc):
    """uint32 key of fp32 scores, ascending in ranking order, from the bit pattern alone."""
    u = np.ascontiguousarray(sc, dtype=F32).view(U32).astype(np.int64)
    mag = u & 0x7FFFFFFF
    neg = (u >> 31) == 1
    key = np.where(neg, u, 0x7FFFFFFF - mag)    # positive: larger magnitude first; negative: larger magnitude later
    key = np.where(mag == 0, 0x7FFFFFFF, key)   # -0 is +0
    key = np.where(mag > 0x7F800000, NAN_KEY, key)
    return key.astype(U32)


def key_to_float(key):
    """The inverse of ``desc_key``: fp32 of uint32 keys (NAN_KEY gives the default quiet NaN).  Keys no float has -- below
    +inf's, 0x80000000 (that would be -0), between -inf's and NAN_KEY -- are refused."""
    k = np.asarray(key).astype(np.int64)
    pos = k <= 0x7FFFFFFF
    bad = (pos & (k < 0x007FFFFF)) | (k == 0x80000000) | ((k > 0xFF800000) & (k != NAN_KEY)) | (k < 0) | (k > NAN_KEY)
    if bad.any():
        raise ValueError("no float has key 0x%08X" % int(k[bad].flat[0]))
    u = np.where(pos, 0x7FFFFFFF - k, k)
    u = np.where(k == NAN_KEY, NAN_BITS[0], u)
    return u.astype(U32).view(F32)


def reference_rank(sc):
    """int64 ``[nq, n]``: row q = ids of ``sc[q]`` best to worst."""
    sc = np.ascontiguousarray(sc, dtype=F32)
    return np.argsort(desc_key(sc), axis=1, kind="stable").astype(np.int64)


def reference_topk(sc, k):
    """(ids int64 ``[nq, k]``, scores fp32 ``[nq, k]``): the first k of ``reference_rank`` with the scores as they lie."""
    ids = reference_rank(sc)[:, :k]
    return ids, np.take_along_axis(np.ascontiguousarray(sc, dtype=F32), ids, axis=1)


def reference_positions(sc, id_lists):
    """Per query, int64 positions of the listed ids in ``reference_rank`` (an id listed twice has one position)."""
    sc = np.ascontiguousarray(sc, dtype=F32)
    if max((len(ids) for ids in id_lists), default=0) <= 4:         # short lists: count instead of sorting every row
        key, col = desc_key(sc), np.arange(sc.shape[1])
        return [np.array([np.count_nonzero((key[q] < key[q, i]) | ((key[q] == key[q, i]) & (col < i))) for i in ids], dtype=np.int64)
                for q, ids in enumerate(id_lists)]
    rank = reference_rank(sc)
    out = []
    for q, ids in enumerate(id_lists):
        inv = np.empty(rank.shape[1], dtype=np.int64)
        inv[rank[q]] = np.arange(rank.shape[1])
        out.append(inv[np.asarray(ids, dtype=np.int64)])
    return out


def reference_lookup(ranks, id_lists):
    """Per query, the position of each listed id inside the GIVEN ranking rows ``ranks [nq, n]``, -1 where it is absent."""
    out = []
    for q, ids in enumerate(id_lists):
        where = {int(v): p for p, v in enumerate(ranks[q])}
        out.append(np.array([where.get(int(i), -1) for i in ids], dtype=np.int64))
    return out


# ------------------------------------------------------------------------------------------------ row generators
# each: (rng, nq, n) -> fp32 [nq, n], deterministic in rng

def gauss_ties(rng, nq, n):
    """0.03 N(0, 1) with every fifth column a copy of its right neighbour: runs of ties all over the row."""
    sc = (rng.standard_normal((nq, n)) * 0.03).astype(F32)
    m = sc[:, 1::5].shape[1]
    sc[:, 0:5 * m:5] = sc[:, 1::5]
    return sc


def byte_only(b):
    """Keys that differ in byte ``b`` alone (all 256 values drawn): the LDS sort runs one pass, the tiled passes three idle ones."""
    def gen(rng, nq, n):
        if b == 3:
            base = np.full((nq, 1), 0x007FFFFF, dtype=np.int64)     # the one low part every top byte is a float with
        else:
            base = (0x41 << 24) | rng.integers(0, 1 << 24, (nq, 1))
        base = base & ~(0xFF << (8 * b))
        return key_to_float(base | (rng.integers(0, 256, (nq, n)) << (8 * b)))
    gen.__doc__ = "keys that differ only in byte %d" % b
    return gen


def bytes_0_3(rng, nq, n):
    """Keys that differ only in bytes 0 and 3: the two middle passes are skipped, the outer two are not."""
    top = rng.integers(1, 0xFF, (nq, n))            # 0x01..0xFE: with the fixed middle bytes every such key is a float
    return key_to_float((top << 24) | 0x123400 | rng.integers(0, 256, (nq, n)))


def all_equal(rng, nq, n):
    return np.full((nq, n), 0.25, dtype=F32)


def one_differs(where):
    """All keys equal but for one element at ``where`` (negative: from the end): better in row 0, worse in row 1, NaN in row 2."""
    def gen(rng, nq, n):
        sc = np.full((nq, n), 0.25, dtype=F32)
        for q in range(nq):
            sc[q, where] = (F32(0.5), F32(0.125), np.array(NAN_BITS[q % 4], dtype=U32).view(F32))[q % 3]
        return sc
    return gen


def _all_byte_pool():
    i = np.arange(256, dtype=np.int64)
    # top byte i with a low part that is a float for EVERY i (0x00 needs >= 0x7FFFFF, 0xFF needs <= 0x800000); each of the
    # three lower bytes is a permutation of 0..255
    keys = (i << 24) | (((i + 0x80) & 0xFF) << 16) | (((7 * i + 3) & 0xFF) << 8) | ((13 * i + 5) & 0xFF)
    special = np.array([0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                        0x00000000, 0x80000000] + list(NAN_BITS), dtype=U32).view(F32)
    return np.concatenate([key_to_float(keys), special])


ALL_BYTE_POOL = _all_byte_pool()


def all_bytes(rng, nq, n):
    """Every byte value 0..255 in every key byte, +-inf, the largest finite values, subnormals, both zeros and NaNs of both
    signs and several payloads, at random places; the rest of a longer row repeats them (ties).  A row shorter than the pool
    holds a random part of it."""
    pool = ALL_BYTE_POOL
    out = np.empty((nq, n), dtype=F32)
    for q in range(nq):
        if n <= len(pool):
            row = pool[rng.permutation(len(pool))[:n]]
        else:
            row = np.concatenate([pool, pool[rng.integers(0, len(pool), n - len(pool))]])[rng.permutation(n)]
        out[q] = row
    return out


def ascending(rng, nq, n):
    return np.tile(np.linspace(-1, 1, n, dtype=F32), (nq, 1))


def descending(rng, nq, n):
    return np.tile(np.linspace(1, -1, n, dtype=F32), (nq, 1))


def two_values(rng, nq, n):
    return rng.choice(np.array([-0.5, 0.5], dtype=F32), size=(nq, n))


def concentrated(rng, nq, n):
    """0.3 + 1e-4 N(0, 1): the top key bytes agree, a select needs more than one level."""
    return (0.3 + 1e-4 * rng.standard_normal((nq, n))).astype(F32)


def few_finite(m):
    """All NaN (every payload of NAN_BITS) except ``min(m, n)`` finite scores at random places."""
    def gen(rng, nq, n):
        sc = np.array(NAN_BITS, dtype=U32)[rng.integers(0, 4, (nq, n))].view(F32)
        for q in range(nq):
            at = rng.permutation(n)[:min(m, n)]
            sc[q, at] = (rng.standard_normal(len(at)) * 0.03).astype(F32)
        return sc
    return gen


Kind = collections.namedtuple("Kind", "gen min_n")
KINDS = collections.OrderedDict([
    ("gauss_ties", Kind(gauss_ties, 1)),
    ("byte0", Kind(byte_only(0), 1)), ("byte1", Kind(byte_only(1), 1)), ("byte2", Kind(byte_only(2), 1)), ("byte3", Kind(byte_only(3), 1)),
    ("bytes_0_3", Kind(bytes_0_3, 1)),
    ("all_equal", Kind(all_equal, 1)),
    ("one_differs_0", Kind(one_differs(0), 1)), ("one_differs_4095", Kind(one_differs(4095), 4096)),
    ("one_differs_4096", Kind(one_differs(4096), 4097)), ("one_differs_last", Kind(one_differs(-1), 1)),
    ("all_bytes", Kind(all_bytes, 1)),
    ("ascending", Kind(ascending, 1)), ("descending", Kind(descending, 1)),
    ("two_values", Kind(two_values, 1)),
    ("concentrated", Kind(concentrated, 1)),
    ("few_finite_7", Kind(few_finite(7), 1)), ("few_finite_30", Kind(few_finite(30), 1)), ("few_finite_1500", Kind(few_finite(1500), 1)),
])
ROTATED = [k for k in KINDS if k != "gauss_ties" and not k.startswith("few_finite_") or k == "few_finite_7"]


def make(name, kind, nq, n):
    """The scores of a table row: a function of the row's name alone."""
    sc = KINDS[kind].gen(np.random.default_rng(zlib.crc32(name.encode())), nq, n)
    assert sc.dtype == F32 and sc.shape == (nq, n)
    return np.ascontiguousarray(sc)


# ------------------------------------------------------------------------------------------------ the sampled route's samples

def sampled_positions(n, q):
    """The TKS_SAMPLES columns of query q the SAMPLED route draws its threshold from (one jittered column per stride of
    n // 4096), restated so that a row can be built whose candidate count is known.  A restatement that drifts from the
    kernel cannot make a test pass wrongly: the rows built on it are checked against the reference like any other, they
    would merely stop reaching the in-kernel fallback."""
    stride = n // TKS_SAMPLES
    j = np.arange(TKS_SAMPLES, dtype=np.uint64)
    jitter = (((j * 2654435761) & 0xFFFFFFFF) ^ ((q * 40503 + 0x9E3779B9) & 0xFFFFFFFF)) >> 9
    return (j * stride + jitter % stride).astype(np.int64)


def sampled_threshold_rank(n, k):
    """m: the SAMPLED route's threshold is the m-th best of its samples."""
    expect = max(6 * k, 2048)
    return max(9, -(-expect * TKS_SAMPLES // n))


def sampled_candidates(nq, n, k, ncand):
    """fp32 [nq, n] on which the SAMPLED route collects EXACTLY ``ncand`` candidates per query (m <= ncand): the m best
    samples score 1, ``ncand - m`` unsampled columns score 2 (better than the threshold sample), every other column scores
    between -1 and 0 with ties.  ncand = TKS_CAP fills the candidate buffer to its last slot, TKS_CAP + 1 and ncand < k
    leave the answer to the in-kernel exact fallback."""
    m = sampled_threshold_rank(n, k)
    assert m <= ncand <= n - TKS_SAMPLES
    rng = np.random.default_rng(n + 7 * k + ncand)
    sc = -(rng.integers(1, 1000, (nq, n)) / 1000.0).astype(F32)
    for q in range(nq):
        samples = sampled_positions(n, q)
        sc[q, samples[rng.permutation(TKS_SAMPLES)[:m]]] = 1.0
        free = np.setdiff1d(np.arange(n), samples)
        sc[q, free[rng.permutation(len(free))[:ncand - m]]] = 2.0
    return sc


# ------------------------------------------------------------------------------------------------ the checkers

def _first_mismatch(got, want):
    q, p = np.argwhere(got != want)[0]
    return "first at query %d, position %d: got %s, expected %s" % (q, p, got[q, p], want[q, p])


def check_rank(ranker, sc, case, id_offset=0):
    """``ranker(sc) -> int64 [nq, n]`` must be ``reference_rank(sc) + id_offset``."""
    got = np.asarray(ranker(sc))
    want = reference_rank(sc) + id_offset
    assert got.shape == want.shape and got.dtype == np.int64, "%s: ranking is %s %s" % (case, got.dtype, got.shape)
    assert np.array_equal(got, want), "%s: wrong ranking, %s" % (case, _first_mismatch(got, want))


def check_topk(topk, sc, k, case, id_offset=0):
    """``topk(sc, k) -> (ids [nq, k], scores [nq, k])`` must be the reference's ids (+ id_offset) and the bits of their scores."""
    ids, vals = (np.asarray(a) for a in topk(sc, k))
    want_ids, want_vals = reference_topk(sc, k)
    want_ids = want_ids + id_offset
    assert ids.shape == want_ids.shape and vals.shape == want_vals.shape, "%s: top-k shapes %s %s" % (case, ids.shape, vals.shape)
    assert np.array_equal(ids, want_ids), "%s: wrong top-%d ids, %s" % (case, k, _first_mismatch(ids, want_ids))
    gb, wb = np.ascontiguousarray(vals, dtype=F32).view(U32), want_vals.view(U32)
    assert np.array_equal(gb, wb), "%s: wrong top-%d score bits, %s" % (case, k, _first_mismatch(gb, wb))


def check_positions(positions, sc, id_lists, case):
    """``positions(sc, id_lists) -> flat int64`` (the lists concatenated) must be the ids' places in the reference ranking."""
    got = np.asarray(positions(sc, id_lists)).reshape(-1)
    want = reference_positions(sc, id_lists)
    flat = np.concatenate(want) if want else np.empty(0, np.int64)
    assert got.shape == flat.shape, "%s: %d positions for %d ids" % (case, got.size, flat.size)
    if not np.array_equal(got, flat):
        t = int(np.argwhere(got != flat)[0, 0])
        q = int(np.searchsorted(np.cumsum([len(w) for w in want]), t, side="right"))
        ids = np.concatenate([np.asarray(i, dtype=np.int64).reshape(-1) for i in id_lists])
        raise AssertionError("%s: wrong position, first at entry %d (query %d, id %d): got %d, expected %d"
                             % (case, t, q, ids[t], got[t], flat[t]))


# ------------------------------------------------------------------------------------------------ the tables

BIG_OFFSET = (1 << 32) + 5

RankRow = collections.namedtuple("RankRow", "name n nq kind route id_offset")
RANK_N_SMALL = (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192)
RANK_N_TILED = (8193, 12288, 12289, 20479)
RANK_BOUNDARIES = SMALL_EDGES                   # every kind lies in every band between these (the host test holds it to that)


def _rank_full_table():
    """Per n: gauss_ties and two further kinds in rotation; then, so that EVERY kind lies on each side of every boundary --
    in each band between two neighbouring boundaries, i.e. in each instantiation of the one-workgroup sort and in the tiled
    passes --, the kinds a band still lacks go to the sizes next to its borders."""
    sizes = RANK_N_SMALL + RANK_N_TILED
    kinds = {n: ["gauss_ties"] for n in sizes}
    turn = 0
    for n in sizes:
        while len(kinds[n]) < 3:
            kind = ROTATED[turn % len(ROTATED)]
            turn += 1
            if KINDS[kind].min_n <= n:
                kinds[n].append(kind)
    edges = (0,) + RANK_BOUNDARIES + (sizes[-1],)
    for lo, hi in zip(edges[:-1], edges[1:]):
        band = [n for n in sizes if lo < n <= hi]
        have = {k for n in band for k in kinds[n]}
        lack = [k for k in ROTATED if k not in have]
        for i, kind in enumerate(lack):             # alternately to the sizes next to the band's two borders
            near = [n for n in (band if i % 2 else band[::-1]) if KINDS[kind].min_n <= n]
            if near:
                kinds[near[0]].append(kind)
    rows = []
    for n in sizes:
        for i, kind in enumerate(kinds[n]):
            nq = 3 if n % 2 or i % 2 else 1         # an odd n with nq = 3 starts rows 1 and 2 at 4-byte alignment
            route = "SMALL" if n <= SMALL_EDGES[-1] else "PACKED"
            offset = BIG_OFFSET if kind == "gauss_ties" and n in (4097, 8193) else 0
            rows.append(RankRow("rank_full[%d,%s]" % (n, kind), n, nq, kind, route, offset))
    return rows


RANK_FULL = _rank_full_table()

SegRow = collections.namedtuple("SegRow", "name widths nq route")
SEGMENTS = [SegRow("segments[%s]" % "+".join(map(str, w)) if len(w) < 8 else "segments[%dx%d]" % (len(w), w[0]), tuple(w), nq, route)
            for w, nq, route in (([1] * 32, 3, "SMALL"), ([0, 5, 0, 2043], 1, "SMALL"), ([4096, 4096], 3, "SMALL"),
                                 ([8191, 1], 3, "SMALL"), ([3000, 5193], 3, "PACKED"), ([4095, 1, 4097], 3, "PACKED"))]


def segment_scores(row):
    """fp32 [nq, sum(widths)] for a SegRow: gauss_ties with, on BOTH sides of every block border, a tie value, a zero (-0 left,
    +0 right) and a NaN (payloads differ)."""
    n = sum(row.widths)
    sc = make(row.name, "gauss_ties", row.nq, n)
    nan = np.array(NAN_BITS, dtype=U32).view(F32)
    for border in np.cumsum(row.widths)[:-1]:
        left = [F32(0.125), F32(-0.0), nan[1]]
        right = [nan[2], F32(0.0), F32(0.125)]
        for i, v in enumerate(left):
            if border - 3 + i >= 0:
                sc[:, border - 3 + i] = v
        for i, v in enumerate(right):
            if border + i < n:
                sc[:, border + i] = v
    return sc


def split_blocks(sc, widths):
    """The column blocks of ``sc`` (each contiguous on its own), empty ones included."""
    cuts = np.concatenate([[0], np.cumsum(widths)])
    return [np.ascontiguousarray(sc[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


TopkRow = collections.namedtuple("TopkRow", "name n k nq kind route inner id_offset")
# ``route``: what ops.topk_route must answer.  ``inner``: the ranking route underneath it on the default switches -- of the row
# itself for SORT, of the k + SEL_CAP candidates for SELECT; for SAMPLED, "fallback" where the in-kernel exact select must answer


def _topk_table():
    rows = []

    def add(n, k, route, inner, kind="gauss_ties", nq=None, id_offset=0):
        nq = nq if nq is not None else (3 if n % 2 else 1)
        rows.append(TopkRow("topk[%d,%d,%s]" % (n, k, kind), n, k, nq, kind, route, inner, id_offset))

    for n, k in ((1, 1), (100, 100), (5000, 4999), (8192, 1), (8192, 8192)):                 # trimmed in the one-workgroup sort
        add(n, k, "SORT", "SMALL", id_offset=BIG_OFFSET if (n, k) == (5000, 4999) else 0)
    for n, k in ((8193, 1), (8193, 8193), (8193, 8192), (12289, 4096), (12289, 4097), (16383, 63), (20383, 1000), (16647, 66)):
        add(n, k, "SORT", "PACKED", id_offset=BIG_OFFSET if (n, k) == (12289, 4097) else 0)    # k on and next to a tile border, k = n, n - 1
    add(16648, 66, "SELECT", "SMALL", nq=3)                                                     # the edges of 4 (k + 4096) <= n
    add(20384, 1000, "SELECT", "SMALL", nq=3, id_offset=BIG_OFFSET)
    add(32768, 4096, "SELECT", "SMALL", nq=3)                                                   # 8192 candidates
    add(32772, 4097, "SELECT", "PACKED", nq=3)                                                  # 8193 candidates
    add(40000, 1500, "SELECT", "SMALL", "concentrated", nq=3)                                   # more than one level of the select
    add(40000, 1500, "SELECT", "SMALL", "two_values", nq=3)
    add(40000, 2000, "SELECT", "SMALL", "few_finite_1500", nq=3)                                # real NaN rows before the NaN padding
    add(262143, 1024, "SELECT", "SMALL", nq=3)                                                  # one below 256 k <= n
    add(262400, 1025, "SELECT", "SMALL", nq=1)                                                  # one above k <= 1024
    add(16384, 1, "SAMPLED", "", nq=3)
    add(16384, 64, "SAMPLED", "", nq=3, id_offset=BIG_OFFSET)
    add(20479, 10, "SAMPLED", "", nq=3)
    add(262144, 1024, "SAMPLED", "", nq=3)
    # all-equal scores at and one past the candidate cap's n.  They do NOT fill the candidate buffer: the route orders by (key, id),
    # its threshold is the m-th best SAMPLE by id, and about 2048 columns pass.  SAMPLED_EXACT below holds rows that do meet the cap.
    add(16384, 64, "SAMPLED", "", "all_equal", nq=3)
    add(16385, 64, "SAMPLED", "", "all_equal", nq=3)
    add(20000, 50, "SAMPLED", "", "few_finite_30", nq=3)
    return rows


TOPK = _topk_table()

# SAMPLED rows whose candidate count is constructed (sampled_candidates): the buffer filled to its last slot, one more, fewer than k
SampledRow = collections.namedtuple("SampledRow", "name n k nq ncand route inner")
SAMPLED_EXACT = [SampledRow("topk[262144,1024,candidates=%d]" % c, 262144, 1024, 3, c, "SAMPLED", inner)
                 for c, inner in ((TKS_CAP, ""), (TKS_CAP + 1, "fallback"), (1023, "fallback"))]

PosRow = collections.namedtuple("PosRow", "name n nq lengths")
LIST_LENGTHS = (0, 1, 2, 3, 255, 256, 257, 512, 513)
RANK_OF = [PosRow("rank_of[%d]" % n, n, len(LIST_LENGTHS), tuple(min(l, n) for l in LIST_LENGTHS)) for n in (1, 4095, 4096, 4097, 8193)]
RANK_OF_ALL = PosRow("rank_of[300,arange]", 300, 3, (300, 300, 300))
RANK_OF_WIDE = PosRow("rank_of[8193,nq=2049]", 8193, 2049, (1,) * 2049)       # the grid collapses to one workgroup per query
RANK_COUNT_SHARDS = (PosRow("rank_count[8193,two shards]", 8193, 3, (257, 3, 513)), 4097)      # the cut: not on a tile border
RANK_POSITIONS = [PosRow("rank_positions[%d]" % n, n, 3, (5, 600, 0)) for n in (RP_ROWS_PER_BLOCK - 1, RP_ROWS_PER_BLOCK, RP_ROWS_PER_BLOCK + 1)]


def position_case(row, cut=None):
    """(scores fp32 [nq, n], id lists) of a PosRow: gauss_ties with NaN scores sprinkled in (and, with ``cut``, one tie run
    across that column); list q holds the best row, the worst row, a NaN-scored row, two rows of one tie run and a duplicate,
    as far as its length allows, then random ids (repeats happen)."""
    rng = np.random.default_rng(zlib.crc32(row.name.encode()))
    sc = gauss_ties(rng, row.nq, row.n)
    nan = np.array(NAN_BITS, dtype=U32).view(F32)
    sc[:, ::97] = nan[rng.integers(0, 4, sc[:, ::97].shape)]
    if cut is not None:
        sc[:, cut - 3:cut + 3] = F32(0.01)
    key = desc_key(sc)
    if row.nq > 64:             # one id per query, picked without sorting: the best row, a NaN row, either member of a tie pair
        q = np.arange(row.nq)
        pick = np.stack([np.argmin(key, axis=1), 97 * (q % (row.n // 97)), 5 * (q % (row.n // 5 - 1)), 5 * (q % (row.n // 5 - 1)) + 1])
        return np.ascontiguousarray(sc), [pick[i % 4, i:i + 1].astype(np.int64) for i in q]
    lists = []
    for q, length in enumerate(row.lengths):
        if row is RANK_OF_ALL:
            lists.append((np.arange(row.n), np.arange(row.n)[::-1].copy(), rng.permutation(row.n))[q].astype(np.int64))
            continue
        order = np.argsort(key[q], kind="stable")
        finite = order[key[q][order] != NAN_KEY]
        best, worst, nan_id = order[0], (finite[-1] if len(finite) else order[-1]), order[-1]
        if cut is not None:
            tie = [cut - 1, cut]
        else:
            same = np.flatnonzero(key[q][order][1:] == key[q][order][:-1])
            tie = [order[same[0]], order[same[0] + 1]] if len(same) else [best, best]
        head = [best, worst, nan_id, tie[0], tie[1], tie[0]]
        head = head[q % 6:] + head[:q % 6]
        ids = np.concatenate([np.array(head, dtype=np.int64), rng.integers(0, row.n, max(0, length - len(head)))])[:length]
        lists.append(ids.astype(np.int64))
    return np.ascontiguousarray(sc), lists


def lookup_case(row, extra=3):
    """(ranks int64 [nq, n + extra] -- each row a permutation, of which the first n columns are the ranking --, id lists) of a
    PosRow for mdx_rank_positions: listed are ids at the first and last of the n columns, ids that occur only in the columns
    beyond n and ids that occur nowhere (both: -1)."""
    rng = np.random.default_rng(zlib.crc32(row.name.encode()))
    ld = row.n + extra
    ranks = np.stack([rng.permutation(ld) for _ in range(row.nq)]).astype(np.int64)
    lists = []
    for q, length in enumerate(row.lengths):
        head = [ranks[q, 0], ranks[q, row.n - 1], ranks[q, row.n], ld + 7, ranks[q, row.n // 2]]
        rest = rng.permutation(ld)
        rest = rest[~np.isin(rest, head)][:max(0, length - len(head))]                    # unique within a query
        lists.append(np.concatenate([np.array(head, dtype=np.int64), rest])[:length].astype(np.int64))
    return ranks, lists
