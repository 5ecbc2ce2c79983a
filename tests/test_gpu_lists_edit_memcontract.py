"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the two entry points that edit the
lists of the inverted file: mdx_lists_merge and mdx_lists_compact.  Several shapes each, so that the leftovers of the largest call are
the stale pre-fill of the smaller ones; every caller pointer at the smallest alignment include/mdx_lists_edit.h allows -- 1 byte for
the payload rows (off the 16-byte grid: the byte path, whatever the width; on it: 16-byte pieces where the width and the strides are
multiples of 16, dwords where of 4; the same bits), 8 for the int64 vectors.  Row strides above the width on either side of a call: the
bytes between the rows of an output must stay as they were, which every run checks itself.  The oracle is the restatement
(tests/lists_edit_restatement.py), bit for bit."""
import numpy as np
import pytest
import torch

import lists_edit_restatement as LR
import memguard
from test_gpu_memcontract import Lazy, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = []


def add(name, made, larger=None, **kw):
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), larger=larger, **kw)
    case.release = made.release
    CASES.append(case)
    return case


def structure(rng, sizes, width, first_id=0):
    """(rows uint8 [m, width], members int64 [m] ascending inside a list, offsets int64 [K + 1]) with lists of ``sizes``."""
    m = int(sum(sizes))
    offsets = np.zeros(len(sizes) + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    members = np.empty(m, np.int64)
    ids = first_id + rng.permutation(m)
    for l in range(len(sizes)):
        members[offsets[l]:offsets[l + 1]] = np.sort(ids[offsets[l]:offsets[l + 1]])
    return rng.integers(0, 256, (m, width)).astype(np.uint8), members, offsets


def strided(env, name, rows, ld):
    """``rows`` uploaded at the row stride ``ld`` (random bytes between the rows): the [m, width] view of it."""
    if ld is None:
        return env.put(name, rows)
    wide = np.random.default_rng(ld).integers(0, 256, (rows.shape[0], ld)).astype(np.uint8)
    wide[:, :rows.shape[1]] = rows
    return env.put(name, wide)[:, :rows.shape[1]]


def call_into(env, m, width, out_ld, call):
    """``call(out_rows)`` with its rows going to a guarded block of the row stride ``out_ld`` (None: the wrapper's own, contiguous);
    the bytes between the rows are what they were."""
    if out_ld is None:
        return call(None)
    block = env.empty("out_rows", (m, out_ld), torch.uint8)
    before = block[:, width:].clone()
    rows, members, offsets = call(block[:, :width])
    assert rows.data_ptr() == block.data_ptr() and torch.equal(block[:, width:], before)
    return rows, members, offsets


def _merge(width, a_sizes, b_sizes, strides=(None, None, None), beyond=False):
    def make():
        rng = np.random.default_rng(width + sum(a_sizes))
        a = structure(rng, a_sizes, width)
        b = structure(rng, b_sizes, width, first_id=sum(a_sizes))
        if beyond:                                                         # a last offset beyond m: clamped
            a[2][-1] += 7
            b[2][-1] += 1 << 40
        want = LR.merge(*a, *b)
        assert len(want[1]) == sum(a_sizes) + sum(b_sizes) and want[2][-1] == len(want[1])

        def run(env):
            a_t = (strided(env, "a_rows", a[0], strides[0]), env.put("a_members", a[1]), env.put("a_offsets", a[2]))
            b_t = (strided(env, "b_rows", b[0], strides[1]), env.put("b_members", b[1]), env.put("b_offsets", b[2]))
            rows, members, offsets = call_into(env, len(want[1]), width, strides[2], lambda out: env.ops.lists_merge(*a_t, *b_t, out_rows=out))
            return {"rows": rows.contiguous(), "members": members, "offsets": offsets}

        def verify(o):
            for name, w in zip(("rows", "members", "offsets"), want):
                bits_equal(o[name], w, name)
        return [(run, verify)]
    return make


def keep_flags(mode, sizes, rng):
    m = sum(sizes)
    keep = np.zeros(m, bool)
    if mode == "alternate":
        keep[::2] = True
    elif mode == "first":
        keep[0] = True
    elif mode == "last":
        keep[-1] = True
    elif mode == "random":
        keep[:] = rng.random(m) < 0.6
    else:                                                                  # per list: nothing, everything, every second, ...
        start = 0
        for l, s in enumerate(sizes):
            keep[start:start + s] = (False, True, np.arange(s) % 2 == 1)[l % 3]
            start += s
    return keep


def _compact(width, sizes, mode, strides=(None, None), known_total=True, beyond=False):
    def make():
        rng = np.random.default_rng(width + sum(sizes))
        rows, members, offsets = structure(rng, sizes, width)
        if beyond:
            offsets[-1] += 9
        kept = LR.prefix(keep_flags(mode, sizes, rng))
        want = LR.compact(rows, members, offsets, kept)
        total = int(kept[-1])
        assert 1 <= total == len(want[1]) < len(members)

        def run(env):
            given = (strided(env, "rows", rows, strides[0]), env.put("members", members), env.put("offsets", offsets), env.put("kept", kept))
            out, out_members, out_offsets = call_into(env, total, width, strides[1], lambda o: env.ops.lists_compact(
                *given, total=total if known_total else None, out_rows=o))
            return {"rows": out.contiguous(), "members": out_members, "offsets": out_offsets}

        def verify(o):
            for name, w in zip(("rows", "members", "offsets"), want):
                bits_equal(o[name], w, name)
        return [(run, verify)]
    return make


# K = 5: an empty list on either side, a list only b populates, lists around and above a wave; then lists longer than the span of a
# workgroup (1024 pieces: 256 rows of 64 bytes, 341 of 3) with a total that is no multiple of it
A5, B5 = (0, 3, 0, 70, 1), (2, 0, 0, 5, 300)
LONG_A, LONG_B = (700, 0, 1), (0, 300, 513)
# entry point -> (builder, the arguments of the largest shape and of the smaller ones)
STAGES = {
    "lists_merge": (_merge, (64, LONG_A, LONG_B), (
        (1, (1,), (1,)),
        (3, A5, B5, (5, 8, 7)),                                            # the byte path, three different strides
        (20, A5, B5),                                                      # the dword path
        (16, A5, B5), (64, A5, B5, (64, 80, 64)), (128, A5, B5),           # 16-byte pieces; off the grid in the alignment runs
        (3, LONG_A, LONG_B),
        (16, (0,) * 5, B5),                                                # ma = 0
        (16, A5, (0,) * 5, (None, None, 48)),                              # mb = 0
        (20, A5, B5, (24, None, None), True),                              # last offsets beyond m
    )),
    "lists_compact": (_compact, (64, (700, 0, 513, 300), "random"), (
        (16, (3, 70, 9, 300, 1, 64), "lists"),                             # lists with nothing, everything, every second position kept
        (3, (3, 70, 9), "alternate", (5, 7)),
        (20, (3, 70, 9), "alternate", (None, None), False),                # the total read back by the wrapper
        (16, (5, 66, 0), "first"),                                         # a total of one kept row
        (128, (5, 66, 0, 2), "last", (None, 144)),
        (1, (9,), "alternate"),                                            # K = 1
        (64, (40, 300), "lists", (None, None), True, True),                # a last offset beyond m
    )),
}

for _entry, (_builder, _big_args, _smaller) in STAGES.items():
    _big = add("%s[big]" % _entry, Lazy(_builder(*_big_args)))
    for _i, _args in enumerate(_smaller):
        _small = add("%s[small%d]" % (_entry, _i), Lazy(_builder(*_args)), larger=_big)
        if _big.larger is None:
            _big.larger = _small

# entry point -> its cases.  The census of tests/test_memguard_host.py does not see these entry points (their prototypes are in
# include/mdx_lists_edit.h); tests/test_lists_edit_host.py::test_every_launching_entry_point_has_memory_contract_cases reads this table.
COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")] for entry in STAGES}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_memory_contract(case):
    from mdir_amd import ops
    log = []
    assert case.larger is not None and case.larger is not case
    try:
        memguard.run_contract(ops, case, DEV, alignment_run=True, log=log.append)
        assert "stale" in log and any(step.startswith("align ") and step.endswith("same bits") for step in log), log
    finally:
        case.release()
        case.larger.release()
        print("%s: %s" % (case.name, "; ".join(log)))
