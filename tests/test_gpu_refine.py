"""ops.refine_i8 on the device (include/mdx_refine.h), bit for bit against the restatement (tests/refine_restatement.py): every d at
which the kernel takes another path -- d_pad = 64, the 1024 columns a lane's loads cover in one instruction, the two, three and more
than four slices of a row, the 16-byte and the byte loads of the query --, every S around a workgroup's 64 entries and the sort's
powers of two, ids and positions that are not there, a NaN scale, a zero row, query codes off the 16-byte grid, the output on top of
the input, lattice data with many tied scores, and the independence of a query's row from the batch."""
import ctypes

import numpy as np
import pytest
import torch

import ivf_restatement as IR
import lattice
import lists_i8_restatement as LI
import refine_restatement as RR
from test_gpu_ivf import dev, host
from test_gpu_refine_memcontract import problem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
# d_pad = 64 (1, 15, 16, 63, 64) and 128 (65); the last lanes of one slice (1008, 1024) and the first of the second (1040); two slices
# full (2048) and a third begun (2049, which takes the kernel of four); 4100: more than four slices, the query loaded slice by slice
DIMS = [1, 15, 16, 63, 64, 65, 1008, 1024, 1040, 2048, 2049, 4100]
SHORTLISTS = [1, 63, 64, 65, 257, 4096]
N, M = 300, 200                                       # m < n: a third of the ids is not stored


def off_grid(t, by=1):
    """A copy of the int8 tensor ``t`` at an address that is ``by`` modulo 16."""
    raw = torch.empty(t.numel() + 32, dtype=torch.int8, device=t.device)
    at = (by - raw.data_ptr()) % 16
    out = raw[at:at + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == by and out.is_contiguous()
    return out


def run(given, d):
    from mdir_amd import ops
    t = [dev(a) for a in given]
    return tuple(host(x) for x in ops.refine_i8(t[0], t[1], d, *t[2:]))


@pytest.mark.parametrize("d", DIMS)
def test_refine_equals_the_restatement(d):
    for s in SHORTLISTS:
        for nq in (1, 3):
            given = problem(7 * s + nq, nq, s, M, N, d)
            codes, scales, where, qcodes, qscales, ids = given
            if s >= 8:                                                      # the premise: every special value is among the inputs
                assert (where == -1).any() and (where == M).any() and (where == 1 << 40).any() and np.isnan(scales).any() and (scales == 0).any()
                assert all((ids == v).any() for v in (-1, N, N + 5)) and (ids[:, -1] == ids[:, -2]).all()
            want_ids, want = RR.refine(codes, scales, d, where, qcodes, qscales, ids)
            got_ids, got = run(given, d)
            IR.same_bits(got_ids, want_ids), IR.same_bits(got, want)
            if s == 4096:
                assert np.isnan(got).any() and (got == 0).any() and np.isfinite(got).sum() > nq * s // 2


@pytest.mark.parametrize("d", [16, 64, 1024, 1040, 2048])
def test_query_codes_off_the_16_byte_grid_give_the_same_bits(d):
    from mdir_amd import ops
    given = problem(d, 3, 65, M, N, d)
    want_ids, want = RR.refine(given[0], given[1], d, *given[2:])
    t = [dev(a) for a in given]
    assert t[3].data_ptr() % 16 == 0
    for by in (1, 8, 15):
        got_ids, got = ops.refine_i8(t[0], t[1], d, t[2], off_grid(t[3], by), t[4], t[5])
        IR.same_bits(host(got_ids), want_ids), IR.same_bits(host(got), want)


@pytest.mark.parametrize("s", [1, 65, 4096])
def test_the_output_may_lie_on_the_input(s):
    """out_ids == ids through the C ABI: the sort holds all of a query's ids in LDS before it writes one."""
    from mdir_amd import _lib, ops
    d, nq = 70, 3
    given = problem(s, nq, s, M, N, d)
    want_ids, want = RR.refine(given[0], given[1], d, *given[2:])
    codes, scales, where, qcodes, qscales, ids = (dev(a) for a in given)
    h = _lib.lib()
    ws = torch.empty(h.mdx_refine_i8_workspace(nq, s), dtype=torch.uint8, device=DEV)
    out = torch.empty((nq, s), dtype=torch.float32, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    _lib.check(h.mdx_refine_i8(p(codes), p(scales), M, d, p(where), N, p(qcodes), p(qscales), nq, p(ids), s, p(ids), p(out), p(ws), ws.numel(),
                               ops._stream()), "mdx_refine_i8")
    IR.same_bits(host(ids), want_ids), IR.same_bits(host(out), want)


@pytest.mark.parametrize("d", [24, 1040])
def test_lattice_scores_are_the_integer_products_and_ties_ascend_in_id(d):
    """tests/lattice.common with amp = 1: every nonzero row holds a +-127, so its scale is 1 and its codes are its values; the int8
    score is the integer dot product, exactly, and about a hundred distinct values are shared by the whole shortlist."""
    from mdir_amd import ops
    n, nq = 500, 4
    lat = lattice.common(n, d, nq, seed=3, amp=1)
    rng = np.random.default_rng(d)
    members = np.sort(rng.permutation(n)[:n - 50]).astype(np.int64)
    codes, scales = ops.lists_i8_encode(dev(lat.db), dev(members))
    qcodes, qscales = ops.quantize_i8(dev(lat.queries))
    where = RR.where_of(members, n)
    ids = np.stack([rng.permutation(n) for _ in range(nq)]).astype(np.int64)
    got_ids, got = (host(x) for x in ops.refine_i8(codes, scales, d, dev(where), qcodes, qscales, dev(ids)))
    exact = lattice.expected(lat.qi, lat.xi, 1.0)
    tied = 0
    for q in range(nq):
        stored = where[got_ids[q]] >= 0
        assert stored.sum() == len(members) and stored[:len(members)].all() and np.isnan(got[q][~stored]).all()
        assert sorted(got_ids[q].tolist()) == list(range(n))
        IR.same_bits(got[q][stored] + F32(0), exact[q][got_ids[q][stored]] + F32(0))          # -0 == +0: a zero row scores 0 * 0
        head = got[q][:len(members)]
        assert (head[:-1] >= head[1:]).all()
        same = np.flatnonzero(head[1:] == head[:-1])
        assert (got_ids[q][same] < got_ids[q][same + 1]).all()
        tied += len(same)
        tail = got_ids[q][len(members):]                                    # the ids that are not stored: NaN, in ascending id
        assert (tail[:-1] < tail[1:]).all()
    assert tied > nq * len(members) // 2
    want_ids, want = RR.refine(host(codes), host(scales), d, where, host(qcodes), host(qscales), ids)
    IR.same_bits(got_ids, want_ids), IR.same_bits(got, want)


@pytest.mark.parametrize("d,s", [(64, 65), (1040, 257)])
def test_a_query_does_not_depend_on_the_batch(d, s):
    from mdir_amd import ops
    nq = 3
    given = problem(d + s, nq, s, M, N, d)
    t = [dev(a) for a in given]
    all_ids, all_sc = (host(x) for x in ops.refine_i8(t[0], t[1], d, *t[2:]))
    for q in range(nq):
        one_ids, one_sc = ops.refine_i8(t[0], t[1], d, t[2], t[3][q:q + 1].contiguous(), t[4][q:q + 1].contiguous(), t[5][q:q + 1].contiguous())
        IR.same_bits(host(one_ids)[0], all_ids[q]), IR.same_bits(host(one_sc)[0], all_sc[q])
    # and not on the order of the queries
    back = [2, 0, 1]
    swapped = ops.refine_i8(t[0], t[1], d, t[2], *(dev(a[back]) for a in given[3:]))
    IR.same_bits(host(swapped[0]), all_ids[back]), IR.same_bits(host(swapped[1]), all_sc[back])
