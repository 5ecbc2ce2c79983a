"""What the three storages of the inverted file state once and share (mdir_amd/ivf.py ``InvertedLists``; csrc/mdx_ivf_plan.h): one
partition whatever the storage, one column layout of the candidates whatever the scorer, and one set of label checks for the
constructor and ``IVFPQIndex.add``.  The shape is the smallest with an empty list, a partial tile, a full tile, two tiles and a bit,
and a third, partial group of entries on a list."""
import numpy as np
import pytest
import torch

from test_gpu_ivf import SIZES, dev, host, labels_of_sizes

pytestmark = pytest.mark.gpu
F32 = np.float32
D, M_SUB, NPROBE = 64, 4, 3


@pytest.fixture(scope="module")
def family():
    """(rows, centroids, labels, codebook) on the device and the three indices of them."""
    from mdir_amd import ivf, ivfpq
    rng = np.random.default_rng(27)
    n, lists = sum(SIZES), len(SIZES)
    rows, cents = dev(rng.standard_normal((n, D)).astype(F32)), dev(rng.standard_normal((lists, D)).astype(F32))
    labels = dev(labels_of_sizes(rng, SIZES))
    codebook = dev(rng.standard_normal((M_SUB, 256, D // M_SUB)).astype(F32))
    made = (ivf.IVFIndex(rows, cents, labels), ivf.IVFIndex(rows, cents, labels, storage="i8"),
            ivfpq.IVFPQIndex(rows, cents, labels, m=M_SUB, codebook=codebook, keep_rows=False))
    yield rows, cents, labels, codebook, made
    for index in made:
        index.close()


def test_one_partition_and_one_column_layout_whatever_the_storage(family):
    from mdir_amd import ops
    rows, cents, labels, codebook, (f32, i8, coded) = family
    for other in (i8, coded):
        assert torch.equal(other.order, f32.order) and torch.equal(other.offsets, f32.offsets)
        assert other.host_sizes == f32.host_sizes == list(SIZES) and other._capacity == f32._capacity
    rng = np.random.default_rng(28)
    nq, lists = 2 * ops.IVF_QUERY_GROUP + 1, len(SIZES)
    # every query probes the largest list -- two full groups of entries and a third of one -- and two of the others, the empty one too
    probes = np.array([[lists - 1] + list(rng.permutation(lists - 1)[:NPROBE - 1]) for _ in range(nq)], np.int64)
    assert (probes[:, 1:] == 0).any()
    probes_t, queries = dev(probes), dev(rng.standard_normal((nq, D)).astype(F32))
    cap, items = f32.capacity(NPROBE), f32.items(nq, NPROBE)
    plan = ops.ivf_plan(probes_t, f32.offsets, f32.n, cap)
    _, ids_f32 = ops.ivf_scan(rows, f32.order, f32.offsets, queries, plan, NPROBE, cap, items)
    qcodes, qscales = ops.quantize_i8(ops.center_rows(queries, "ND", None))
    _, ids_i8 = ops.lists_i8_scan(i8.codes, i8.scales, D, i8.order, i8.offsets, qcodes, qscales, plan, NPROBE, cap, items)
    coarse = dev(rng.standard_normal((nq, NPROBE)).astype(F32))
    _, ids_pq = ops.lists_pq_scan(coded.codes, coded.order, coded.n, coded.offsets, ops.pq_lut(codebook, queries), coarse, probes_t, plan, cap)
    assert torch.equal(ids_i8, ids_f32) and torch.equal(ids_pq, ids_f32)
    # and that layout is the plan's: the members of the probed lists back to back in probe order, -1 beyond them
    order, offsets, got = host(f32.order), host(f32.offsets), host(ids_f32)
    for q in range(nq):
        want = np.concatenate([order[offsets[l]:offsets[l + 1]] for l in probes[q]])
        assert np.array_equal(got[q, :len(want)], want) and (got[q, len(want):] == -1).all()


def test_the_constructor_and_add_refuse_the_same_labels_in_their_own_words(family):
    from mdir_amd import ivf
    rows, cents, labels, codebook, (f32, i8, coded) = family
    n, lists, b = rows.shape[0], len(SIZES), 5
    batch, few = rows[:b].contiguous(), labels[:b].contiguous()
    held = (coded.n, coded.size, list(coded.host_sizes), list(coded._capacity))
    for spoil in (lambda t: t.int(), lambda t: t[:-1], lambda t: t.tolist()):
        with pytest.raises(ValueError, match="labels must be an int64 \\[%d\\]" % n):
            ivf.IVFIndex(rows, cents, spoil(labels))
        with pytest.raises(ValueError, match="labels must be an int64 \\[%d\\]" % b):
            coded.add(batch, spoil(few))
    for at, value in ((0, lists), (b - 1, -1)):
        bad_all, bad_few = labels.clone(), few.clone()
        bad_all[at], bad_few[at] = value, value
        with pytest.raises(ValueError, match="labels must lie in \\[0, %d\\)" % lists):
            ivf.IVFIndex(rows, cents, bad_all)
        with pytest.raises(ValueError, match="labels must lie in \\[0, %d\\)" % lists):
            coded.add(batch, bad_few)
    assert (coded.n, coded.size, coded.host_sizes, coded._capacity) == held         # a refused batch leaves the index as it was
