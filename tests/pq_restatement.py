"""The product quantiser (mdir_amd/pq.py) and the IVF-PQ search (include/mdx_lists_pq.h; mdir_amd/ivfpq.py) restated in numpy (a helper
module, imported by test_pq_host.py, test_gpu_lists_pq.py and test_gpu_lists_pq_memcontract.py; no GPU).

``chain``       the exact fp32 chain of the library between the rows of two matrices, with its zero padding to a multiple of 64
``assign``      labels and winning values of every sub-vector: the first argmax of fl(chain + bias)
``encode`` / ``decode`` / ``train``   as pq.py states them; ``train`` draws from the same torch generator
``lut``         the table of a batch of queries
``scan``        per query the candidate ids and ADC scores in column order
``search``      scan + the selection of tests/ivf_restatement.py
"""
import numpy as np

import ivf_restatement as IR
import kmeans_restatement as KR

F32 = np.float32
CODEWORDS = 256


def chain(a, b):
    """fp32 [len(a), len(b)]: acc = +0, acc = fmaf(a[k], b[k], acc) for k ascending, continued over zeros to round_up(d, 64): where
    d % 64 != 0 one more fmaf(0, 0, acc), which is acc + 0 (a -0 becomes +0)."""
    from oracle import chain as OC
    out = OC.gemm_nt_chain(a, b)
    return out + F32(0) if a.shape[1] % 64 else out


def bias(words_m):
    """fp32 [256]: -0.5 * chain(c_j, c_j) (the multiplication is exact)."""
    return (F32(-0.5) * np.diagonal(chain(words_m, words_m))).astype(F32)


def assign(words, vectors):
    """(labels int64 [T, M], best fp32 [T, M]): per subspace the first argmax of fl(chain(v_m, c_mj) + b_mj), ties to the smaller id,
    -0 == +0, NaN last."""
    words, vectors = np.asarray(words, F32), np.asarray(vectors, F32)
    m_sub, _, dsub = words.shape
    labels = np.empty((len(vectors), m_sub), np.int64)
    best = np.empty((len(vectors), m_sub), F32)
    for m in range(m_sub):
        block = chain(vectors[:, m * dsub:(m + 1) * dsub], words[m]) + bias(words[m])[None, :]        # one fp32 addition
        labels[:, m], best[:, m] = KR.argmax_first(block)
    return labels, best


def encode(words, vectors):
    return assign(words, vectors)[0].astype(np.uint8)


def decode(words, codes):
    words = np.asarray(words, F32)
    return np.concatenate([words[m][codes[:, m].astype(np.int64)] for m in range(words.shape[0])], axis=1)


def draw(t, seed, train_rows=None):
    """(sample ids or None, the ids of the initial codewords within the sample): pq.train's draws from its torch generator."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    sample = None
    if train_rows is not None:
        perm = torch.randperm(t, generator=gen)
        if train_rows < t:
            sample = np.sort(perm[:train_rows].numpy())
    rows = t if sample is None else len(sample)
    return sample, torch.randperm(rows, generator=gen)[:CODEWORDS].numpy()


def train(vectors, m_sub, iters=10, seed=0, train_rows=None, initial=None):
    """(codewords fp32 [M, 256, dsub], history, iterations) of pq.train.  ``initial``: ids of the first codewords within the training
    sample, in place of the generator's."""
    vectors = np.asarray(vectors, F32)
    t, d = vectors.shape
    dsub = d // m_sub
    sample, first = draw(t, seed, train_rows)
    if initial is not None:
        first = np.asarray(initial)
    rows = vectors if sample is None else vectors[sample]
    words = np.ascontiguousarray(rows[first].reshape(CODEWORDS, m_sub, dsub).transpose(1, 0, 2))
    history, updates, previous = [], 0, None
    while True:
        labels, best = assign(words, rows)
        history.extend(best.astype(np.float64).sum(axis=0).tolist())
        changed = labels.size if previous is None else int((labels != previous).sum())
        if updates == iters or changed == 0:
            break
        for m in range(m_sub):
            members, offsets = KR.csr(labels[:, m], CODEWORDS)
            sums = KR.sums32(np.ascontiguousarray(rows[:, m * dsub:(m + 1) * dsub]), members, offsets, CODEWORDS)
            counts = np.diff(offsets)
            have = counts > 0
            words[m][have] = sums[have] / counts[have].astype(F32)[:, None]                     # one fp32 division
        previous = labels
        updates += 1
    return words, history, updates


def centred(queries, center=None):
    queries = np.asarray(queries, F32)
    return queries if center is None else queries - np.asarray(center, F32)[None, :]


def lut(words, queries, center=None):
    """fp32 [nq, M, 256]: the chain of sub-vector m of x_q = q - center with every codeword of subspace m."""
    words = np.asarray(words, F32)
    m_sub, _, dsub = words.shape
    x = centred(queries, center)
    return np.stack([chain(x[:, m * dsub:(m + 1) * dsub], words[m]) for m in range(m_sub)], axis=1)


def scan(codes, members, n, offsets, table, coarse, probes, cap=None):
    """Per query (ids int64, scores fp32) of its candidates in column order: the members of its valid probes' lists in probe order;
    score = coarse[q, p], then + table[q, m, code[m]] for m ascending, fp32 additions; NaN for a member id outside [0, n).  ``codes``
    uint8 [len(members), M] in list order."""
    members = np.asarray(members, np.int64)
    starts, sizes = IR.clamped(offsets, len(members))
    out = []
    for q, row in enumerate(np.asarray(probes, np.int64)):
        ids, scores = [np.empty(0, np.int64)], [np.empty(0, F32)]
        for p, l in enumerate(row):
            if not 0 <= l < len(sizes):
                continue
            at = slice(int(starts[l]), int(starts[l] + sizes[l]))
            acc = np.full(int(sizes[l]), coarse[q, p], F32)
            for m in range(codes.shape[1]):
                acc = acc + table[q, m, codes[at, m].astype(np.int64)]
            acc[(members[at] < 0) | (members[at] >= n)] = np.nan
            ids.append(members[at]), scores.append(acc.astype(F32))
        ids, scores = np.concatenate(ids), np.concatenate(scores)
        out.append((ids, scores) if cap is None else (ids[:cap], scores[:cap]))
    return out


def search(codes, members, n, offsets, table, coarse, probes, k, cap=None):
    """(ids int64 [nq, k], scores fp32 [nq, k], scanned int64 [nq]): the ADC ranking."""
    cands = scan(codes, members, n, offsets, table, coarse, probes, cap)
    ids, sc = np.empty((len(cands), k), np.int64), np.empty((len(cands), k), F32)
    for q, (cand_ids, cand_scores) in enumerate(cands):
        ids[q], sc[q] = IR.select(cand_scores, cand_ids, k)
    return ids, sc, np.array([len(c[0]) for c in cands], np.int64)
