#!/usr/bin/env python3
"""k-reciprocal re-ranking on one MI355X, one JSON line on stdout (profiles/r17_k_reciprocal.{json,md}).

The build, on clustered synthetic unit rows (clusters of --cluster rows around random centres; random rows have near-empty
reciprocal sets), k1 = 20, k2 = 6: search.knn_join on its own, then each encoding pass (sets, raw offsets, raw fill, expand
offsets, expand fill) as HIP events with the bytes it must move (its inputs read once and its outputs written once; the rows
the raw fill gathers for pairs outside the lists are counted from the data) and the resulting bytes / s; mean and maximum nnz of
both CSRs; the device bytes the encoding keeps.

The query-time call, 70 queries near database rows, truncate = 1000 and 4096: ops.krecip_rerank alone and the batch (topk(R) +
the call), beside rerank.diffusion(..., truncate=R) (k = 50, its defaults) on the same rows as the only reference point.

    python tools/krecip_bench.py [--n 1004993] [--d 2048] [--steps 5] [--warmup 1] [--truncate 1000 4096] [--no-diffusion]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mdir_amd import ops, rerank, search  # noqa: E402
from diffusion_bench import stats, timed  # noqa: E402  (tools/ is sys.path[0])

DEV = "cuda:0"
NQ, K1, K2, LAM = 70, 20, 6, 0.3


def clustered_rows(n, d, cluster, seed, sigma=0.175):
    """[n, d] unit rows: row i = centre[i % nc] + sigma * sqrt(d) * noise (the set of tests/test_gpu_krecip.py), made in slices."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    nc = max(1, n // cluster)
    cent = torch.randn((nc, d), generator=g, device=DEV)
    x = torch.empty((n, d), dtype=torch.float32, device=DEV)
    step = 1 << 16
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        lab = torch.arange(lo, hi, device=DEV) % nc
        x[lo:hi] = cent[lab] + sigma * d ** 0.5 * torch.randn((hi - lo, d), generator=g, device=DEV)
        x[lo:hi] /= x[lo:hi].norm(dim=1, keepdim=True)
    return x


def once(fn):
    """(result, ms) of one call between HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts)


def passed(ms, moved):
    return {"ms": round(ms, 3), "bytes": int(moved), "gb_per_s": round(moved / ms / 1e6, 1)}


def build(x):
    n, d = x.shape
    k = min(K1, n)
    res, join_ms = once(lambda: search.knn_join(None, x, k))
    ids, sims = res.ids, res.scores
    out = {"knn_join_ms": round(join_ms, 1)}
    sets, ms = once(lambda: ops.krecip_sets(ids))
    out["sets"] = passed(ms, nbytes(ids) * (1 + k) + nbytes(*sets))                     # every entry scans one other list
    ro, ms = once(lambda: ops.krecip_raw_offsets(sets))
    out["raw_offsets"] = passed(ms, nbytes(sets[0], sets[1]) + sets[0].numel() * sets[2].shape[1] * 4 + 3 * nbytes(ro))
    nnz = int(ro[n].item())
    (rc, rv), ms = once(lambda: ops.krecip_raw_fill(x, ids, sims, sets, ro, nnz))
    row = torch.repeat_interleave(torch.arange(n, device=DEV), ro[1:] - ro[:-1])
    outside = int((~(ids[row] == rc.long()[:, None]).any(dim=1)).sum().item())
    del row
    out["raw_fill"] = passed(ms, nbytes(sets[0], sets[1], ids, sims, ro, rc, rv) + sets[0].numel() * sets[2].shape[1] * 4
                             + 2 * outside * d * 4)
    out["raw_fill"]["pairs_outside_the_lists"] = outside
    raw = (ro, rc, rv)
    kk = min(K2, k)
    eo, ms = once(lambda: ops.krecip_expand_offsets(ids, kk, raw))
    out["expand_offsets"] = passed(ms, nbytes(ids) + kk * nbytes(rc) + 3 * nbytes(eo))
    ennz = int(eo[n].item())
    (ec, ev), ms = once(lambda: ops.krecip_expand_fill(ids, kk, raw, eo, ennz))
    out["expand_fill"] = passed(ms, nbytes(ids, eo, ec, ev) + kk * nbytes(rc, rv))
    for name, o in (("raw", ro), ("expanded", eo)):
        lens = o[1:] - o[:-1]
        out[name + "_nnz"] = {"total": int(o[n].item()), "mean": round(float(lens.float().mean().item()), 2), "max": int(lens.max().item())}
    kth = sims[:, k - 1].contiguous()
    out["device_bytes"] = nbytes(*sets, ro, rc, rv, eo, ec, ev, kth)
    return (sets, kth, k, kk, raw, (eo, ec, ev)), out


def query(x, enc, rs, steps, warmup, with_diffusion):
    sets, kth, k, kk, raw, exp = enc
    n, d = x.shape
    g = torch.Generator(device=DEV).manual_seed(7)
    q = x[::max(1, n // NQ)][:NQ] + 0.175 * torch.randn((NQ, d), generator=g, device=DEV)
    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    first = ops.scores_rowmajor(x, q, "ND")
    out = torch.empty_like(first)
    ws = ops._workspace(ops.rank_workspace_bytes(n, NQ), DEV)
    runs = []
    graph = rerank.DiffusionGraph(x, weights=True) if with_diffusion else None
    for r in rs:
        r = min(r, n)
        top = ops.topk(first, r, workspace=ws)[0]
        call = timed(lambda: ops.krecip_rerank((sets[2], sets[3]), kth, k, kk, raw, exp, first, top, LAM, out=out), steps, warmup)
        batch = timed(lambda: ops.krecip_rerank((sets[2], sets[3]), kth, k, kk, raw, exp, first,
                                                ops.topk(first, r, workspace=ws)[0], LAM, out=out), steps, warmup)
        run = {"r": r, "call_ms": stats(call), "topk_plus_call_ms": stats(batch)}
        if graph is not None:
            dif = timed(lambda: rerank.diffusion(q, x, graph, scores=first, truncate=r), steps, warmup)
            run["diffusion_truncated_topk_plus_call_ms"] = stats(dif)
        runs.append(run)
    return {"nq": NQ, "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--cluster", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--truncate", type=int, nargs="+", default=[1000, 4096])
    ap.add_argument("--no-diffusion", action="store_true", help="skip the truncated-diffusion reference (its graph is a second kNN join)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("krecip_bench needs an MI355X (cuda:0)")
    x = clustered_rows(a.n, a.d, a.cluster, seed=1)
    res = {"device": torch.cuda.get_device_name(0), "n": a.n, "d": a.d, "cluster": a.cluster, "k1": K1, "k2": K2, "lam": LAM}
    enc, res["build"] = build(x)
    print(json.dumps(res), file=sys.stderr, flush=True)                               # the build alone, should the rest be cut short
    res["query"] = query(x, enc, a.truncate, a.steps, a.warmup, not a.no_diffusion)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
