#!/usr/bin/env python3
"""Truncated diffusion on one MI355X, one JSON line on stdout (profiles/r09_truncated_diffusion.{json,md}).

For R in --truncate (default 1000 and 4096), 70 queries, iters = 20, kq = 10, k = 50:

  ring       N = 1 004 993 ring lattice (row i lists i +- 1 .. i +- 25: every edge mutual), first-stage scores peaked on a
             contiguous arc per query, so every subgraph row keeps about k edges: the upper bound of the solve's work
  configs2   the graph of N = 1 004 993 random unit rows (D = 2048, as profiles/r08), queries near database rows: the top-R
             rows of a query are hardly each other's neighbours, so the subgraphs are nearly empty: the lower bound
  small      the same at rOxford5k size (N = 4 993, D = 2048)

Each reports, as HIP events (median / min / max over --steps after --warmup):
  call_ms    ops.diffusion_truncated: the solve launch, out = s - 3 over [nq, N], the scatter of f
  topk_ms    mdx_topk of the first-stage scores with k = R
  whole_ms   the batch: (configs2 / small: the similarity +) topk(R) + the truncated solve + mdx_rank_full
and the kept edges per subgraph row (mean over the queries), the steps taken and the residuals.  The split of call_ms into
the solve kernel and the two output passes is rocprofv3's (--kernel-trace --stats around this tool).

    python tools/diffusion_truncated_bench.py [--steps 10] [--warmup 2] [--truncate 1000 4096] [--no-1m] [--no-random-1m]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mdir_amd import ops, rerank  # noqa: E402
from diffusion_bench import stats, timed, unit_rows  # noqa: E402  (tools/ is sys.path[0])

DEV = "cuda:0"
NQ, ITERS, KQ, GAMMA, ALPHA, K = 70, 20, 10, 3.0, 0.99, 50


def kept_edges(wgraph, tid):
    """Mean over the queries of the in-set ELL entries per subgraph row (host, on the device's lists)."""
    cols, _, counts = wgraph
    out = []
    for q in range(tid.shape[0]):
        t = tid[q]
        c = cols[t].long()
        valid = torch.arange(cols.shape[1], device=DEV)[None, :] < counts[t].long()[:, None]
        inset = torch.isin(c, t) & valid
        out.append(inset.sum().item() / t.numel())
    return round(float(np.mean(out)), 3)


def one(wgraph, first, r, steps, warmup, similarity=None):
    n = first.shape[1]
    ws = ops._workspace(ops.rank_workspace_bytes(n, NQ), DEV)
    out = torch.empty_like(first)
    tid, tsim = ops.topk(first, r, workspace=ws)
    _, res, nsteps = ops.diffusion_truncated(wgraph, first, tid, tsim, KQ, GAMMA, ALPHA, ITERS, 1e-6, out=out,
                                             return_residual=True)

    def whole():
        if similarity is not None:
            similarity()
        i, s = ops.topk(first, r, workspace=ws)
        ops.diffusion_truncated(wgraph, first, i, s, KQ, GAMMA, ALPHA, ITERS, 1e-6, out=out)
        ops.rank_full(out)

    call = timed(lambda: ops.diffusion_truncated(wgraph, first, tid, tsim, KQ, GAMMA, ALPHA, ITERS, 1e-6, out=out),
                 steps, warmup)
    topk = timed(lambda: ops.topk(first, r, workspace=ws), steps, warmup)
    batch = timed(whole, steps, warmup)
    return {"r": r, "call_ms": stats(call), "topk_ms": stats(topk), "whole_ms": stats(batch),
            "queries_per_s": round(NQ / (float(np.median(batch)) / 1e3), 1), "kept_edges_per_row": kept_edges(wgraph, tid),
            "steps_taken": [int(nsteps.min().item()), int(nsteps.max().item())],
            "residual": [float(res.min().item()), float(res.max().item())]}


def bench_ring(n, rs, steps, warmup):
    off = torch.cat([torch.arange(1, K // 2 + 1), -torch.arange(1, K // 2 + 1)]).to(DEV)
    ids = (torch.arange(n, device=DEV)[:, None] + off[None, :]) % n
    sims = (1.0 - 0.01 * off.abs().float())[None, :].expand(n, K).contiguous()
    wgraph = ops.knn_graph_weights(ids, sims, GAMMA)
    del ids, sims
    centre = torch.arange(NQ, device=DEV)[:, None] * (n // NQ) + 12345
    j = torch.arange(n, device=DEV)[None, :]
    first = (0.9 - torch.minimum((j - centre) % n, (centre - j) % n).float() / n).contiguous()
    del j
    return {"n": n, "k": K, "nq": NQ, "runs": [one(wgraph, first, r, steps, warmup) for r in rs]}


def bench_random(n, d, rs, steps, warmup, seed):
    x = unit_rows(n, d, seed)
    graph = rerank.DiffusionGraph(x, k=K, gamma=GAMMA, weights=True)
    wgraph = (graph.cols, graph.wvals, graph.counts)
    q = x[::max(1, n // NQ)][:NQ] + 0.8 * unit_rows(NQ, d, seed + 1)
    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    first = torch.empty((NQ, n), dtype=torch.float32, device=DEV)
    ops.scores_rowmajor(x, q, "ND", out=first)
    runs = [one(wgraph, first, min(r, n), steps, warmup, lambda: ops.scores_rowmajor(x, q, "ND", out=first)) for r in rs]
    return {"n": n, "d": d, "k": K, "nq": NQ, "edges": graph.edges(), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--truncate", type=int, nargs="+", default=[1000, 4096])
    ap.add_argument("--no-1m", action="store_true", help="rOxford5k size only")
    ap.add_argument("--no-random-1m", action="store_true", help="skip the 1M random-database graph (its build takes ~40 s)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diffusion_truncated_bench needs an MI355X (cuda:0)")
    res = {"device": torch.cuda.get_device_name(0), "iters": ITERS, "kq": KQ, "gamma": GAMMA, "alpha": ALPHA}
    res["roxford_size"] = bench_random(4993, 2048, a.truncate, a.steps, a.warmup, seed=1)
    if not a.no_1m:
        res["ring_1m"] = bench_ring(1004993, a.truncate, a.steps, a.warmup)
        torch.cuda.empty_cache()
        if not a.no_random_1m:
            res["configs2"] = bench_random(1004993, 2048, a.truncate, a.steps, a.warmup, seed=2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
