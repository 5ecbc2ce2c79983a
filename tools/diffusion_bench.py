#!/usr/bin/env python3
"""Diffusion on one MI355X, one JSON line on stdout (profiles/r08_diffusion.{json,md}).

  graph      the graph at configs[2] (N = 1 004 993, D = 2048, k = 50, random unit rows), DiffusionGraph's steps: the whole
             build (host clock around the synchronised lists + graph) and mdx_knn_graph alone (HIP events, on the
             same lists), the mean and maximum edges per row.  A random database has little mutual structure: its edge counts are not those of
             real descriptors.
  solve      one 70-query solve, iters = 20, on that graph: ms per batch (HIP events, median / min / max over --steps after
             --warmup), queries/s including the first-stage similarity and the seeds' top-k, and the SpMM's GB/s over
             edges * (nq_pad * 4 + 8) + N * nq_pad * 4 * 2 bytes per step over the time of a WHOLE CG step (SpMM, the
             vector passes and the reductions): a lower bound of the SpMM's own rate (its kernel time: rocprofv3)
  ring       the same solve on a ring lattice at N = 1 004 993, k = 50 (row i lists i +- 1 .. i +- 25: every edge mutual,
             50.2 M edges), the edge count of a database with real mutual structure; its neighbours are adjacent rows, so
             the gathers hit the caches far more often than on real data
  small      the same solve at rOxford5k size (N = 4 993, D = 2048, k = 50): microseconds

    python tools/diffusion_bench.py [--steps 10] [--warmup 2] [--no-1m]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mdir_amd import ops, rerank  # noqa: E402

DEV = "cuda:0"


def unit_rows(n, d, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=DEV)
    x /= x.norm(dim=1, keepdim=True)
    return x


def stats(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def timed(fn, steps, warmup):
    out = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return out


def bench(n, d, k, nq, steps, warmup, seed, iters=20, kq=10, gamma=3.0, alpha=0.99):
    x = unit_rows(n, d, seed)
    kk = min(k, n)
    # DiffusionGraph's own steps, timed apart: the chunked exact similarity + top-k lists, then mdx_knn_graph
    torch.cuda.synchronize()
    t0 = time.time()
    ids = torch.empty((n, kk), dtype=torch.int64, device=DEV)
    sims = torch.empty((n, kk), dtype=torch.float32, device=DEV)
    chunk = rerank.dba_chunk(n, kk)
    block = torch.empty((chunk, n), dtype=torch.float32, device=DEV)
    tws = ops._workspace(ops.rank_workspace_bytes(n, chunk), DEV)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        ids[i0:i1], sims[i0:i1] = ops.topk(ops.scores_rowmajor(x, x[i0:i1], "ND", out=block[:i1 - i0]), kk, workspace=tws)
    del block, tws
    cols, vals, counts = ops.knn_graph(ids, sims, gamma)
    torch.cuda.synchronize()
    build_s = time.time() - t0
    graph_ms = timed(lambda: ops.knn_graph(ids, sims, gamma), max(3, steps // 2), 1)
    del ids, sims
    graph = (cols, vals, counts)
    edges = int(counts.sum(dtype=torch.int64).item())
    counts = counts.double()

    q = x[::max(1, n // nq)][:nq] + 0.8 * unit_rows(nq, d, seed + 1)
    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    first = torch.empty((nq, n), dtype=torch.float32, device=DEV)
    out = torch.empty_like(first)
    ws = ops._workspace(ops.rank_workspace_bytes(n, nq), DEV)

    def solve_only():
        ops.diffusion(graph, first, sid, ssim, gamma, alpha, iters, 1e-6, out=out)

    def whole():
        ops.scores_rowmajor(x, q, "ND", out=first)
        s_ids, s_sims = ops.topk(first, kq, workspace=ws)
        ops.diffusion(graph, first, s_ids, s_sims, gamma, alpha, iters, 1e-6, out=out)

    ops.scores_rowmajor(x, q, "ND", out=first)
    sid, ssim = ops.topk(first, kq, workspace=ws)
    _, res, nsteps = ops.diffusion(graph, first, sid, ssim, gamma, alpha, iters, 1e-6, out=out, return_residual=True)
    solve = timed(solve_only, steps, warmup)
    step = timed(whole, steps, warmup)
    nqp = (nq + 3) // 4 * 4
    spmm_bytes = edges * (nqp * 4 + 8) + n * nqp * 4 * 2
    med = float(np.median(solve))
    return {"n": n, "d": d, "k": kk, "nq": nq, "kq": kq, "iters": iters, "gamma": gamma, "alpha": alpha,
            "graph_build_s": round(build_s, 3), "knn_graph_ms": stats(graph_ms),
            "edges": edges, "counts_mean": round(float(counts.mean().item()), 3), "counts_max": int(counts.max().item()),
            "solve_ms": stats(solve), "solve_ms_per_cg_step": round(med / iters, 4),
            "whole_ms": stats(step), "queries_per_s": round(nq / (float(np.median(step)) / 1e3), 1),
            "spmm_bytes_per_step": int(spmm_bytes),
            "spmm_gbs_over_whole_step": round(spmm_bytes / (med / iters / 1e3) / 1e9, 1),
            "gathered_block_mb": round(n * nqp * 4 / 1e6, 1),
            "steps_taken": [int(nsteps.min().item()), int(nsteps.max().item())],
            "residual": [float(res.min().item()), float(res.max().item())]}


def bench_ring(n, k, nq, steps, warmup, iters=20, kq=10, gamma=3.0, alpha=0.99):
    off = torch.cat([torch.arange(1, k // 2 + 1), -torch.arange(1, k // 2 + 1)]).to(DEV)
    ids = (torch.arange(n, device=DEV)[:, None] + off[None, :]) % n
    sims = (1.0 - 0.01 * off.abs().float())[None, :].expand(n, k).contiguous()
    graph = ops.knn_graph(ids, sims, gamma)
    del ids, sims
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    first = torch.rand((nq, n), generator=g, device=DEV)
    out = torch.empty_like(first)
    sid, ssim = ops.topk(first, kq)
    solve = timed(lambda: ops.diffusion(graph, first, sid, ssim, gamma, alpha, iters, 1e-6, out=out), steps, warmup)
    edges = int(graph[2].sum(dtype=torch.int64).item())
    nqp = (nq + 3) // 4 * 4
    spmm_bytes = edges * (nqp * 4 + 8) + n * nqp * 4 * 2
    med = float(np.median(solve))
    return {"n": n, "k": k, "nq": nq, "iters": iters, "edges": edges, "solve_ms": stats(solve),
            "solve_ms_per_cg_step": round(med / iters, 4), "spmm_bytes_per_step": int(spmm_bytes),
            "spmm_gbs_over_whole_step": round(spmm_bytes / (med / iters / 1e3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-1m", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diffusion_bench needs an MI355X (cuda:0)")
    res = {"device": torch.cuda.get_device_name(0)}
    res["roxford_size"] = bench(4993, 2048, 50, 70, a.steps, a.warmup, seed=1)
    if not a.no_1m:
        res["configs2"] = bench(1004993, 2048, 50, 70, a.steps, a.warmup, seed=2)
        torch.cuda.empty_cache()
        res["ring_1m"] = bench_ring(1004993, 50, 70, a.steps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
