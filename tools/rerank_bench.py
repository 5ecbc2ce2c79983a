#!/usr/bin/env python3
"""Re-ranking on one MI355X, one JSON line on stdout (profiles/r07_rerank.{json,md}).

  aqe        alpha-QE at configs[2] (N = 1 004 993, Q = 70, D = 2048, exact chain): per-stage ms from HIP events --
             scores, topk, aggregate, scores, ranking (mdx_rank_full of the expanded scores) -- median / min / max over
             --steps steps after --warmup, and queries/s of the whole step
  aggregate  mdx_knn_aggregate alone at the DBA shape (1 M output rows, k = 10, D = 2048): GB/s over
             nq*k*d*4 + 2*nq*d*4 bytes and the fraction of 8 TB/s
  dba        database_augmentation whole, k = 10, at N = 100 000 and N = 1 004 993 (default chunk): seconds, and the fraction
             of the fp32 MFMA peak (157.3 TFLOP/s) over 2 N^2 D flops
  scores_nq  the exact similarity (mdx_scores_rowmajor) against the 1 M database at several nq (the DBA chunk included):
             ms and fraction of the fp32 MFMA peak

    python tools/rerank_bench.py [--steps 20] [--warmup 3] [--no-dba-1m]
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

PEAK_F32 = 157.3e12          # fp32 MFMA, dense, spec (MI355X)
PEAK_HBM = 8.0e12            # bytes/s, spec
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


def bench_aqe(x, steps, warmup, k=2, alpha=3.0, nq=70):
    q = x[::x.shape[0] // nq][:nq] + 0.8 * unit_rows(nq, x.shape[1], 2)
    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    n = x.shape[0]
    sc = torch.empty((nq, n), dtype=torch.float32, device=DEV)
    ranks = torch.empty((nq, n), dtype=torch.int64, device=DEV)
    ws = ops._workspace(ops.rank_workspace_bytes(n, nq), DEV)
    names = ("scores", "topk", "aggregate", "scores2", "ranking")
    per = {s: [] for s in names}
    total = []
    for step in range(warmup + steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        ops.scores_rowmajor(x, q, "ND", out=sc)
        ev[1].record()
        ids, sims = ops.topk(sc, k, workspace=ws)
        ev[2].record()
        qx = ops.knn_aggregate(x, ids, sims, alpha, self_rows=q)
        ev[3].record()
        ops.scores_rowmajor(x, qx, "ND", out=sc)
        ev[4].record()
        ops.rank_full(sc, out=ranks, workspace=ws)
        ev[5].record()
        torch.cuda.synchronize()
        if step >= warmup:
            for i, s in enumerate(names):
                per[s].append(ev[i].elapsed_time(ev[i + 1]))
            total.append(ev[0].elapsed_time(ev[-1]))
    # the library path (rerank.query_expansion) gives the same scores as the staged loop above
    lib_scores, _ = rerank.query_expansion(q, x, k, alpha)
    same = bool(torch.equal(lib_scores, sc))
    med = float(np.median(total))
    return {"n": n, "nq": nq, "d": x.shape[1], "k": k, "alpha": alpha, "steps": steps, "warmup": warmup,
            "stage_ms": {s: stats(v) for s, v in per.items()}, "step_ms": stats(total),
            "queries_per_s": round(nq / (med / 1e3), 1), "staged_equals_rerank_api": same}


def bench_aggregate(x, steps, k=10, alpha=3.0):
    n, d = x.shape
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    ids = torch.randint(0, n, (n, k), generator=g, device=DEV, dtype=torch.int64)
    sims = torch.rand((n, k), generator=g, device=DEV) * 0.5 + 0.5
    out = torch.empty_like(x)
    ops.knn_aggregate(x, ids, sims, alpha, out=out)
    times = []
    for _ in range(max(3, steps // 4)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.knn_aggregate(x, ids, sims, alpha, out=out)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    med = float(np.median(times))
    nbytes = n * k * d * 4 + 2 * n * d * 4
    return {"nq": n, "k": k, "d": d, "ms": stats(times), "bytes": nbytes, "GB_per_s": round(nbytes / (med / 1e3) / 1e9, 1),
            "fraction_of_8TBps": round(nbytes / (med / 1e3) / PEAK_HBM, 3)}


def bench_scores_nq(x, nqs, reps=5):
    n, d = x.shape
    res = []
    for nq in nqs:
        q = x[:nq].contiguous()
        out = torch.empty((nq, n), dtype=torch.float32, device=DEV)
        ops.scores_rowmajor(x, q, "ND", out=out)
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.scores_rowmajor(x, q, "ND", out=out)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        med = float(np.median(times))
        res.append({"nq": nq, "ms": stats(times), "fraction_of_fp32_mfma_peak": round(2.0 * nq * n * d / (med / 1e3) / PEAK_F32, 3)})
        del out
    return res


def bench_dba(x, k=10, alpha=3.0):
    n, d = x.shape
    chunk = rerank.dba_chunk(n, k)
    rerank.database_augmentation(x[:min(n, 4 * chunk)].contiguous(), k, alpha, chunk=chunk)     # warm the shapes
    torch.cuda.synchronize()
    t0 = time.time()
    out = rerank.database_augmentation(x, k, alpha)
    torch.cuda.synchronize()
    sec = time.time() - t0
    del out
    return {"n": n, "d": d, "k": k, "chunk": chunk, "seconds": round(sec, 3),
            "fraction_of_fp32_mfma_peak": round(2.0 * n * n * d / sec / PEAK_F32, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-dba-1m", action="store_true", help="skip the ~1 minute DBA of the 1 M database")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rerank_bench.py needs an MI355X: there is no CPU fallback")
    n, d = 1004993, 2048
    x = unit_rows(n, d, 1)
    line = {"tool": "rerank_bench", "device": torch.cuda.get_device_name(0)}
    line["aqe"] = bench_aqe(x, args.steps, args.warmup)
    line["aggregate"] = bench_aggregate(x, args.steps)
    chunk_1m = rerank.dba_chunk(n, 10)
    line["scores_nq"] = bench_scores_nq(x, sorted({70, 128, chunk_1m, 512, 1024}))
    line["dba"] = [bench_dba(x[:100000].contiguous())]
    if not args.no_dba_1m:
        line["dba"].append(bench_dba(x))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
