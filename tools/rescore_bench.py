#!/usr/bin/env python3
"""Exact rescoring of int8 shortlists (mdx_rescore / mdx_rescore_certify) on one MI355X, one JSON line on stdout
(profiles/r11_rescore.{json,md}).

Shape: 1 004 993 x 2048, 70 queries (each a database row plus noise, as tools/i8_bench.py), K in {100, 1000, 4096}.  As HIP
events (median / min / max over --steps after --warmup):
  rescore_ms      ops.rescore of the [70, K] shortlist, and GB/s on the gathered bytes (70 K d 4)
  certify_ms      ops.rescore_certify
  batch_ms        the certified batch: i8 similarity + topk(K) + rescore + certify, and queries/s from its median
  f32_batch_ms    the exact fp32 batch it stands beside: scores_rowmajor + topk(k), k = 10
  search_exact_ms search(..., k=10, exact=True) (the batch, plus scores_rowmajor + topk on the queries whose certified depth
                  is below k), and the share of queries that fell back
and the certified depth (min / p10 / median) on random unit rows and on a clustered set (2 000 centres, spread 0.02 per
element).  The per-kernel split is rocprofv3's (--kernel-trace --stats around this tool, in a run of its own).

    python tools/rescore_bench.py [--steps 20] [--warmup 3] [--n 1004993]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mdir_amd import ops  # noqa: E402
from mdir_amd.search import search  # noqa: E402
from diffusion_bench import stats, timed, unit_rows  # noqa: E402  (tools/ is sys.path[0])

DEV = "cuda:0"
K_SET = (100, 1000, 4096)
K_SMALL = 10


def queries(x, nq, seed):
    n, d = x.shape
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    q = x[torch.arange(0, n, n // nq, device=DEV)[:nq]] + 0.05 * torch.randn((nq, d), generator=g, device=DEV)
    return (q / q.norm(dim=1, keepdim=True)).contiguous()


def depth_stats(depth):
    c = depth.cpu().numpy()
    return {"min": int(c.min()), "p10": float(np.percentile(c, 10)), "median": float(np.median(c)), "max": int(c.max())}


def run_set(name, x, q, steps, warmup, timing):
    n, d = x.shape
    nq = q.shape[0]
    ix = ops.DescriptorIndex(x, "ND", storage="i8")
    bounds = ix.i8_bounds()
    sc = torch.empty((nq, n), dtype=torch.float32, device=DEV)
    ws = ops._workspace(ops.rank_workspace_bytes(n, nq), DEV)
    out = {"set": name, "per_k": []}
    for K in K_SET:
        ix.scores(q, "ND", out=sc)
        top_ids, top_sc = ops.topk(sc, K, workspace=ws)
        t = top_sc[:, K - 1].contiguous()
        ids, rsc = ops.rescore(x, q, top_ids, "ND")
        depth, _ = ops.rescore_certify(rsc, t, q, bounds, n)
        row = {"K": K, "depth": depth_stats(depth)}
        if timing:
            rs = timed(lambda: ops.rescore(x, q, top_ids, "ND"), steps, warmup)
            ce = timed(lambda: ops.rescore_certify(rsc, t, q, bounds, n), steps, warmup)

            def batch():
                ix.scores(q, "ND", out=sc)
                ti, ts = ops.topk(sc, K, workspace=ws)
                i2, s2 = ops.rescore(x, q, ti, "ND")
                ops.rescore_certify(s2, ts[:, K - 1], q, bounds, n)
            bt = timed(batch, steps, warmup)
            se = timed(lambda: search(ix, x, q, K_SMALL, K, exact=True), max(3, steps // 2), 1)
            res = search(ix, x, q, K_SMALL, K, exact=True)
            gathered = nq * K * d * 4
            row.update({"rescore_ms": stats(rs), "rescore_GBps": round(gathered / (float(np.median(rs)) * 1e-3) / 1e9, 1),
                        "certify_ms": stats(ce), "batch_ms": stats(bt),
                        "batch_queries_per_s": round(nq / (float(np.median(bt)) / 1e3), 1),
                        "search_exact_ms": stats(se), "fallback_share": round(res.fallback.numel() / nq, 4)})
        out["per_k"].append(row)
    if timing:
        f32 = timed(lambda: (ops.scores_rowmajor(x, q, "ND", out=sc), ops.topk(sc, K_SMALL, workspace=ws)), steps, warmup)
        out["f32_batch_ms"] = stats(f32)
        out["f32_batch_queries_per_s"] = round(nq / (float(np.median(f32)) / 1e3), 1)
    ix.close()
    del sc, ws
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--nq", type=int, default=70)
    a = ap.parse_args()
    x = unit_rows(a.n, a.d, 1)
    q = queries(x, a.nq, 2)
    rows = [run_set("random", x, q, a.steps, a.warmup, True)]
    # clustered: 2 000 centres, every row a centre plus noise (in place of the random rows)
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    centres = unit_rows(2000, a.d, 4)
    pick = torch.randint(0, 2000, (a.n,), generator=g, device=DEV)
    for lo in range(0, a.n, 1 << 17):
        hi = min(a.n, lo + (1 << 17))
        x[lo:hi] = centres[pick[lo:hi]] + 0.02 * torch.randn((hi - lo, a.d), generator=g, device=DEV)
        x[lo:hi] /= x[lo:hi].norm(dim=1, keepdim=True)
    q = queries(x, a.nq, 5)
    rows.append(run_set("clustered", x, q, a.steps, a.warmup, False))
    print(json.dumps({"tool": "rescore_bench", "gpu": torch.cuda.get_device_name(0), "n": a.n, "d": a.d, "nq": a.nq,
                      "results": rows}))


if __name__ == "__main__":
    main()
