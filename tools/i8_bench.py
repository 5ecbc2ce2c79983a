#!/usr/bin/env python3
"""The int8 shard (MDX_I8) on one MI355X, one JSON line on stdout (profiles/r10_i8_shard.{json,md}).

Shapes: configs2 = 1 004 993 x 2048 with 70 queries, configs4 = 1 125 x 512 with 1 125 queries (query == database), random
unit rows.  For each, as HIP events (median / min / max over --steps after --warmup):
  build_ms       DescriptorIndex(storage=...) in memory from the caching allocator (i8 / f16 / f32)
  scores_ms      the similarity call (query re-tiling + kernel) on the i8, f16 and f32 shards
  whole_ms       a batch: the similarity + mdx_rank_full, and queries/s from its median
and the top-100 agreement of the i8 (and f16) scores with the fp32 ones: the share of the 100 ids of the fp32 top-100 that
the other top-100 also names, averaged over the queries.  The per-kernel split is rocprofv3's (--kernel-trace --stats
around this tool, in a run of its own).

    python tools/i8_bench.py [--steps 20] [--warmup 3] [--no-1m]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mdir_amd import ops  # noqa: E402
from diffusion_bench import stats, timed, unit_rows  # noqa: E402  (tools/ is sys.path[0])

DEV = "cuda:0"


def agreement(a, b, k=100):
    ia, _ = ops.topk(a, k)
    ib, _ = ops.topk(b, k)
    hit = [np.intersect1d(x, y).size / k for x, y in zip(ia.cpu().numpy(), ib.cpu().numpy())]
    return round(float(np.mean(hit)), 4)


def shape(name, n, d, nq, steps, warmup):
    x = unit_rows(n, d, 1)
    if nq == n:
        q = x
    else:
        g = torch.Generator(device=DEV)
        g.manual_seed(2)
        q = x[torch.arange(0, n, n // nq, device=DEV)[:nq]] + 0.05 * torch.randn((nq, d), generator=g, device=DEV)
        q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    out = {"shape": name, "n": n, "d": d, "nq": nq}
    res = {}
    for storage in ("i8", "f16", "f32"):
        ix = ops.DescriptorIndex(x, "ND", storage=storage)
        build = timed(lambda: ops.DescriptorIndex(x, "ND", storage=storage).close(), max(3, steps // 4), 1)
        sc = torch.empty((nq, n), dtype=torch.float32, device=DEV)
        ws = ops._workspace(ops.rank_workspace_bytes(n, nq), DEV)
        ranks = torch.empty((nq, n), dtype=torch.int64, device=DEV)
        call = timed(lambda: ix.scores(q, "ND", out=sc), steps, warmup)
        batch = timed(lambda: (ix.scores(q, "ND", out=sc), ops.rank_full(sc, out=ranks, workspace=ws)), steps, warmup)
        res[storage] = ix.scores(q, "ND")
        out[storage] = {"device_bytes": ix.device_bytes, "build_ms": stats(build), "scores_ms": stats(call), "whole_ms": stats(batch),
                        "queries_per_s": round(nq / (float(np.median(batch)) / 1e3), 1)}
        ix.close()
        del ws, ranks, sc
        torch.cuda.empty_cache()
    out["top100_agreement_with_f32"] = {"i8": agreement(res["i8"], res["f32"]), "f16": agreement(res["f16"], res["f32"])}
    out["max_abs_diff_with_f32"] = {k: float((res[k] - res["f32"]).abs().max()) for k in ("i8", "f16")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-1m", action="store_true")
    a = ap.parse_args()
    rows = []
    if not a.no_1m:
        rows.append(shape("configs2", 1004993, 2048, 70, a.steps, a.warmup))
        torch.cuda.empty_cache()
    rows.append(shape("configs4", 1125, 512, 1125, a.steps, a.warmup))
    print(json.dumps({"tool": "i8_bench", "gpu": torch.cuda.get_device_name(0), "results": rows}))


if __name__ == "__main__":
    main()
