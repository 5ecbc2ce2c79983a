#!/usr/bin/env python3
"""The exact kNN join (mdir_amd/search.py knn_join: the neighbour lists of DBA and of the diffusion graph) on one MI355X, one JSON
line on stdout (profiles/r13_knn_join.md).

Set: --n x 2048 unit rows in planted groups of 64 (a first row and 63 copies moved by 0.5 times a unit gaussian direction,
normalised: pair cosines around 0.8), k = 50.  Per size, as HIP events (one run each after --warmup runs of the pruned route; the
exact route runs once):
  bounds_ms      ops.knn_bounds of every chunk of rows (the int8 sweep that keeps the k largest lower bounds per row), summed,
                 and its int8 operations per second against the 5.0 POPS dense I8 figure
  candidates_ms  ops.join_candidates_rows of every chunk at the per-row thresholds (the second int8 sweep), likewise
  resolve_ms     ops.knn_resolve of every chunk's candidates (exact chains, ordering, dense top-k)
  knn_join_ms    search.knn_join(index, ...) end to end, candidates per row and pruned_rows
  exact_ms       search.knn_join(None, ...): the chunked scores_rowmajor + topk loop that DBA and DiffusionGraph ran before,
                 and whether its bits equal the pruned route's

    python tools/knn_join_bench.py [--n 200000 1004993] [--k 50] [--warmup 1] [--no-exact]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mdir_amd import ops  # noqa: E402
from mdir_amd.search import knn_join  # noqa: E402
from diffusion_bench import timed, unit_rows  # noqa: E402  (tools/ is sys.path[0])

DEV = "cuda:0"
I8_PEAK_OPS = 5.0e15
CHUNK = 1 << 15


def planted(n, d, seed, group=64, noise=0.5):
    x = unit_rows(n, d, seed)
    g = torch.Generator(device=DEV)
    g.manual_seed(seed + 1)
    groups = n // group
    members = torch.randperm(n, generator=g, device=DEV)[:groups * group].reshape(groups, group)
    step = 1024                                               # groups at a time: the noise of all of them is 8 GB at 1M rows
    for lo in range(0, groups, step):
        m = members[lo:lo + step]
        u = torch.randn((m.shape[0], group - 1, d), generator=g, device=DEV)
        u /= u.norm(dim=2, keepdim=True)
        v = x[m[:, :1]] + noise * u
        x[m[:, 1:]] = v / v.norm(dim=2, keepdim=True)
    return x


def once(fn):
    return round(timed(fn, 1, 0)[0], 3)


def bench(n, d, k, warmup, seed, exact):
    rows = planted(n, d, seed)
    ix = ops.DescriptorIndex(rows, "ND", storage="i8")
    st = ops.join_stats(ix, rows)
    ops_per_sweep = 2.0 * n * n * d
    out = {"n": n, "d": d, "k": k, "chunk": CHUNK}
    for _ in range(warmup):
        knn_join(ix, rows, k)
    bounds = cands = resolve = 0.0
    total = 0
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        box = {}
        bounds += once(lambda: box.__setitem__("t", ops.knn_bounds(ix, st, ix, st, lo, hi, k)))
        cap = max(1 << 20, 4 * k * (hi - lo))
        cands += once(lambda: box.__setitem__("p", ops.join_candidates_rows(ix, st, ix, st, box["t"], lo, hi, cap)))
        pairs, count = box["p"]
        if count > cap:
            pairs, count = ops.join_candidates_rows(ix, st, ix, st, box["t"], lo, hi, count)
        total += count
        resolve += once(lambda: ops.knn_resolve(rows, rows, pairs, lo, hi - lo, k))
        del pairs, box
    out["bounds_ms"] = round(bounds, 2)
    out["bounds_pops"] = round(ops_per_sweep / (bounds * 1e-3) / 1e15, 3)
    out["bounds_of_peak"] = round(ops_per_sweep / (bounds * 1e-3) / I8_PEAK_OPS, 3)
    out["candidates_ms"] = round(cands, 2)
    out["candidates_of_peak"] = round(ops_per_sweep / (cands * 1e-3) / I8_PEAK_OPS, 3)
    out["resolve_ms"] = round(resolve, 2)
    out["candidates_per_row"] = round(total / n, 2)
    box = {}
    out["knn_join_ms"] = once(lambda: box.__setitem__("r", knn_join(ix, rows, k)))
    got = box["r"]
    out["pruned_rows"] = got.pruned_rows
    if exact:
        out["exact_ms"] = once(lambda: box.__setitem__("e", knn_join(None, rows, k)))
        want = box["e"]
        out["same_bits"] = bool(torch.equal(got.ids, want.ids) and torch.equal(got.scores.view(torch.int32), want.scores.view(torch.int32)))
        out["exact_over_pruned"] = round(out["exact_ms"] / out["knn_join_ms"], 2)
    ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[200000, 1004993])
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--no-exact", action="store_true")
    args = ap.parse_args()
    res = {"tool": "knn_join_bench", "device": torch.cuda.get_device_name(0),
           "sets": [bench(n, args.d, args.k, args.warmup, args.seed, not args.no_exact) for n in args.n]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
