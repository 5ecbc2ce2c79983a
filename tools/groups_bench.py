#!/usr/bin/env python3
"""Near-duplicate groups (mdir_amd/search.py duplicate_groups) beside the self-join they consume, on one MI355X: one JSON line
on stdout (profiles/r16_groups.md).  The set and the protocol are tools/join_bench.py's: --n x --d unit rows with 2 000 planted
groups of 4; HIP events around each call, median / min / max over --steps after --warmup, interleaved so that both sides of a
comparison see the same session.

  one_threshold     self_join(ix, x, tau) and duplicate_groups(ix, x, tau) at tau = 0.9, call by call in turn; the groups found;
                    whether the labels equal the components of self_join's own pairs under a host union-find
  union_alone       groups_union_pairs over ALL candidates of the upper triangle at tau = 0.9 in one launch, on a fresh forest
                    (no pair can be skipped at the start), and the label pass
  five_thresholds   duplicate_groups at (0.95, 0.9, 0.85, 0.8, 0.75) in one call beside five self_join calls
  degenerate        --cluster identical rows planted in the set: duplicate_groups at tau = 0.9 -- time, candidates against chains, the
                    largest candidate buffer one call held; --degenerate-self-join also runs self_join there with max_pairs, to see
                    whether it ends (it holds every pair: 12 bytes each and the exact stage's workspace on top)

    python tools/groups_bench.py [--steps 3] [--warmup 1] [--n 1004993] [--cluster 50000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mdir_amd import ops  # noqa: E402
from mdir_amd.search import duplicate_groups, self_join  # noqa: E402
from diffusion_bench import stats, timed  # noqa: E402  (tools/ is sys.path[0])
from join_bench import planted  # noqa: E402

DEV = "cuda:0"
FIVE = (0.95, 0.9, 0.85, 0.8, 0.75)


def host_components(n, i, j):
    """Labels of the components of the edges (i, j) by a sequential union-find (the pairs of a self-join: few)."""
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(i.tolist(), j.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    touched = np.unique(np.concatenate([i, j]))
    for v in touched.tolist():
        parent[v] = find(v)
    return parent


def interleaved(fns, steps, warmup):
    """timed() of several calls, one step of each in turn."""
    out = [[] for _ in fns]
    for s in range(warmup + steps):
        for k, fn in enumerate(fns):
            t = timed(fn, 1, 0)
            if s >= warmup:
                out[k] += t
    return out


def one_threshold(ix, x, tau, steps, warmup):
    n = x.shape[0]
    sj, dg = interleaved([lambda: self_join(ix, x, tau), lambda: duplicate_groups(ix, x, tau)], steps, warmup)
    res, g = self_join(ix, x, tau), duplicate_groups(ix, x, tau)
    i = np.repeat(np.arange(n), np.diff(res.offsets.cpu().numpy()))
    want = host_components(n, i, res.ids.cpu().numpy())
    return {"tau": tau, "self_join_ms": stats(sj), "duplicate_groups_ms": stats(dg), "hits": int(res.ids.numel()),
            "groups": int(g.offsets.numel() - 1), "groups_of_two_or_more": int((g.offsets[1:] - g.offsets[:-1] > 1).sum()),
            "stats": g.stats, "labels_equal_components_of_self_join": bool(np.array_equal(g.labels.cpu().numpy(), want))}


def union_alone(ix, x, tau, steps, warmup):
    n = x.shape[0]
    st = ops.join_stats(ix, x)
    _, count = ops.join_candidates(ix, st, ix, st, tau, 0, n, True, 0)
    pairs, _ = ops.join_candidates(ix, st, ix, st, tau, 0, n, True, max(count, 1))
    forest = {}

    def fresh():
        forest["f"] = ops.groups_init(1, n, x.device)
    un, lb = [], []
    for s in range(warmup + steps):
        fresh()
        t = timed(lambda: ops.groups_union_pairs(x, pairs, tau, *forest["f"]), 1, 0)
        u = timed(lambda: ops.groups_labels(forest["f"][0]), 1, 0)
        if s >= warmup:
            un += t
            lb += u
    return {"tau": tau, "candidates": int(count), "union_pairs_ms": stats(un), "labels_ms": stats(lb), "status": ops.groups_status(forest["f"][1])}


def five_thresholds(ix, x, steps, warmup):
    five, each = interleaved([lambda: duplicate_groups(ix, x, list(FIVE)), lambda: [self_join(ix, x, t) for t in FIVE]], steps, warmup)
    g = duplicate_groups(ix, x, list(FIVE))
    return {"taus": FIVE, "duplicate_groups_ms": stats(five), "five_self_joins_ms": stats(each), "groups": [int(o.numel() - 1) for o in g.offsets],
            "stats": g.stats}


def degenerate(x, cluster, tau, with_self_join, max_pairs):
    n = x.shape[0]
    g = torch.Generator(device=DEV)
    g.manual_seed(16)
    where = torch.randperm(n, generator=g, device=DEV)[:cluster]
    x[where] = x[where[0]].clone()
    ix = ops.DescriptorIndex(x, "ND", storage="i8")
    held = {"pairs": 0}
    real = ops.join_candidates

    def counting(*a, **kw):
        pairs, count = real(*a, **kw)
        held["pairs"] = max(held["pairs"], int(pairs.numel()))
        return pairs, count
    ops.join_candidates = counting
    try:
        t = timed(lambda: duplicate_groups(ix, x, tau), 1, 0)
        res = duplicate_groups(ix, x, tau)
    finally:
        ops.join_candidates = real
    sizes = res.offsets[1:] - res.offsets[:-1]
    out = {"cluster": cluster, "tau": tau, "duplicate_groups_ms": stats(t), "largest_group": int(sizes.max()), "groups": int(sizes.numel()),
           "peak_candidate_bytes": 8 * held["pairs"], "stats": res.stats, "pairs_a_self_join_would_hold": cluster * (cluster - 1) // 2}
    if with_self_join:
        try:
            t = timed(lambda: self_join(ix, x, tau, max_pairs=max_pairs), 1, 0)
            out["self_join"] = {"completed": True, "ms": stats(t)}
        except (ValueError, MemoryError, RuntimeError) as e:
            out["self_join"] = {"completed": False, "error": str(e)[:200]}
    ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tau", type=float, default=0.9)
    ap.add_argument("--cluster", type=int, default=50000, help="identical rows of the degenerate set (0: skip it)")
    ap.add_argument("--degenerate-self-join", action="store_true")
    ap.add_argument("--max-pairs", type=int, default=None)
    ap.add_argument("--only", default="one,union,five,degenerate")
    args = ap.parse_args()
    only = set(args.only.split(","))
    out = {"tool": "groups_bench", "n": args.n, "d": args.d, "steps": args.steps, "warmup": args.warmup}
    x = planted(args.n, args.d, 7)
    ix = ops.DescriptorIndex(x, "ND", storage="i8")
    for name, fn in (("one", lambda: one_threshold(ix, x, args.tau, args.steps, args.warmup)),
                     ("union", lambda: union_alone(ix, x, args.tau, args.steps, args.warmup)),
                     ("five", lambda: five_thresholds(ix, x, args.steps, args.warmup))):
        if name in only:
            out[name] = fn()
            print(json.dumps({"progress": name, **out[name]}), file=sys.stderr, flush=True)
    ix.close()
    if "degenerate" in only and args.cluster > 1:
        out["degenerate"] = degenerate(x, min(args.cluster, args.n), args.tau, args.degenerate_self_join, args.max_pairs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
