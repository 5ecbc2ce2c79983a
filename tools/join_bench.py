#!/usr/bin/env python3
"""Exact self-join and range search (mdir_amd/search.py self_join / range_search) on one MI355X, one JSON line on stdout
(profiles/r12_join.{json,md}).

Sets: --n x 2048 random unit rows with planted near-duplicate groups (2 000 groups of 4, noise spread around the
thresholds), and a clustered set (2 000 centres, spread 0.02 per element, as tools/rescore_bench.py).  Per threshold, as HIP
events (median / min / max over --steps after --warmup):
  join_ms        the join kernel over the whole upper triangle (ops.join_candidates, one call: every chunk of rows), and its
                 int8 operations per second against the 5.0 POPS dense I8 figure (2x the ~2.5 PF dense BF16 rate)
  resolve_ms     the exact stage and the ordering alone (ops.join_resolve of every candidate of the upper triangle)
  self_join_ms   search.self_join end to end (join kernel + exact stage + ordering, chunked), candidates and hits
  exact_route    search.self_join(None, ...) at tau = 0.9 on the planted set, whole (the upper triangle: each row block against
                 the rows from its first row on), once, and whether its bits equal the pruned route's
and range_search with 70 queries (database rows plus noise) on both routes.  --range-only runs nothing but 20 pruned
range_search calls (for a kernel trace of that call: rocprofv3 --kernel-trace --stats -- python tools/join_bench.py --range-only).

    python tools/join_bench.py [--steps 3] [--warmup 1] [--n 1004993] [--range-only]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mdir_amd import ops  # noqa: E402
from mdir_amd.search import range_search, self_join  # noqa: E402
from diffusion_bench import stats, timed, unit_rows  # noqa: E402  (tools/ is sys.path[0])

DEV = "cuda:0"
I8_PEAK_OPS = 5.0e15
TAUS = (0.95, 0.9, 0.8)


def planted(n, d, seed, groups=2000):
    x = unit_rows(n, d, seed)
    g = torch.Generator(device=DEV)
    g.manual_seed(seed + 1)
    members = torch.randperm(n, generator=g, device=DEV)[:groups * 4].reshape(groups, 4)
    sigma = 0.05 + 0.6 * torch.rand(groups, 1, 1, generator=g, device=DEV)   # pair cosines ~ 1 / (1 + sigma^2): 0.73 .. 0.998
    noise = torch.randn((groups, 3, d), generator=g, device=DEV)
    noise /= noise.norm(dim=2, keepdim=True)
    v = x[members[:, :1]] + sigma * noise
    x[members[:, 1:]] = v / v.norm(dim=2, keepdim=True)
    return x


def clustered(n, d, seed, centres=2000, spread=0.02):
    c = unit_rows(centres, d, seed)
    g = torch.Generator(device=DEV)
    g.manual_seed(seed + 2)
    x = c[torch.randint(0, centres, (n,), generator=g, device=DEV)] + spread * torch.randn((n, d), generator=g, device=DEV)
    return x / x.norm(dim=1, keepdim=True)


def same_bits(a, b):
    return all(torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)
               for u, v in zip(a, b))


def run_set(name, x, steps, warmup, exact_tau):
    n, d = x.shape
    t_ix = timed(lambda: ops.DescriptorIndex(x, "ND", storage="i8").close(), 1, 1)
    ix = ops.DescriptorIndex(x, "ND", storage="i8")
    st = ops.join_stats(ix, x)
    t_st = timed(lambda: ops.join_stats(ix, x), steps, warmup)
    out = {"set": name, "index_ms": stats(t_ix), "stats_ms": stats(t_st), "per_tau": []}
    ops_total = 2.0 * d * n * (n - 1) / 2
    for tau in TAUS:
        cap = 1 << 24
        _, count = ops.join_candidates(ix, st, ix, st, tau, 0, n, True, cap)
        jt = timed(lambda: ops.join_candidates(ix, st, ix, st, tau, 0, n, True, cap), steps, warmup)
        pairs, _ = ops.join_candidates(ix, st, ix, st, tau, 0, n, True, max(count, 1))
        rs = timed(lambda: ops.join_resolve(x, x, pairs, tau, 0, n), steps, warmup) if count else [0.0]
        res = self_join(ix, x, tau)
        sj = timed(lambda: self_join(ix, x, tau), steps, warmup)
        med = float(np.median(jt))
        row = {"tau": tau, "candidates": int(count), "hits": int(res.ids.numel()),
               "join_ms": stats(jt), "join_TOPS": round(ops_total / (med * 1e-3) / 1e12, 1),
               "join_fraction_of_i8_peak": round(ops_total / (med * 1e-3) / I8_PEAK_OPS, 3),
               "resolve_ms": stats(rs), "self_join_ms": stats(sj)}
        if tau == exact_tau:
            ex = timed(lambda: self_join(None, x, tau), 1, 0)
            row.update({"exact_route_upper_triangle_ms": stats(ex), "routes_bit_equal": same_bits(res, self_join(None, x, tau))})
        out["per_tau"].append(row)
        print(json.dumps({"progress": name, **out["per_tau"][-1]}), file=sys.stderr, flush=True)
    ix.close()
    return out


def range_queries(x, seed=3, nq=70):
    n, d = x.shape
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    q = x[torch.arange(0, n, n // nq, device=DEV)[:nq]] + 0.02 * torch.randn((nq, d), generator=g, device=DEV)
    return (q / q.norm(dim=1, keepdim=True)).contiguous()


def range_block(x, steps, warmup, nq=70, tau=0.9):
    q = range_queries(x, nq=nq)
    ix = ops.DescriptorIndex(x, "ND", storage="i8")
    a = range_search(ix, x, q, tau)
    b = range_search(None, x, q, tau)
    same = same_bits(a, b)
    pr = timed(lambda: range_search(ix, x, q, tau), steps * 5, warmup)
    er = timed(lambda: range_search(None, x, q, tau), steps * 5, warmup)
    ix.close()
    return {"nq": nq, "tau": tau, "hits": int(a.ids.numel()), "routes_bit_equal": bool(same), "pruned_ms": stats(pr),
            "exact_ms": stats(er)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sets", default="planted,clustered")
    ap.add_argument("--range-only", action="store_true")
    args = ap.parse_args()
    if args.range_only:
        x = planted(args.n, args.d, 7)
        ix = ops.DescriptorIndex(x, "ND", storage="i8")
        q = range_queries(x)
        t = timed(lambda: range_search(ix, x, q, 0.9), 20, 3)
        print(json.dumps({"tool": "join_bench", "range_only": True, "pruned_ms": stats(t)}))
        return
    out = {"tool": "join_bench", "n": args.n, "d": args.d, "i8_peak_ops": I8_PEAK_OPS, "sets": []}
    for name in args.sets.split(","):
        x = planted(args.n, args.d, 7) if name == "planted" else clustered(args.n, args.d, 11)
        out["sets"].append(run_set(name, x, args.steps, args.warmup, 0.9 if name == "planted" else None))
        if name == "planted":
            out["range_search"] = range_block(x, args.steps, args.warmup)
        del x
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
