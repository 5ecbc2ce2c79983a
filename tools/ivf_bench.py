#!/usr/bin/env python
"""The inverted file (mdir_amd/ivf.py) on one MI355X, in one session: N = 1 004 993 rows of D = 2048, k = 100, `lists` in {1024, 4096},
`nprobe` in {1, 8, 32, 128}, nq in {70, 2048}.

The database is synthetic and clustered, because recall on unstructured random rows would say nothing: `--centres` unit vectors
(normal, normalised), every row one of them (drawn with Dirichlet(2) weights, so the clusters differ in size) plus normal noise of
`--noise` per coordinate, renormalised; the queries are drawn the same way from the same centres.  The index is
`IVFIndex.train(rows, lists, train_rows=--train-rows, iters=--iters)`.

Per point: the time of `index.search` and of its stages -- coarse (`coarse.scores` + `ops.topk`), plan, scan, select, timed by calling
them the way `search` does -- by HIP events after a warm-up call, the median of `--calls` calls with the minimum and the maximum (a point
whose warm-up took more than `--heavy` seconds is timed once); `scanned` min / median / max; recall@k against the exact top-k.  Per nq, in
the same session: `index.scores` + `ops.topk` on the fp32 index of the rows (the exact top-k itself) and `search.search` on the int8
index with a shortlist of 1000, with its recall.  Prints one JSON line and, with --markdown, the tables of profiles/r21_ivf.md."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def timed(fn):
    """(result, milliseconds) of fn by HIP events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize()
    return out, start.elapsed_time(stop)


def stats(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def staged_search(index, queries, k, nprobe):
    """`IVFIndex.search` stage by stage (the same calls on the same query chunks): ({stage: ms}, ids)."""
    from mdir_amd import ops
    ms = {"coarse": 0.0, "plan": 0.0, "scan": 0.0, "select": 0.0}
    chunk, cap, parts = index.query_chunk(nprobe), index.capacity(nprobe), []
    for q0 in range(0, queries.shape[0], chunk):
        block = queries[q0:q0 + chunk]
        probes, t = timed(lambda: ops.topk(index.coarse.scores(block, "ND"), nprobe)[0])
        ms["coarse"] += t
        plan, t = timed(lambda: ops.ivf_plan(probes, index.offsets, index.n, cap))
        ms["plan"] += t
        cand, t = timed(lambda: ops.ivf_scan(index.rows, index.order, index.offsets, block, plan, nprobe, cap,
                                             index.items(block.shape[0], nprobe)))
        ms["scan"] += t
        out, t = timed(lambda: ops.ivf_select(cand[0], cand[1], plan, nprobe, index.lists, k))
        ms["select"] += t
        parts.append(out[0])
        del cand, plan
    return ms, torch.cat(parts)


def recall(ids, exact_ids):
    """The share of the exact top-k found, averaged over the queries."""
    hit = (ids.unsqueeze(2) == exact_ids.unsqueeze(1)).any(dim=2).float().sum(dim=1)
    return float((hit / exact_ids.shape[1]).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--nq", type=int, nargs="+", default=[70, 2048])
    ap.add_argument("--centres", type=int, default=3000)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--train-rows", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--shortlist", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--heavy", type=float, default=3.0)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    from mdir_amd import ivf, ops, search
    dev = torch.device("cuda:0")
    n, d, k = args.n, args.d, args.k
    gen = torch.Generator(device=dev).manual_seed(0)
    host = np.random.default_rng(0)
    centres = torch.randn((args.centres, d), generator=gen, device=dev)
    centres /= centres.norm(dim=1, keepdim=True)
    weights = host.dirichlet(np.full(args.centres, 2.0))

    def draw(count):
        """`count` rows: a centre each, normal noise, renormalised; made in pieces (no second copy of 8 GB)."""
        of = torch.from_numpy(host.choice(args.centres, count, p=weights)).to(dev)
        out = torch.empty((count, d), dtype=torch.float32, device=dev)
        for i0 in range(0, count, 1 << 16):
            piece = centres[of[i0:i0 + (1 << 16)]] + args.noise * torch.randn((min(count, i0 + (1 << 16)) - i0, d), generator=gen, device=dev)
            out[i0:i0 + piece.shape[0]] = piece / piece.norm(dim=1, keepdim=True)
        return out, of
    rows, row_centre = draw(n)
    sizes = torch.bincount(row_centre, minlength=args.centres).cpu().numpy()
    queries = {nq: draw(nq)[0] for nq in args.nq}
    line = {"n": n, "d": d, "k": k, "centres": args.centres, "noise": args.noise, "train_rows": args.train_rows, "iters": args.iters,
            "calls": args.calls, "device": torch.cuda.get_device_name(0), "query_group": ops.IVF_QUERY_GROUP,
            "centre_sizes": {"min": int(sizes.min()), "median": float(np.median(sizes)), "max": int(sizes.max())}, "reference": {}, "ivf": {}}

    # the two routes that read the whole database, and the exact top-k every recall is measured against
    exact_ids = {}
    full = ops.DescriptorIndex(rows, "ND")
    for nq, q in queries.items():
        ops.topk(full.scores(q, "ND"), k)
        times = []
        for _ in range(args.calls):
            (ids, _), t = timed(lambda: ops.topk(full.scores(q, "ND"), k))
            times.append(t)
        exact_ids[nq] = ids
        line["reference"]["nq=%d" % nq] = {"fp32 scores + topk": stats(times)}
    full.close()
    del full
    i8 = ops.DescriptorIndex(rows, "ND", storage="i8")
    for nq, q in queries.items():
        search.search(i8, rows, q, k, args.shortlist)
        times = []
        for _ in range(args.calls):
            res, t = timed(lambda: search.search(i8, rows, q, k, args.shortlist))
            times.append(t)
        line["reference"]["nq=%d" % nq]["int8 + rescore %d" % args.shortlist] = dict(stats(times), recall=recall(res.ids, exact_ids[nq]))
    i8.close()
    del i8

    for lists in args.lists:
        t0 = time.time()
        index = ivf.IVFIndex.train(rows, lists, train_rows=min(n, args.train_rows), iters=args.iters)
        torch.cuda.synchronize()
        hs = np.array(index.host_sizes)
        entry = {"build_s": time.time() - t0, "list_sizes": {"min": int(hs.min()), "median": float(np.median(hs)), "max": int(hs.max()),
                                                              "empty": int((hs == 0).sum())}, "points": {}}
        for nq, q in queries.items():
            for nprobe in args.nprobe:
                t0 = time.time()
                res = index.search(q, k, nprobe)
                torch.cuda.synchronize()
                warm = time.time() - t0
                calls = args.calls if warm < args.heavy else 1
                whole, stages = [], []
                for _ in range(calls):
                    whole.append(timed(lambda: index.search(q, k, nprobe))[1])
                    ms, ids = staged_search(index, q, k, nprobe)
                    assert torch.equal(ids, res.ids)
                    stages.append(ms)
                scanned = res.scanned.cpu().numpy()
                rows_read = float(scanned.sum())
                entry["points"]["nq=%d nprobe=%d" % (nq, nprobe)] = {
                    "calls": calls, "search": stats(whole), "stages": {s: stats([m[s] for m in stages]) for s in stages[0]},
                    "scanned": {"min": int(scanned.min()), "median": float(np.median(scanned)), "max": int(scanned.max())},
                    "capacity": index.capacity(nprobe), "items_launched": index.items(min(nq, index.query_chunk(nprobe)), nprobe),
                    "query_chunk": index.query_chunk(nprobe), "recall": recall(res.ids, exact_ids[nq]),
                    "scan_gflops": 2e-6 * rows_read * d / np.median([m["scan"] for m in stages])}
                print("lists=%d nq=%d nprobe=%d: %s" % (lists, nq, nprobe, json.dumps(entry["points"]["nq=%d nprobe=%d" % (nq, nprobe)])),
                      file=sys.stderr, flush=True)
        index.close()
        line["ivf"]["lists=%d" % lists] = entry
    print(json.dumps(line))
    if args.markdown:
        fmt = lambda s: "%.2f (%.2f .. %.2f)" % (s["median"], s["min"], s["max"])
        print("| nq | route | median ms (min .. max) | recall@%d |\n|---|---|---|---|" % k)
        for key, v in line["reference"].items():
            for route, s in v.items():
                print("| %s | %s | %s | %s |" % (key[3:], route, fmt(s), "%.4f" % s["recall"] if "recall" in s else "1 (the reference)"))
        print("\n| lists | nq | nprobe | search ms | coarse | plan | scan | select | scanned min / median / max | recall@%d | scan GFLOP/s |"
              "\n|---|---|---|---|---|---|---|---|---|---|---|" % k)
        for lkey, entry in line["ivf"].items():
            for pkey, p in entry["points"].items():
                nq, nprobe = (part.split("=")[1] for part in pkey.split())
                print("| %s | %s | %s | %s | %s | %d / %d / %d | %.4f | %.0f |" % (
                    lkey[6:], nq, nprobe, fmt(p["search"]), " | ".join("%.2f" % p["stages"][s]["median"] for s in ("coarse", "plan", "scan", "select")),
                    p["scanned"]["min"], p["scanned"]["median"], p["scanned"]["max"], p["recall"], p["scan_gflops"]))
        for lkey, entry in line["ivf"].items():
            print("%s: built in %.1f s; list sizes min / median / max %d / %d / %d, %d empty" % (
                lkey, entry["build_s"], entry["list_sizes"]["min"], entry["list_sizes"]["median"], entry["list_sizes"]["max"],
                entry["list_sizes"]["empty"]))


if __name__ == "__main__":
    main()
