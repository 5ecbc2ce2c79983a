#!/usr/bin/env python
"""The graph index (mdir_amd/graph.py, include/mdx_graph.h) on one MI355X, in one session and one process: the database and the partition
of profiles/r21_ivf.md (tools/ivf_bench.py: N = 1 004 993 rows of D = 2048, synthetic and clustered, the same generator and seed), k = 100.

  build    the lists from `IVFNeighbours` (4096 int8 lists, 16 probes, shortlist 200, reverse merge) at k = k0 + 1; `ops.graph_detours`;
           the rest of `graph.optimise` (the torch sorts and gathers); wall time of one call each.  Beside the detours a `clone()` of
           their output bytes, by HIP events, median of `--rounds`.
  search   for every nq and every (beam, width, seeds, entries) of the grid, `index.search(q, k, ...)` by HIP events after a warm-up
           call: median and min .. max of `--rounds` rounds in which all routes take turns; recall@k from `search.recall_at` against
           the exact top-k; `steps` and `scored` per query.
  stages   per graph route, in rounds of their own: the seeds' scan (`index.seeds_of`) and the walk alone (`ops.graph_search` on those
           seeds), and two variants of the walk that move its parts: every query a copy of query 0 (all workgroups read the same rows,
           so all but the first find them in the caches), and the first 64 of the D columns only (the rows in place at the same
           stride: a 32 times shorter chain and gather, the same selection, table and merge sort per step).
  ivf      the competing routes in the same rounds: `IVFIndex.search` on fp32 lists at 4096 / 8 and 4096 / 32, and on int8 lists with
           shortlist 1000 at 4096 / 8.
Nothing here is a pass mark.  Prints one JSON line per section as it goes and, with --markdown, the tables of profiles/r30_graph.md;
--out writes the JSON report to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ivf_bench import stats, timed  # noqa: E402

GRID = ((128, 1, 8, "sample"), (128, 1, 8, "medoids"), (128, 2, 8, "medoids"), (128, 4, 16, "medoids"), (256, 1, 8, "medoids"),
        (256, 4, 16, "medoids"), (512, 8, 16, "medoids"))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.time() - t0) * 1e3


def say(section, entry):
    print(json.dumps({section: entry}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--k0", type=int, default=64)
    ap.add_argument("--nq", type=int, nargs="+", default=[70, 2048])
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--shortlist", type=int, default=200)
    ap.add_argument("--centres", type=int, default=3000)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--train-rows", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    from mdir_amd import cluster, graph, ivf, ops, search
    dev = torch.device("cuda:0")
    n, d, k = args.n, args.d, args.k
    gen = torch.Generator(device=dev).manual_seed(0)                        # the database of tools/ivf_bench.py, draw for draw
    host = np.random.default_rng(0)
    centres = torch.randn((args.centres, d), generator=gen, device=dev)
    centres /= centres.norm(dim=1, keepdim=True)
    weights = host.dirichlet(np.full(args.centres, 2.0))

    def draw(count):
        of = torch.from_numpy(host.choice(args.centres, count, p=weights)).to(dev)
        out = torch.empty((count, d), dtype=torch.float32, device=dev)
        for i0 in range(0, count, 1 << 16):
            piece = centres[of[i0:i0 + (1 << 16)]] + args.noise * torch.randn((min(count, i0 + (1 << 16)) - i0, d), generator=gen, device=dev)
            out[i0:i0 + piece.shape[0]] = piece / piece.norm(dim=1, keepdim=True)
        return out
    rows = draw(n)
    queries = {nq: draw(nq) for nq in args.nq}
    report = {"n": n, "d": d, "k": k, "degree": args.degree, "k0": args.k0, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    say("setup", report)

    full = ops.DescriptorIndex(rows, "ND")
    exact_ids = {nq: ops.topk(full.scores(q, "ND"), k)[0] for nq, q in queries.items()}
    full.close()
    del full

    # ---- build
    lists = min(args.lists, n)
    km, t_kmeans = wall(lambda: cluster.kmeans(rows, lists, train_rows=min(n, args.train_rows), iters=args.iters))
    i8, t_i8 = wall(lambda: ivf.IVFIndex(rows, km.centroids, km.labels, storage="i8"))
    handle = ivf.IVFNeighbours(i8, min(args.nprobe, lists), shortlist=args.shortlist)
    (ids, _), t_lists = wall(lambda: handle.lists_of(rows, args.k0 + 1))
    stripped, t_strip = wall(lambda: graph.strip_self(ids))
    del ids
    det, t_det = wall(lambda: ops.graph_detours(stripped))
    det_ms, clone_ms = [], []
    for _ in range(args.rounds):
        det_ms.append(timed(lambda: ops.graph_detours(stripped))[1])
        clone_ms.append(timed(lambda: det.clone())[1])
    edges, t_rest = wall(lambda: graph.optimise(stripped, args.degree, detours=det))
    del stripped, det
    entries = {"sample": graph.GraphIndex._sample(n, 1024, 0, dev)}
    entries["medoids"], t_medoids = wall(lambda: graph.medoids(rows, km.centroids, km.labels))
    report["build"] = {"kmeans_s": t_kmeans / 1e3, "ivf_i8_lists_s": t_i8 / 1e3, "knn_lists_s": t_lists / 1e3, "strip_self_ms": t_strip,
                       "detours_first_call_ms": t_det, "detours_ms": stats(det_ms), "clone_of_detours_ms": stats(clone_ms),
                       "rest_ms": t_rest, "medoids_ms": t_medoids, "medoids": int(entries["medoids"].shape[0]),
                       "graph_bytes": edges.numel() * 4, "valid_edges": int((edges >= 0).sum())}
    say("build", report["build"])
    indexes = {name: graph.GraphIndex(rows, edges, e) for name, e in entries.items()}

    # ---- the routes, taking turns
    f32 = ivf.IVFIndex(rows, km.centroids, km.labels, storage="f32")
    routes = {}
    for beam, width, seeds, ent in GRID:
        if beam < k:
            continue
        routes["graph beam %d width %d seeds %d %s" % (beam, width, seeds, ent)] = \
            (lambda q, b=beam, w=width, s=seeds, e=ent: indexes[e].search(q, k, beam=b, width=w, seeds=s))
    routes["ivf f32 %d / 8" % lists] = lambda q: f32.search(q, k, min(8, lists))
    routes["ivf f32 %d / 32" % lists] = lambda q: f32.search(q, k, min(32, lists))
    routes["ivf i8 %d / 8 shortlist 1000" % lists] = lambda q: i8.search(q, k, min(8, lists), shortlist=1000)
    report["search"] = {}
    for nq, q in queries.items():
        ms, last = {name: [] for name in routes}, {}
        for name, fn in routes.items():                                      # the warm-up round
            fn(q)
        for _ in range(args.rounds):
            for name, fn in routes.items():
                last[name], t = timed(lambda: fn(q))
                ms[name].append(t)
        table = {}
        for name, res in last.items():
            row = {"ms": stats(ms[name]), "recall": float(np.mean(search.recall_at(res.ids, exact_ids[nq], k)[:, 0]))}
            if hasattr(res, "steps"):
                row["steps"] = float(res.steps.double().mean())
                row["scored"] = float(res.scored.double().mean())
            else:
                row["scanned"] = float(res.scanned.double().mean())
            table[name] = row
        report["search"]["nq=%d" % nq] = table
        say("search nq=%d" % nq, table)
        # the parts of the graph routes
        same = q[:1].expand(nq, d).contiguous()
        short_rows, short_q = rows[:, :min(64, d)], q[:, :min(64, d)].contiguous()
        parts = {}
        for beam, width, seeds, ent in GRID:
            if beam < k:
                continue
            index = indexes[ent]
            sd = index.seeds_of(q, seeds)
            sd_same = sd[:1].expand(nq, sd.shape[1]).contiguous()
            calls = {"seeds": lambda: index.seeds_of(q, seeds),
                     "walk": lambda: ops.graph_search(rows, edges, q, sd, k, beam, width),
                     "walk, one query copied": lambda: ops.graph_search(rows, edges, same, sd_same, k, beam, width),
                     "walk, 64 columns": lambda: ops.graph_search(short_rows, edges, short_q, sd, k, beam, width)}
            ms, steps = {name: [] for name in calls}, {}
            for r in range(args.rounds + 1):                                 # the first round is the warm-up
                for name, fn in calls.items():
                    out, t = timed(fn)
                    ms[name].append(t)
                    if name != "seeds":
                        steps[name] = float(out[2].double().mean())
            parts["graph beam %d width %d seeds %d %s" % (beam, width, seeds, ent)] = \
                {name: dict(stats(v[1:]), **({"steps": steps[name]} if name in steps else {})) for name, v in ms.items()}
        report.setdefault("stages", {})["nq=%d" % nq] = parts
        say("stages nq=%d" % nq, parts)
    for index in indexes.values():
        index.close()
    f32.close()
    i8.close()

    print(json.dumps(report), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    if args.markdown:
        b = report["build"]
        print("\n| stage | time |\n|---|---|")
        for key in ("kmeans_s", "ivf_i8_lists_s", "knn_lists_s"):
            print("| %s | %.2f s |" % (key[:-2], b[key]))
        for key in ("strip_self_ms", "rest_ms", "medoids_ms"):
            print("| %s | %.1f ms |" % (key[:-3], b[key]))
        for key in ("detours_ms", "clone_of_detours_ms"):
            print("| %s | %.2f (%.2f .. %.2f) ms |" % (key[:-3], b[key]["median"], b[key]["min"], b[key]["max"]))
        for nq_name, table in report["search"].items():
            print("\n%s\n\n| route | median ms (min .. max) | recall@%d | steps | scored or scanned per query |\n|---|---|---|---|---|" % (nq_name, k))
            for name, row in table.items():
                print("| %s | %.2f (%.2f .. %.2f) | %.4f | %s | %.0f |" % (
                    name, row["ms"]["median"], row["ms"]["min"], row["ms"]["max"], row["recall"],
                    "%.1f" % row["steps"] if "steps" in row else "", row.get("scored", row.get("scanned", 0))))
        for nq_name, parts in report["stages"].items():
            print("\n%s, median ms (steps per query)\n\n| route | seeds | walk | walk, one query copied | walk, 64 columns |\n|---|---|---|---|---|" % nq_name)
            for name, row in parts.items():
                print("| %s | %.2f | %s |" % (name, row["seeds"]["median"], " | ".join(
                    "%.2f (%.1f)" % (row[c]["median"], row[c]["steps"]) for c in ("walk", "walk, one query copied", "walk, 64 columns"))))


if __name__ == "__main__":
    main()
