#!/usr/bin/env python
"""The approximate kNN join over the inverted file (IVFIndex.knn_join, include/mdx_knn_reverse.h) on one MI355X, in one session and
one process: the database and the partitions of profiles/r21_ivf.md (tools/ivf_bench.py: N = 1 004 993 rows of D = 2048, synthetic and
clustered, the same generator and seed), k = 50, int8 lists, shortlist 200, (lists, nprobe) in {(4096, 8), (4096, 16), (4096, 32), (1024, 32)}.

  exact    the exact route of `search.knn_join(None, rows, k)` on the first `--sample` rows (the rows are independent draws, so these
           are a random sample) -- the same `_ExactKnn` steps at the same chunk -- timed by HIP events and scaled by N / sample;
           its lists are what every recall is measured against.
  pruned   with --pruned: `search.knn_join` on an int8 `DescriptorIndex`, all rows, wall time.
  join     per point `index.knn_join(k, nprobe, shortlist)` with reverse=False (the forward stage) and reverse=True (the total), wall
           time of one call each after the index is built; recall@k of both on the sample; the sum of `gained`.
  merge    on the forward lists of the point: the three launches of `ops.knn_reverse_merge` (count, fill, merge) and the prefix sum
           between them by HIP events, median of `--calls`; the largest offer segment; beside them a `clone()` of the [N, k] pair.
  random   `--random-rows` unit rows without cluster structure (D = `--random-d`), 256 fp32 lists, 8 and 32 probes: recall@k with and
           without the merge against the exact join of all of them.
Nothing here is a pass mark.  Prints one JSON line per section as it goes (so that a run cut short leaves what it measured) and, with
--markdown, the tables of profiles/r26_ivf_knn.md."""
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

from ivf_bench import recall, stats, timed  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.time() - t0) * 1e3


def say(section, entry):
    print(json.dumps({section: entry}), flush=True)


def merge_stages(ids, scores, calls):
    """The stages of ops.knn_reverse_merge on one pair of lists: ({stage: stats of ms}, largest segment, gained sum)."""
    from mdir_amd import ops
    ms = {s: [] for s in ("count", "offsets", "fill", "merge", "clone")}
    for _ in range(calls + 1):                                              # the first round is the warm-up
        counts, t = timed(lambda: ops.knn_reverse_count(ids, scores))
        ms["count"].append(t)
        offsets, t = timed(lambda: ops.knn_reverse_offsets(counts))
        ms["offsets"].append(t)
        offers, t = timed(lambda: ops.knn_reverse_fill(ids, scores, offsets))
        ms["fill"].append(t)
        out, t = timed(lambda: ops.knn_reverse_apply(ids, scores, offsets, offers))
        ms["merge"].append(t)
        _, t = timed(lambda: (ids.clone(), scores.clone()))
        ms["clone"].append(t)
        del offers
    return {s: stats(v[1:]) for s, v in ms.items()}, int(counts.max()), int(offsets[-1]), int(out[2].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--points", type=int, nargs="*", default=[4096, 8, 4096, 16, 4096, 32, 1024, 32], help="lists nprobe lists nprobe ...")
    ap.add_argument("--shortlist", type=int, default=200)
    ap.add_argument("--sample", type=int, default=8192)
    ap.add_argument("--centres", type=int, default=3000)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--train-rows", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--random-rows", type=int, default=131072)
    ap.add_argument("--random-d", type=int, default=256)
    ap.add_argument("--pruned", action="store_true")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    from mdir_amd import ivf, ops, search
    dev = torch.device("cuda:0")
    n, d, k, sample = args.n, args.d, args.k, min(args.sample, args.n)
    gen = torch.Generator(device=dev).manual_seed(0)                        # the database of tools/ivf_bench.py, draw for draw
    host = np.random.default_rng(0)
    centres = torch.randn((args.centres, d), generator=gen, device=dev)
    centres /= centres.norm(dim=1, keepdim=True)
    weights = host.dirichlet(np.full(args.centres, 2.0))
    of = torch.from_numpy(host.choice(args.centres, n, p=weights)).to(dev)
    rows = torch.empty((n, d), dtype=torch.float32, device=dev)
    for i0 in range(0, n, 1 << 16):
        piece = centres[of[i0:i0 + (1 << 16)]] + args.noise * torch.randn((min(n, i0 + (1 << 16)) - i0, d), generator=gen, device=dev)
        rows[i0:i0 + piece.shape[0]] = piece / piece.norm(dim=1, keepdim=True)
    del centres, of
    report = {"n": n, "d": d, "k": k, "shortlist": args.shortlist, "sample": sample, "device": torch.cuda.get_device_name(0)}
    say("setup", report)

    # the exact route on the sample, at the chunk knn_join(None, ...) takes
    chunk = min(search.knn_chunk(n, k), n)
    exact_ids = torch.empty((sample, k), dtype=torch.int64, device=dev)
    exact_sims = torch.empty((sample, k), dtype=torch.float32, device=dev)
    route = search._ExactKnn(rows, k, chunk)
    route.run(0, min(chunk, sample), exact_ids, exact_sims)
    _, t = timed(lambda: route.run(0, sample, exact_ids, exact_sims))
    route.close()
    del route
    report["exact"] = {"chunk": chunk, "sample_ms": t, "scaled_s": t * n / sample / 1e3}
    say("exact", report["exact"])

    report["points"] = {}
    points = list(zip(args.points[::2], args.points[1::2]))
    index, built = None, None
    for lists, nprobe in points:
        if built != lists:
            if index is not None:
                index.close()
            index, build_ms = wall(lambda: ivf.IVFIndex.train(rows, lists, storage="i8", train_rows=min(n, args.train_rows), iters=args.iters))
            built = lists
        entry = {"build_s": build_ms / 1e3, "chunk": min(index.query_chunk(nprobe, args.shortlist), ivf.KNN_JOIN_CHUNK)}
        try:
            forward, entry["forward_ms"] = wall(lambda: index.knn_join(k, nprobe, shortlist=args.shortlist, reverse=False))
            merged, entry["total_ms"] = wall(lambda: index.knn_join(k, nprobe, shortlist=args.shortlist))
        except ValueError as e:                                              # a row with fewer than k candidates: said, not hidden
            entry["refused"] = str(e)
            report["points"]["%d/%d" % (lists, nprobe)] = entry
            say("point %d/%d" % (lists, nprobe), entry)
            continue
        sc = forward.scanned.double()
        entry["scanned"] = {"min": int(sc.min()), "median": float(sc.median()), "max": int(sc.max())}
        entry["recall_forward"] = recall(forward.ids[:sample], exact_ids)
        entry["recall_merged"] = recall(merged.ids[:sample], exact_ids)
        entry["gained"] = int(merged.gained.sum())
        entry["rows_that_gained"] = int((merged.gained > 0).sum())
        del merged
        entry["stages_ms"], entry["largest_segment"], entry["offers"], gained = merge_stages(forward.ids, forward.scores, args.calls)
        assert gained == entry["gained"]
        del forward
        report["points"]["%d/%d" % (lists, nprobe)] = entry
        say("point %d/%d" % (lists, nprobe), entry)
    if index is not None:
        index.close()
    del index

    if args.pruned:
        i8 = ops.DescriptorIndex(rows, "ND", storage="i8")
        res, t = wall(lambda: search.knn_join(i8, rows, k))
        report["pruned"] = {"wall_s": t / 1e3, "pruned_rows": int(res.pruned_rows), "recall": recall(res.ids[:sample], exact_ids)}
        i8.close()
        del i8, res
        say("pruned", report["pruned"])
    del rows

    # rows without cluster structure
    if args.random_rows:
        m = args.random_rows
        flat = torch.randn((m, args.random_d), generator=gen, device=dev)
        flat /= flat.norm(dim=1, keepdim=True)
        truth, t = wall(lambda: search.knn_join(None, flat, k))
        report["random"] = {"rows": m, "d": args.random_d, "lists": 256, "exact_ms": t, "points": {}}
        index = ivf.IVFIndex.train(flat, 256, iters=args.iters)
        for nprobe in (8, 32):
            forward, tf = wall(lambda: index.knn_join(k, nprobe, reverse=False))
            merged, tm = wall(lambda: index.knn_join(k, nprobe))
            report["random"]["points"][str(nprobe)] = {
                "forward_ms": tf, "total_ms": tm, "recall_forward": recall(forward.ids, truth.ids), "recall_merged": recall(merged.ids, truth.ids),
                "gained": int(merged.gained.sum()), "largest_segment": int(ops.knn_reverse_count(forward.ids, forward.scores).max())}
        index.close()
        say("random", report["random"])

    print(json.dumps(report), flush=True)
    if args.markdown:
        print("\n| lists / nprobe | forward ms | total ms | count | prefix sum | fill | merge | clone | recall fwd | recall merged | gained | "
              "largest segment |\n|---|---|---|---|---|---|---|---|---|---|---|---|")
        for name, e in report["points"].items():
            if "refused" in e:
                print("| %s | refused: %s |" % (name, e["refused"]))
                continue
            st = e["stages_ms"]
            print("| %s | %.0f | %.0f | %s | %.4f | %.4f | %d | %d |" % (
                name, e["forward_ms"], e["total_ms"], " | ".join("%.2f" % st[s]["median"] for s in ("count", "offsets", "fill", "merge", "clone")),
                e["recall_forward"], e["recall_merged"], e["gained"], e["largest_segment"]))


if __name__ == "__main__":
    main()
