#!/usr/bin/env python
"""One iteration of spherical k-means (mdir_amd/cluster.py) beside the same iteration written in torch ops, on one MI355X, in one
session: N = 1 004 993 unit rows of D = 2048, K = 256 and K = 4096.  The library's iteration is timed stage by stage -- scores
(`DescriptorIndex.scores` into the reused block, all chunks), argmax (`ops.kmeans_argmax`, all chunks), ordering (the stable sort and
the offsets), sums (`ops.kmeans_sums`) and finish (`ops.kmeans_finish`) -- and the torch iteration likewise: `mm` and `argmax` on the
same chunks, `index_add_` of the rows into the sums, and the normalisation.  HIP events around every stage, a warm-up first, then the
median of `--calls` iterations with the minimum and the maximum beside it; the two sides take turns.  The torch side accumulates with
floating-point atomics: `--calls` runs of it are also compared with each other, and the number of distinct results is reported.
Prints one JSON line and, with --markdown, the table of profiles/r20_kmeans.md."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


class Stages:
    """Accumulates the milliseconds of named stages of one iteration from HIP events."""

    def __init__(self):
        self.pending = []

    def run(self, name, fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        self.pending.append((name, start, stop))
        return out

    def collect(self):
        torch.cuda.synchronize()
        ms = {}
        for name, start, stop in self.pending:
            ms[name] = ms.get(name, 0.0) + start.elapsed_time(stop)
        self.pending = []
        ms["total"] = sum(ms.values())
        return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--compute", default="chain")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    from mdir_amd import cluster, ops
    dev = torch.device("cuda:0")
    n, d = args.n, args.d
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = torch.empty((n, d), dtype=torch.float32, device=dev)
    for i0 in range(0, n, 1 << 16):                       # unit rows, made in pieces: no second copy of 8 GB
        piece = torch.randn((min(n, i0 + (1 << 16)) - i0, d), generator=gen, device=dev)
        rows[i0:i0 + piece.shape[0]] = piece / piece.norm(dim=1, keepdim=True)
    del piece
    line = {"n": n, "d": d, "calls": args.calls, "warmup": args.warmup, "compute": args.compute, "device": torch.cuda.get_device_name(0),
            "segment": ops.KMEANS_SEGMENT, "ms": {}}
    for k in args.k:
        cents = rows.index_select(0, torch.randperm(n, generator=torch.Generator().manual_seed(k))[:k].to(dev))
        chunk = cluster.assign_chunk(n, k, d, args.compute)
        block = torch.empty((chunk, k), dtype=torch.float32, device=dev)
        labels = torch.empty(n, dtype=torch.int64, device=dev)
        best = torch.empty(n, dtype=torch.float32, device=dev)
        index = ops.DescriptorIndex(cents, "ND")
        st = Stages()

        def ours():
            for i0 in range(0, n, chunk):
                i1 = min(n, i0 + chunk)
                sc = st.run("scores", lambda: index.scores(rows[i0:i1], "ND", out=block[:i1 - i0], compute=args.compute))
                st.run("argmax", lambda: ops.kmeans_argmax(sc, out_labels=labels[i0:i1], out_best=best[i0:i1]))
            members, offsets, _ = st.run("ordering", lambda: cluster._members(labels, k))
            sums = st.run("sums", lambda: ops.kmeans_sums(rows, members, offsets, k))
            return st.run("finish", lambda: ops.kmeans_finish(sums, 1e-6, previous=cents))

        def theirs():
            ct = cents.t()
            for i0 in range(0, n, chunk):
                i1 = min(n, i0 + chunk)
                sc = st.run("mm", lambda: torch.mm(rows[i0:i1], ct, out=block[:i1 - i0]))
                st.run("argmax", lambda: torch.argmax(sc, dim=1, out=labels[i0:i1]))
            sums = st.run("index_add_", lambda: torch.zeros((k, d), device=dev).index_add_(0, labels, rows))
            return st.run("normalise", lambda: sums / (sums.norm(dim=1, keepdim=True) + 1e-6))

        for _ in range(args.warmup):
            ours(), theirs()
            st.collect()
        times = {"hip": [], "torch": []}
        distinct = {"hip": set(), "torch": set()}
        for _ in range(args.calls):                       # in turn: both sides see the same clocks
            for side, fn in (("hip", ours), ("torch", theirs)):
                out = fn()
                times[side].append(st.collect())
                distinct[side].add(hash(out.cpu().numpy().tobytes()))
        index.close()

        def stats(side):
            return {name: {"median": float(np.median([t[name] for t in times[side]])), "min": float(np.min([t[name] for t in times[side]])),
                           "max": float(np.max([t[name] for t in times[side]]))} for name in times[side][0]}
        line["ms"]["K=%d" % k] = {"chunk": chunk, "hip": stats("hip"), "torch": stats("torch"),
                                  "distinct_results": {side: len(v) for side, v in distinct.items()}}
        del block, labels, best, cents
    print(json.dumps(line))
    if args.markdown:
        print("| K | side | stage | median ms (min .. max) |\n|---|---|---|---|")
        for key, v in line["ms"].items():
            for side in ("hip", "torch"):
                for name, s in v[side].items():
                    print("| %s | %s | %s | %.3f (%.3f .. %.3f) |" % (key[2:], side, name, s["median"], s["min"], s["max"]))
        for key, v in line["ms"].items():
            print("K = %s: chunk %d rows; distinct centroid results over %d calls: library %d, torch ops %d"
                  % (key[2:], v["chunk"], args.calls, v["distinct_results"]["hip"], v["distinct_results"]["torch"]))


if __name__ == "__main__":
    main()
