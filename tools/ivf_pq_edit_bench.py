#!/usr/bin/env python
"""Adding and removing rows of an IVF-PQ index after the build (IVFPQIndex.add / .remove, include/mdx_lists_edit.h), on one MI355X, in
one session: the database and the partitions of profiles/r21_ivf.md (tools/ivf_bench.py: N = 1 004 993 rows of D = 2048, synthetic and
clustered, the same generator and seeds; 1024 and 4096 lists), M = 64.

Per partition.  The codebook comes from one training build.  Then
  build    the one-shot constructor with that codebook given (labels given, and labels=None: assigned inside), all rows on the device,
           beside the streamed build: the rows wait on the host, the first 65 536 go to the constructor, the others to `add` 65 536 at
           a time, so the device holds the index and one batch.  Of every `add` the host clock and, by HIP events at the seams of the
           call, its split: assignment, members + residuals + encoding, merge, read-back.  `torch.cuda.max_memory_allocated` of each
           build (reset after the rows of that build are where they wait).  Both indexes must search equal.
  merge    the first and the last merge of the streamed build again, `--calls` times each, beside `clone()` of the bytes the merge
           writes (the floor) and the same merge in torch ops (`bucketize` of the positions, `index_copy_`), whose result must be equal.
  remove   `remove` of 1 % random ids and of the largest list, each on a fresh copy of the index (`from_state`).
Nothing here is a pass mark.  Prints one JSON line and, with --markdown, the tables of profiles/r24_ivf_pq_edit.md."""
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
from ivf_pq_bench import clocked  # noqa: E402


def torch_merge(a_rows, a_members, a_offsets, b_rows, b_members, b_offsets):
    """`ops.lists_merge` in torch ops: the list of every source position by `bucketize`, its destination, `index_copy_`."""
    ma, mb = a_rows.shape[0], b_rows.shape[0]
    dev = a_rows.device
    pa, pb = torch.arange(ma, device=dev), torch.arange(mb, device=dev)
    to_a = pa + b_offsets[torch.bucketize(pa, a_offsets[1:], right=True)]              # the rows of b in the lists before
    to_b = pb + a_offsets[torch.bucketize(pb, b_offsets[1:], right=True) + 1]          # the rows of a in the lists up to its own
    rows = torch.empty((ma + mb, a_rows.shape[1]), dtype=a_rows.dtype, device=dev)
    members = torch.empty((ma + mb,), dtype=torch.int64, device=dev)
    rows.index_copy_(0, to_a, a_rows), rows.index_copy_(0, to_b, b_rows)
    members.index_copy_(0, to_a, a_members), members.index_copy_(0, to_b, b_members)
    return rows, members, a_offsets + b_offsets


class Seams:
    """HIP events at the seams of `IVFPQIndex.add`: after the assignment, before and after the merge."""

    def __init__(self):
        from mdir_amd import cluster, ops
        self.cluster, self.ops, self.real = cluster, ops, (cluster.assign, ops.lists_merge)
        self.marks, self.merges, self.keep = {}, [], False

    def mark(self, name):
        self.marks[name] = torch.cuda.Event(enable_timing=True)
        self.marks[name].record()

    def __enter__(self):
        def assign(*args, **kw):
            out = self.real[0](*args, **kw)
            self.mark("assigned")
            return out

        def merge(*args, **kw):
            self.mark("encoded")
            out = self.real[1](*args, **kw)
            self.mark("merged")
            if self.keep:                                                            # the structures of this merge stay alive
                self.merges.append(args)
            return out
        self.cluster.assign, self.ops.lists_merge = assign, merge
        return self

    def __exit__(self, *exc):
        self.cluster.assign, self.ops.lists_merge = self.real
        return False

    def add(self, index, batch):
        """{phase: ms} of one `index.add(batch)`: the host clock around it, and the events between."""
        torch.cuda.synchronize()
        self.mark("start")
        t0 = time.perf_counter()
        index.add(batch)                                                             # ends in its read-back
        host_ms = 1e3 * (time.perf_counter() - t0)
        self.mark("end")
        torch.cuda.synchronize()
        m = self.marks
        return {"host": host_ms, "assign": m["start"].elapsed_time(m["assigned"]), "encode": m["assigned"].elapsed_time(m["encoded"]),
                "merge": m["encoded"].elapsed_time(m["merged"]), "readback": m["merged"].elapsed_time(m["end"])}


def same_search(a, b, queries, k, nprobe):
    for x, y in zip(a.search(queries, k, nprobe), b.search(queries, k, nprobe)):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--nq", type=int, default=70)
    ap.add_argument("--centres", type=int, default=3000)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--train-rows", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pq-train-rows", type=int, default=65536)
    ap.add_argument("--pq-iters", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    from mdir_amd import cluster, ivfpq, ops
    dev = torch.device("cuda:0")
    n, d, m_sub, step = args.n, args.d, args.m, args.batch
    gen = torch.Generator(device=dev).manual_seed(0)
    host = np.random.default_rng(0)
    centres = torch.randn((args.centres, d), generator=gen, device=dev)
    centres /= centres.norm(dim=1, keepdim=True)
    weights = host.dirichlet(np.full(args.centres, 2.0))

    def draw(count):
        """`count` rows: a centre each, normal noise, renormalised; made in pieces (tools/ivf_bench.py)."""
        of = torch.from_numpy(host.choice(args.centres, count, p=weights)).to(dev)
        out = torch.empty((count, d), dtype=torch.float32, device=dev)
        for i0 in range(0, count, 1 << 16):
            piece = centres[of[i0:i0 + (1 << 16)]] + args.noise * torch.randn((min(count, i0 + (1 << 16)) - i0, d), generator=gen, device=dev)
            out[i0:i0 + piece.shape[0]] = piece / piece.norm(dim=1, keepdim=True)
        return out
    rows = draw(n)
    queries = draw(args.nq)
    say = lambda text: print(text, file=sys.stderr, flush=True)
    peak = lambda: torch.cuda.max_memory_allocated(dev)
    line = {"n": n, "d": d, "m": m_sub, "batch": step, "calls": args.calls, "device": torch.cuda.get_device_name(0), "lists": {}}

    parts = {}
    for lists in args.lists:                                                         # everything that needs all rows at once, first
        fit = cluster.kmeans(rows, lists, iters=args.iters, train_rows=min(n, args.train_rows))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        trained, train_s = clocked(lambda: ivfpq.IVFPQIndex(rows, fit.centroids, fit.labels, m=m_sub, iters=args.pq_iters,
                                                            train_rows=min(n, args.pq_train_rows), keep_rows=False))
        report = {"train_build": {"s": train_s, "peak": peak()}}
        book = trained.codebook
        trained.close()
        del trained
        for name, labels in (("labels", fit.labels), ("assigned", None)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            index, secs = clocked(lambda: ivfpq.IVFPQIndex(rows, fit.centroids, labels, m=m_sub, codebook=book, keep_rows=False))
            report["one_shot_" + name] = {"s": secs, "peak": peak(), "nbytes": index.nbytes()}
            if labels is not None:
                index.close()
        parts[lists] = (fit.centroids, book, index, report)                         # the index of labels=None: what `add` has to equal
        say("lists=%d: %s" % (lists, json.dumps(report)))
    waiting = rows.cpu()                                                             # the rows wait on the host
    del rows, fit, index
    torch.cuda.empty_cache()

    for lists, (centroids, book, want, report) in parts.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        held_before = torch.cuda.memory_allocated(dev)
        adds, upload_s = [], 0.0
        with Seams() as seams:
            batch, t = clocked(lambda: waiting[:step].to(dev))
            upload_s += t
            got, first_s = clocked(lambda: ivfpq.IVFPQIndex(batch, centroids, None, m=m_sub, codebook=book, keep_rows=False))
            for i0 in range(step, n, step):
                del batch
                batch, t = clocked(lambda: waiting[i0:i0 + step].to(dev))
                upload_s += t
                seams.keep = i0 == step or i0 + step >= n                             # the first and the last merge, for later
                adds.append(seams.add(got, batch))
            del batch
        report["streamed"] = {"first_batch_s": first_s, "adds": len(adds), "upload_s": upload_s, "peak": peak(), "held_before": held_before,
                              "nbytes": got.nbytes(), **{"%s_s" % key: sum(a[key] for a in adds) / 1e3 for key in adds[0]},
                              "last_add_ms": adds[-1], "first_add_ms": adds[0]}
        report["streamed"]["total_s"] = first_s + report["streamed"]["host_s"]
        for name in ("codes", "order", "offsets"):
            assert torch.equal(getattr(got, name), getattr(want, name)), name
        for k, nprobe in ((100, 8), (100, min(128, lists))):
            same_search(got, want, queries, k, nprobe)
        say("lists=%d streamed: %s" % (lists, json.dumps(report["streamed"])))

        # the first and the last merge again, beside a copy of the same bytes and the merge in torch ops
        report["merge"] = {}
        for which, given in (("first", seams.merges[0]), ("last", seams.merges[-1])):
            ours = ops.lists_merge(*given)
            theirs = torch_merge(*given)
            assert all(torch.equal(x, y) for x, y in zip(ours, theirs))
            torch.cuda.synchronize()
            times = {"kernel": [], "clone": [], "torch": []}
            for _ in range(args.calls):
                times["kernel"].append(timed(lambda: ops.lists_merge(*given))[1])
                times["clone"].append(timed(lambda: [t.clone() for t in ours])[1])
                times["torch"].append(timed(lambda: torch_merge(*given))[1])
            moved = sum(t.numel() * t.element_size() for t in ours)
            report["merge"][which] = {"ma": given[0].shape[0], "mb": given[3].shape[0], "bytes_written": moved,
                                      **{key: stats(v) for key, v in times.items()}}
            del ours, theirs
        seams.merges.clear()
        say("lists=%d merge: %s" % (lists, json.dumps(report["merge"])))

        # removals, each on a fresh copy
        report["remove"] = {}
        pick = torch.Generator().manual_seed(1)
        largest = max(range(lists), key=lambda l: got.host_sizes[l])
        for which, ids in (("one_per_cent", torch.randperm(n, generator=pick)[:n // 100].to(dev)),
                           ("largest_list", got.order[int(got.offsets[largest]):int(got.offsets[largest + 1])].clone())):
            times, host_ms = [], []
            for _ in range(args.calls + 1):                                          # the first call is the warm-up
                copy = ivfpq.IVFPQIndex.from_state(got.state())
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                removed, t = timed(lambda: copy.remove(ids))
                host_ms.append(1e3 * (time.perf_counter() - t0))
                times.append(t)
                assert removed == ids.numel() and copy.size == n - removed and not torch.isin(copy.order, ids).any()
                copy.close()
            report["remove"][which] = {"ids": ids.numel(), "events_ms": stats(times[1:]), "host_ms": stats(host_ms[1:])}
        say("lists=%d remove: %s" % (lists, json.dumps(report["remove"])))
        got.close(), want.close()
        del got, want, seams
        torch.cuda.empty_cache()
        line["lists"][str(lists)] = report
    print(json.dumps(line))
    if args.markdown:
        gb = lambda b: "%.2f" % (b / 1e9)
        fmt = lambda s: "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])
        print("| lists | build | seconds | peak device memory (GB) | nbytes() (MB) |\n|---|---|---|---|---|")
        for lists, r in line["lists"].items():
            s = r["streamed"]
            for name, secs, top, held in (("constructor, trains the codebook", r["train_build"]["s"], r["train_build"]["peak"], None),
                                          ("constructor, codebook and labels given", r["one_shot_labels"]["s"], r["one_shot_labels"]["peak"],
                                           r["one_shot_labels"]["nbytes"]),
                                          ("constructor, codebook given, labels=None", r["one_shot_assigned"]["s"],
                                           r["one_shot_assigned"]["peak"], r["one_shot_assigned"]["nbytes"]),
                                          ("streamed: constructor on %d rows + %d adds (uploads apart: %.1f s)" % (step, s["adds"], s["upload_s"]),
                                           s["total_s"], s["peak"], s["nbytes"])):
                print("| %s | %s | %.2f | %s | %s |" % (lists, name, secs, gb(top), "-" if held is None else "%.1f" % (held / 1e6)))
        print("\n| lists | first batch (s) | adds: host clock (s) | assignment (s) | members, residuals, encoding (s) | merge (s) | read-back (s) | "
              "last add: assignment / encoding / merge / read-back (ms) |\n|---|---|---|---|---|---|---|---|")
        for lists, r in line["lists"].items():
            s, last = r["streamed"], r["streamed"]["last_add_ms"]
            print("| %s | %.2f | %.2f | %.2f | %.2f | %.3f | %.3f | %.1f / %.1f / %.2f / %.2f |" % (
                lists, s["first_batch_s"], s["host_s"], s["assign_s"], s["encode_s"], s["merge_s"], s["readback_s"], last["assign"],
                last["encode"], last["merge"], last["readback"]))
        print("\n| lists | merge | rows a + b | bytes written (MB) | `ops.lists_merge` ms: median (min .. max) | `clone()` of the result | "
              "torch ops (`bucketize`, `index_copy_`) | kernel GB/s written |\n|---|---|---|---|---|---|---|---|")
        for lists, r in line["lists"].items():
            for which, mg in r["merge"].items():
                print("| %s | %s | %d + %d | %.1f | %s | %s | %s | %.0f |" % (
                    lists, which, mg["ma"], mg["mb"], mg["bytes_written"] / 1e6, fmt(mg["kernel"]), fmt(mg["clone"]), fmt(mg["torch"]),
                    mg["bytes_written"] / mg["kernel"]["median"] / 1e6))
        print("\n| lists | removal | ids | `remove` ms by HIP events: median (min .. max) | by the host clock |\n|---|---|---|---|---|")
        for lists, r in line["lists"].items():
            for which, rm in r["remove"].items():
                print("| %s | %s | %d | %s | %s |" % (lists, which.replace("_", " "), rm["ids"], fmt(rm["events_ms"]), fmt(rm["host_ms"])))


if __name__ == "__main__":
    main()
