#!/usr/bin/env python
"""The product-quantised lists of the inverted file (mdir_amd/ivfpq.py) beside the fp32 and the int8 lists of the same partition, on one
MI355X, in one session: N = 1 004 993 rows of D = 2048, k = 100, shortlist 1000, the configurations of profiles/r21_ivf.md and
profiles/r22_ivf_i8.md -- (lists, nprobe) in {(4096, 8), (4096, 32), (1024, 128)}, nq in {70, 2048} -- and M in {32, 64, 128}.

The database and the queries are those of tools/ivf_bench.py (synthetic, clustered; the same seeds).  Per partition and M: the time to
build the index (residuals, `pq.train`, `pq.encode`; a host clock around work that ends in a synchronise) and to build it again with
that codebook given (residuals and `pq.encode` alone), and `nbytes()` with and without the rows.  Per point: the stages of the fp32 and
int8 searches (tools/ivf_bench.py, tools/ivf_i8_bench.py: the same functions, the same session); per M the time of `index.search`
without and with the shortlist and of its stages, timed by calling them the way `search` does (HIP events, after a warm-up call,
`--calls` calls: median, minimum, maximum) -- coarse, plan, table, scan, select, rescore; recall@k of both against the exact top-k and
against the fp32 lists of the same partition and probes.  There is no condition on speed or recall.
Prints one JSON line and, with --markdown, the tables of profiles/r23_ivf_pq.md."""
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

from ivf_bench import recall, staged_search, stats, timed  # noqa: E402
from ivf_i8_bench import staged_search_i8  # noqa: E402


def staged_search_pq(index, queries, k, nprobe, shortlist):
    """`IVFPQIndex.search` stage by stage (the same calls on the same query chunks): ({stage: ms}, ids)."""
    from mdir_amd import ops
    ms = {s: 0.0 for s in ("coarse", "plan", "table", "scan", "select", "rescore")}
    chunk, cap, parts = index.query_chunk(nprobe, shortlist), index.capacity(nprobe), []
    for q0 in range(0, queries.shape[0], chunk):
        block = queries[q0:q0 + chunk]
        (probes, coarse), t = timed(lambda: ops.topk(index.coarse.scores(block, "ND"), nprobe))
        ms["coarse"] += t
        plan, t = timed(lambda: ops.ivf_plan(probes, index.offsets, index.n, cap))
        ms["plan"] += t
        lut, t = timed(lambda: ops.pq_lut(index.codebook.codewords, block, "ND", None))
        ms["table"] += t
        cand, t = timed(lambda: ops.lists_pq_scan(index.codes, index.order, index.n, index.offsets, lut, coarse, probes, plan, cap))
        ms["scan"] += t
        (ids, _), t = timed(lambda: ops.ivf_select(cand[0], cand[1], plan, nprobe, index.lists, k if shortlist is None else shortlist))
        ms["select"] += t
        del cand, plan, lut
        if shortlist is not None:
            (ids, _), t = timed(lambda: ops.rescore(index.rows, block, torch.where(ids < 0, index.n, ids), "ND", None))
            ms["rescore"] += t
            ids = torch.where(ids >= index.n, -1, ids)[:, :k]
        parts.append(ids)
    return ms, torch.cat(parts)


def clocked(fn):
    """(result, seconds) of fn by the host clock, the device drained before and after."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--points", type=str, nargs="+", default=["4096:8", "4096:32", "1024:128"], help="lists:nprobe")
    ap.add_argument("--nq", type=int, nargs="+", default=[70, 2048])
    ap.add_argument("--m", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--centres", type=int, default=3000)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--train-rows", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pq-train-rows", type=int, default=65536)
    ap.add_argument("--pq-iters", type=int, default=5)
    ap.add_argument("--shortlist", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    from mdir_amd import ivf, ivfpq, ops
    dev = torch.device("cuda:0")
    n, d, k, S = args.n, args.d, args.k, args.shortlist
    points = [tuple(int(x) for x in p.split(":")) for p in args.points]
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
    queries = {nq: draw(nq) for nq in args.nq}
    say = lambda text: print(text, file=sys.stderr, flush=True)
    line = {"n": n, "d": d, "k": k, "shortlist": S, "calls": args.calls, "device": torch.cuda.get_device_name(0),
            "pq_train_rows": args.pq_train_rows, "pq_iters": args.pq_iters, "builds": {}, "points": {}}

    exact_ids = {}
    full = ops.DescriptorIndex(rows, "ND")
    for nq, q in queries.items():
        exact_ids[nq] = ops.topk(full.scores(q, "ND"), k)[0]
    full.close()
    del full

    for lists in sorted({p[0] for p in points}, reverse=True):
        torch.cuda.empty_cache()
        f32 = ivf.IVFIndex.train(rows, lists, train_rows=min(n, args.train_rows), iters=args.iters)
        low = ivf.IVFIndex(rows, f32.centroids, f32.labels, storage="i8")
        say("lists=%d: partition and int8 lists built" % lists)
        coded = {}
        for m in args.m:
            index, whole = clocked(lambda: ivfpq.IVFPQIndex(rows, f32.centroids, f32.labels, m=m, iters=args.pq_iters,
                                                            train_rows=min(n, args.pq_train_rows)))
            again, encode = clocked(lambda: ivfpq.IVFPQIndex(rows, f32.centroids, f32.labels, m=m, codebook=index.codebook, keep_rows=False))
            assert torch.equal(again.codes, index.codes)
            held = {"with_rows": index.nbytes(), "without_rows": again.nbytes(), "codes": index.codes.numel(), "ids": 8 * n,
                    "codebook": 4 * index.codebook.codewords.numel(), "coarse": index.coarse.device_bytes}
            again.close()
            del again
            coded[m] = index
            line["builds"]["lists=%d m=%d" % (lists, m)] = {"train_and_encode_s": whole, "encode_s": encode, "train_s": whole - encode,
                                                            "pq_updates": index.codebook.iterations, "nbytes": held}
            say("lists=%d m=%d: %s" % (lists, m, json.dumps(line["builds"]["lists=%d m=%d" % (lists, m)])))
        for nprobe in [p[1] for p in points if p[0] == lists]:
            for nq, q in queries.items():
                want, got8 = f32.search(q, k, nprobe), low.search(q, k, nprobe, shortlist=S)           # the warm-up calls
                torch.cuda.synchronize()
                whole = {"f32": [], "i8": []}
                stages = {"f32": [], "i8": []}
                for _ in range(args.calls):
                    whole["f32"].append(timed(lambda: f32.search(q, k, nprobe))[1])
                    stages["f32"].append(staged_search(f32, q, k, nprobe)[0])
                    whole["i8"].append(timed(lambda: low.search(q, k, nprobe, shortlist=S))[1])
                    stages["i8"].append(staged_search_i8(low, q, k, nprobe, S)[0])
                point = {"scanned_median": float(want.scanned.float().median()), "share_of_rows": float(want.scanned.float().mean()) / n}
                for route, res in (("f32", want), ("i8", got8)):
                    point[route] = {"search": stats(whole[route]), "stages": {s: stats([x[s] for x in stages[route]]) for s in stages[route][0]},
                                    "recall": recall(res.ids, exact_ids[nq])}
                for m, index in coded.items():
                    adc, sure = index.search(q, k, nprobe), index.search(q, k, nprobe, shortlist=S)   # the warm-up calls
                    torch.cuda.synchronize()
                    assert torch.equal(adc.probes, want.probes) and torch.equal(adc.scanned, want.scanned)
                    times = {"adc": [], "shortlist": []}
                    staged = {"adc": [], "shortlist": []}
                    for _ in range(args.calls):
                        for name, short, res in (("adc", None, adc), ("shortlist", S, sure)):
                            times[name].append(timed(lambda: index.search(q, k, nprobe, shortlist=short))[1])
                            ms, ids = staged_search_pq(index, q, k, nprobe, short)
                            assert torch.equal(ids, res.ids)
                            staged[name].append(ms)
                    point["pq m=%d" % m] = {
                        name: {"search": stats(times[name]), "stages": {s: stats([x[s] for x in staged[name]]) for s in staged[name][0]},
                               "recall": recall(res.ids, exact_ids[nq]), "recall_vs_f32_lists": recall(res.ids, want.ids)}
                        for name, res in (("adc", adc), ("shortlist", sure))}
                    point["pq m=%d" % m]["query_chunk"] = {"adc": index.query_chunk(nprobe), "shortlist": index.query_chunk(nprobe, S)}
                key = "lists=%d nprobe=%d nq=%d" % (lists, nprobe, nq)
                line["points"][key] = point
                say("%s: %s" % (key, json.dumps(point)))
        for index in coded.values():
            index.close()
        f32.close(), low.close()
        del coded, f32, low
    print(json.dumps(line))
    if args.markdown:
        fmt = lambda s: "%.2f (%.2f .. %.2f)" % (s["median"], s["min"], s["max"])
        print("| lists | M | build: residuals, train, encode (s) | with the codebook given: residuals, encode (s) | codeword updates | "
              "nbytes() without rows (MB) | codes | ids | codebook | coarse index | nbytes() with rows (GB) |\n|---|---|---|---|---|---|---|---|---|---|---|")
        for bkey, b in line["builds"].items():
            lists, m = (part.split("=")[1] for part in bkey.split())
            h = b["nbytes"]
            print("| %s | %s | %.1f | %.1f | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f |" % (
                lists, m, b["train_and_encode_s"], b["encode_s"], b["pq_updates"], h["without_rows"] / 1e6, h["codes"] / 1e6, h["ids"] / 1e6,
                h["codebook"] / 1e6, h["coarse"] / 1e6, h["with_rows"] / 1e9))
        print("\n| lists | nprobe | nq | route | search ms: median (min .. max) | coarse | plan | quantise / table | scan | select | rescore | certify | "
              "recall@%d | recall@%d against the fp32 lists |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|" % (k, k))
        for pkey, p in line["points"].items():
            lists, nprobe, nq = (part.split("=")[1] for part in pkey.split())
            routes = [("fp32 lists", p["f32"]), ("int8 lists, shortlist %d" % S, p["i8"])]
            for m in args.m:
                routes += [("PQ M=%d, ADC" % m, p["pq m=%d" % m]["adc"]), ("PQ M=%d, shortlist %d" % (m, S), p["pq m=%d" % m]["shortlist"])]
            for name, r in routes:
                st = r["stages"]
                prep = st.get("quantise", st.get("table"))
                cells = ["%.2f" % st[s]["median"] if s in st and (s != "rescore" or st[s]["max"] > 0) else "-"
                         for s in ("coarse", "plan")] + ["%.2f" % prep["median"] if prep else "-"]
                cells += ["%.2f" % st[s]["median"] if s in st and (s != "rescore" or st[s]["max"] > 0) else "-"
                          for s in ("scan", "select", "rescore", "certify")]
                print("| %s | %s | %s | %s | %s | %s | %.4f | %s |" % (lists, nprobe, nq, name, fmt(r["search"]), " | ".join(cells), r["recall"],
                                                                       "%.4f" % r["recall_vs_f32_lists"] if "recall_vs_f32_lists" in r else "-"))
        print("\nscan stage, median (min .. max) of %d calls:" % args.calls)
        for pkey, p in line["points"].items():
            print("- %s: fp32 %s, int8 %s, %s" % (pkey, fmt(p["f32"]["stages"]["scan"]), fmt(p["i8"]["stages"]["scan"]), ", ".join(
                "PQ M=%d %s (table %s)" % (m, fmt(p["pq m=%d" % m]["adc"]["stages"]["scan"]), fmt(p["pq m=%d" % m]["adc"]["stages"]["table"]))
                for m in args.m)))


if __name__ == "__main__":
    main()
