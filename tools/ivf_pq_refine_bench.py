#!/usr/bin/env python
"""The int8 refinement of IVF-PQ shortlists (IVFPQIndex(..., refine="i8"), include/mdx_refine.h) on one MI355X, in one session and one
process: the database and the partitions of profiles/r21_ivf.md (tools/ivf_bench.py: N = 1 004 993 rows of D = 2048, synthetic and
clustered, the same generator and seeds), M = 64, k = 100, S = 1000, 70 and 2048 queries, the points of profiles/r23_ivf_pq.md --
(lists, nprobe) in {(4096, 8), (4096, 32), (1024, 128)}.

Per partition: a refine=None index that keeps the rows (the parent's fp32 route) and a refine="i8" index with the same codebook;
`nbytes()` of both, with and without the rows.  Per point:
  search   `index.search` in five forms -- ADC alone, refine alone (shortlist=S), refine with rescore=100 and rescore=200, and the fp32
           route (refine=None, shortlist=S) -- by HIP events after a warm-up call, `--calls` calls: median, minimum, maximum; recall@k
           of each against the exact top k.
  stages   the stages of the refine search timed by calling them the way `search` does -- coarse, plan, table, scan, select, quantise,
           refine, rescore (R = 200) -- and, on the same shortlists in the same loop, `ops.rescore` of all S: the stage the refinement
           stands in for.  The refine stage's bytes, nq S (d_pad + 4), over its time.
Per partition also `add` of 65 536 rows and `remove` of 1 % of the ids, with and without the refinement payload, each on a fresh copy
(`from_state`).  Nothing here is a pass mark.  Prints one JSON line and, with --markdown, the tables of profiles/r25_ivf_pq_refine.md."""
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
from ivf_pq_bench import clocked  # noqa: E402

STAGES = ("coarse", "plan", "table", "scan", "select", "quantise", "refine", "rescore", "rescore_all")


def staged_search_refine(index, queries, k, nprobe, shortlist, rescore):
    """`IVFPQIndex.search(..., shortlist, rescore)` on a refine="i8" index that keeps its rows, stage by stage (the same calls on the
    same query chunks), and beside it `ops.rescore` of the whole ADC shortlist ("rescore_all"): ({stage: ms}, ids)."""
    from mdir_amd import ops
    ms = {s: 0.0 for s in STAGES}
    chunk, cap, parts = index.query_chunk(nprobe, shortlist), index.capacity(nprobe), []
    for q0 in range(0, queries.shape[0], chunk):
        block = queries[q0:q0 + chunk]
        (probes, coarse), t = timed(lambda: ops.topk(index.coarse.scores(block, "ND"), nprobe))
        ms["coarse"] += t
        plan, t = timed(lambda: ops.ivf_plan(probes, index.offsets, index.size, cap))
        ms["plan"] += t
        lut, t = timed(lambda: ops.pq_lut(index.codebook.codewords, block, "ND", None))
        ms["table"] += t
        cand, t = timed(lambda: ops.lists_pq_scan(index.codes, index.order, index.n, index.offsets, lut, coarse, probes, plan, cap))
        ms["scan"] += t
        (ids, _), t = timed(lambda: ops.ivf_select(cand[0], cand[1], plan, nprobe, index.lists, shortlist))
        ms["select"] += t
        del cand, plan, lut
        ids = torch.where(ids < 0, index.n, ids)
        (qcodes, qscales), t = timed(lambda: ops.quantize_i8(ops.center_rows(block, "ND", None)))
        ms["quantise"] += t
        (fine_ids, _), t = timed(lambda: ops.refine_i8(index.refine_codes, index.refine_scales, index.d, index.where, qcodes, qscales, ids))
        ms["refine"] += t
        head = fine_ids[:, :rescore].contiguous()
        (sure_ids, _), t = timed(lambda: ops.rescore(index.rows, block, head, "ND", None))
        ms["rescore"] += t
        _, t = timed(lambda: ops.rescore(index.rows, block, ids, "ND", None))
        ms["rescore_all"] += t
        parts.append(torch.where(sure_ids >= index.n, -1, sure_ids)[:, :k])
    return ms, torch.cat(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--points", type=str, nargs="+", default=["4096:8", "4096:32", "1024:128"], help="lists:nprobe")
    ap.add_argument("--nq", type=int, nargs="+", default=[70, 2048])
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--centres", type=int, default=3000)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--train-rows", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pq-train-rows", type=int, default=65536)
    ap.add_argument("--pq-iters", type=int, default=5)
    ap.add_argument("--shortlist", type=int, default=1000)
    ap.add_argument("--rescore", type=int, nargs="+", default=[100, 200])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    from mdir_amd import cluster, ivfpq, ops
    dev = torch.device("cuda:0")
    n, d, k, S, m_sub = args.n, args.d, args.k, args.shortlist, args.m
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
    fresh = draw(args.batch)                                                          # the rows an `add` brings
    say = lambda text: print(text, file=sys.stderr, flush=True)
    rows_bytes = 4 * n * d
    d_pad = (d + 63) // 64 * 64
    line = {"n": n, "d": d, "k": k, "m": m_sub, "shortlist": S, "rescore": args.rescore, "calls": args.calls,
            "device": torch.cuda.get_device_name(0), "builds": {}, "points": {}, "edits": {}}

    exact_ids = {}
    full = ops.DescriptorIndex(rows, "ND")
    for nq, q in queries.items():
        exact_ids[nq] = ops.topk(full.scores(q, "ND"), k)[0]
    full.close()
    del full

    for lists in sorted({p[0] for p in points}, reverse=True):
        torch.cuda.empty_cache()
        fit = cluster.kmeans(rows, lists, iters=args.iters, train_rows=min(n, args.train_rows))
        plain = ivfpq.IVFPQIndex(rows, fit.centroids, fit.labels, m=m_sub, iters=args.pq_iters, train_rows=min(n, args.pq_train_rows))
        fine, build_s = clocked(lambda: ivfpq.IVFPQIndex(rows, fit.centroids, fit.labels, m=m_sub, codebook=plain.codebook, refine="i8"))
        assert torch.equal(fine.codes, plain.codes) and torch.equal(fine.order, plain.order)
        line["builds"][str(lists)] = {
            "build_with_codebook_s": build_s,
            "nbytes": {"plain_without_rows": plain.nbytes() - rows_bytes, "plain_with_rows": plain.nbytes(),
                       "refine_without_rows": fine.nbytes() - rows_bytes, "refine_with_rows": fine.nbytes(),
                       "refine_codes": fine.refine_codes.numel(), "refine_scales": 4 * fine.refine_scales.numel(), "where": 8 * fine.where.numel()}}
        say("lists=%d: %s" % (lists, json.dumps(line["builds"][str(lists)])))
        forms = [("adc", fine, {}), ("refine", fine, {"shortlist": S})]
        forms += [("refine_rescore_%d" % r, fine, {"shortlist": S, "rescore": r}) for r in args.rescore]
        forms += [("fp32_route", plain, {"shortlist": S})]
        for nprobe in [p[1] for p in points if p[0] == lists]:
            for nq, q in queries.items():
                results = {name: index.search(q, k, nprobe, **kw) for name, index, kw in forms}       # the warm-up calls
                staged_search_refine(fine, q, k, nprobe, S, args.rescore[-1])
                torch.cuda.synchronize()
                times = {name: [] for name, _, _ in forms}
                staged = []
                for _ in range(args.calls):
                    for name, index, kw in forms:
                        times[name].append(timed(lambda: index.search(q, k, nprobe, **kw))[1])
                    ms, ids = staged_search_refine(fine, q, k, nprobe, S, args.rescore[-1])
                    assert torch.equal(ids, results["refine_rescore_%d" % args.rescore[-1]].ids)
                    staged.append(ms)
                scanned = results["adc"].scanned.float()
                point = {"scanned_median": float(scanned.median()), "share_of_rows": float(scanned.mean()) / n,
                         "forms": {name: {"search": stats(times[name]), "recall": recall(results[name].ids, exact_ids[nq])} for name, _, _ in forms},
                         "stages": {s: stats([x[s] for x in staged]) for s in STAGES}, "refine_bytes": nq * S * (d_pad + 4),
                         "rescore_all_bytes": nq * S * 4 * d, "query_chunk": fine.query_chunk(nprobe, S)}
                key = "lists=%d nprobe=%d nq=%d" % (lists, nprobe, nq)
                line["points"][key] = point
                say("%s: %s" % (key, json.dumps(point)))
                del results

        # add and remove, with and without the refinement payload, each on a fresh copy that keeps no rows
        edits = {}
        pick = torch.Generator().manual_seed(1)
        gone = torch.randperm(n, generator=pick)[:n // 100].to(dev)
        for name, index in (("plain", plain), ("refine", fine)):
            index.attach_rows(None)
            took = {"add_events_ms": [], "add_host_ms": [], "remove_events_ms": [], "remove_host_ms": []}
            for _ in range(args.calls + 1):                                          # the first call is the warm-up
                for what, call in (("add", lambda c: c.add(fresh)), ("remove", lambda c: c.remove(gone))):
                    copy = ivfpq.IVFPQIndex.from_state(index.state())
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    _, t = timed(lambda: call(copy))
                    took[what + "_host_ms"].append(1e3 * (time.perf_counter() - t0))
                    took[what + "_events_ms"].append(t)
                    assert copy.size == (n + args.batch if what == "add" else n - gone.numel())
                    copy.close()
                    del copy
            edits[name] = {key: stats(v[1:]) for key, v in took.items()}
        line["edits"][str(lists)] = edits
        say("lists=%d edits: %s" % (lists, json.dumps(edits)))
        plain.close(), fine.close()
        del plain, fine, fit
    print(json.dumps(line))
    if args.markdown:
        fmt = lambda s: "%.2f (%.2f .. %.2f)" % (s["median"], s["min"], s["max"])
        print("| lists | refine=None, no rows (MB) | refine=None, rows kept (GB) | refine=\"i8\", no rows (GB) | of that: refine_codes / refine_scales / "
              "where (MB) | refine=\"i8\", rows kept (GB) | build with the codebook given (s) |\n|---|---|---|---|---|---|---|")
        for lists, b in line["builds"].items():
            h = b["nbytes"]
            print("| %s | %.1f | %.2f | %.2f | %.1f / %.1f / %.1f | %.2f | %.2f |" % (
                lists, h["plain_without_rows"] / 1e6, h["plain_with_rows"] / 1e9, h["refine_without_rows"] / 1e9, h["refine_codes"] / 1e6,
                h["refine_scales"] / 1e6, h["where"] / 1e6, h["refine_with_rows"] / 1e9, b["build_with_codebook_s"]))
        names = {"adc": "ADC alone", "refine": "refine=\"i8\", shortlist %d" % S, "fp32_route": "refine=None, shortlist %d (fp32 route)" % S}
        names.update({"refine_rescore_%d" % r: "refine=\"i8\", shortlist %d, rescore %d" % (S, r) for r in args.rescore})
        print("\n| lists | nprobe | nq | form | needs fp32 rows | search ms: median (min .. max) | recall@%d |\n|---|---|---|---|---|---|---|" % k)
        for pkey, p in line["points"].items():
            lists, nprobe, nq = (part.split("=")[1] for part in pkey.split())
            for name, f in p["forms"].items():
                print("| %s | %s | %s | %s | %s | %s | %.4f |" % (lists, nprobe, nq, names[name], "no" if name in ("adc", "refine") else "yes",
                                                                fmt(f["search"]), f["recall"]))
        print("\n| lists | nprobe | nq | coarse | plan | table | scan | select | quantise | refine | rescore of %d | `ops.rescore` of all %d | "
              "refine: GB read | TB/s | `ops.rescore` of all: GB read | TB/s |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"
              % (args.rescore[-1], S))
        for pkey, p in line["points"].items():
            lists, nprobe, nq = (part.split("=")[1] for part in pkey.split())
            st = p["stages"]
            print("| %s | %s | %s | %s | %s | %.2f | %.2f | %.2f | %.2f |" % (
                lists, nprobe, nq, " | ".join("%.2f" % st[s]["median"] for s in STAGES[:6]),
                " | ".join(fmt(st[s]) for s in STAGES[6:]), p["refine_bytes"] / 1e9, p["refine_bytes"] / st["refine"]["median"] / 1e9,
                p["rescore_all_bytes"] / 1e9, p["rescore_all_bytes"] / st["rescore_all"]["median"] / 1e9))
        print("\n| lists | index | `add` of %d rows, ms by HIP events: median (min .. max) | by the host clock | `remove` of %d ids, by HIP events | "
              "by the host clock |\n|---|---|---|---|---|---|" % (args.batch, n // 100))
        for lists, e in line["edits"].items():
            for name, t in e.items():
                print("| %s | %s | %s | %s | %s | %s |" % (lists, "refine=None" if name == "plain" else "refine=\"i8\"", fmt(t["add_events_ms"]),
                                                          fmt(t["add_host_ms"]), fmt(t["remove_events_ms"]), fmt(t["remove_host_ms"])))


if __name__ == "__main__":
    main()
