#!/usr/bin/env python
"""The int8 lists of the inverted file (mdir_amd/ivf.py, storage="i8") beside the fp32 lists of the same partition and beside
`search.search` on the int8 index of the whole database, on one MI355X, in one session: N = 1 004 993 rows of D = 2048, k = 100,
shortlist 1000, the configurations of profiles/r21_ivf.md -- (lists, nprobe) in {(4096, 8), (4096, 32), (1024, 128)}, nq in {70, 2048}.

The database and the queries are those of tools/ivf_bench.py (synthetic, clustered; the same seeds).  Per point and route: the time of
`index.search` and of its stages, timed by calling them the way `search` does (HIP events, after a warm-up call, `--calls` calls: median,
minimum, maximum) -- coarse, plan, scan, select for the fp32 lists; coarse, plan, quantise (the queries' codes), scan, select, rescore,
certify for the int8 lists; recall@k against the exact top-k; for the int8 lists the share of queries with `certified >= k`; the bytes
each index keeps.  Last, the one condition on speed: where the fp32 scan is bound by its LDS broadcasts (1024 lists, 128 probes, 2048
queries) the int8 scan stage has to be faster than the fp32 scan stage by more than the spread of the fp32 stage's calls.
Prints one JSON line and, with --markdown, the tables of profiles/r22_ivf_i8.md."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ivf_bench import recall, staged_search, stats, timed  # noqa: E402


def staged_search_i8(index, queries, k, nprobe, shortlist):
    """`IVFIndex.search(..., shortlist=S)` of an int8 index stage by stage (the same calls on the same query chunks):
    ({stage: ms}, ids, certified)."""
    from mdir_amd import ops
    ms = {s: 0.0 for s in ("coarse", "plan", "quantise", "scan", "select", "rescore", "certify")}
    chunk, cap, parts, depths = index.query_chunk(nprobe, shortlist), index.capacity(nprobe), [], []
    for q0 in range(0, queries.shape[0], chunk):
        block = queries[q0:q0 + chunk]
        probes, t = timed(lambda: ops.topk(index.coarse.scores(block, "ND"), nprobe)[0])
        ms["coarse"] += t
        plan, t = timed(lambda: ops.ivf_plan(probes, index.offsets, index.n, cap))
        ms["plan"] += t
        (qcodes, qscales), t = timed(lambda: ops.quantize_i8(ops.center_rows(block, "ND", None)))
        ms["quantise"] += t
        cand, t = timed(lambda: ops.lists_i8_scan(index.codes, index.scales, index.d, index.order, index.offsets, qcodes, qscales, plan, nprobe,
                                                  cap, index.items(block.shape[0], nprobe)))
        ms["scan"] += t
        (ids, scores), t = timed(lambda: ops.ivf_select(cand[0], cand[1], plan, nprobe, index.lists, shortlist))
        ms["select"] += t
        scanned = ops.ivf_plan_views(plan, block.shape[0], nprobe, index.lists)["count"].clone()
        del cand, plan
        (sure_ids, sure), t = timed(lambda: ops.rescore(index.rows, block, torch.where(ids < 0, index.n, ids), "ND", None))
        ms["rescore"] += t
        (depth, _), t = timed(lambda: ops.rescore_certify(sure, scores[:, shortlist - 1], block, index.bounds, max(index.n, shortlist), "ND", None))
        ms["certify"] += t
        parts.append(torch.where(sure_ids >= index.n, -1, sure_ids)[:, :k])
        depths.append(torch.where(scanned <= shortlist, shortlist, depth.to(torch.int64)))
    return ms, torch.cat(parts), torch.cat(depths)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--points", type=str, nargs="+", default=["4096:8", "4096:32", "1024:128"], help="lists:nprobe")
    ap.add_argument("--nq", type=int, nargs="+", default=[70, 2048])
    ap.add_argument("--centres", type=int, default=3000)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--train-rows", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--shortlist", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    from mdir_amd import ivf, ops, search
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
    line = {"n": n, "d": d, "k": k, "shortlist": S, "calls": args.calls, "device": torch.cuda.get_device_name(0),
            "query_group": ops.IVF_QUERY_GROUP, "reference": {}, "points": {}}

    exact_ids = {}
    full = ops.DescriptorIndex(rows, "ND")
    for nq, q in queries.items():
        exact_ids[nq] = ops.topk(full.scores(q, "ND"), k)[0]
    full.close()
    del full
    i8 = ops.DescriptorIndex(rows, "ND", storage="i8")
    for nq, q in queries.items():
        search.search(i8, rows, q, k, S)
        times = []
        for _ in range(args.calls):
            res, t = timed(lambda: search.search(i8, rows, q, k, S))
            times.append(t)
        line["reference"]["nq=%d" % nq] = dict(stats(times), recall=recall(res.ids, exact_ids[nq]))
    i8.close()
    del i8

    built = {}
    for lists, nprobe in points:
        if lists not in built:
            for old in built.values():
                old[0].close(), old[1].close()
            built.clear()
            torch.cuda.empty_cache()
            f32 = ivf.IVFIndex.train(rows, lists, train_rows=min(n, args.train_rows), iters=args.iters)
            (low, _) = timed(lambda: ivf.IVFIndex(rows, f32.centroids, f32.labels, storage="i8"))
            built[lists] = (f32, low)
        f32, low = built[lists]
        for nq, q in queries.items():
            want, got = f32.search(q, k, nprobe), low.search(q, k, nprobe, shortlist=S)             # the warm-up calls
            torch.cuda.synchronize()
            whole = {"f32": [], "i8": []}
            stages = {"f32": [], "i8": []}
            for _ in range(args.calls):
                whole["f32"].append(timed(lambda: f32.search(q, k, nprobe))[1])
                ms, ids = staged_search(f32, q, k, nprobe)
                assert torch.equal(ids, want.ids)
                stages["f32"].append(ms)
                whole["i8"].append(timed(lambda: low.search(q, k, nprobe, shortlist=S))[1])
                ms, ids, certified = staged_search_i8(low, q, k, nprobe, S)
                assert torch.equal(ids, got.ids) and torch.equal(certified, got.certified)
                stages["i8"].append(ms)
            sure = (got.certified >= k)
            prefix_ok = bool(((got.ids == want.ids) | ~sure.unsqueeze(1)).all())                    # certified rows are the fp32 rows
            point = {
                "scanned_median": float(got.scanned.float().median()), "share_of_rows": float(got.scanned.float().mean()) / n,
                "f32": {"search": stats(whole["f32"]), "stages": {s: stats([m[s] for m in stages["f32"]]) for s in stages["f32"][0]},
                        "recall": recall(want.ids, exact_ids[nq]), "bytes": rows.numel() * 4},
                "i8": {"search": stats(whole["i8"]), "stages": {s: stats([m[s] for m in stages["i8"]]) for s in stages["i8"][0]},
                       "recall": recall(got.ids, exact_ids[nq]), "certified_share": float(sure.float().mean()), "certified_rows_equal": prefix_ok,
                       "bytes": rows.numel() * 4 + low.codes.numel() + low.scales.numel() * 4},
                "query_chunk": {"f32": f32.query_chunk(nprobe), "i8": low.query_chunk(nprobe, S)}}
            line["points"]["lists=%d nprobe=%d nq=%d" % (lists, nprobe, nq)] = point
            print("lists=%d nprobe=%d nq=%d: %s" % (lists, nprobe, nq, json.dumps(point)), file=sys.stderr, flush=True)
    key = "lists=1024 nprobe=128 nq=2048"
    if key in line["points"]:
        a, b = line["points"][key]["f32"]["stages"]["scan"], line["points"][key]["i8"]["stages"]["scan"]
        line["condition"] = {"f32_scan": a, "i8_scan": b, "f32_spread": a["max"] - a["min"],
                             "met": bool(a["median"] - b["median"] > a["max"] - a["min"] and b["max"] < a["min"])}
    print(json.dumps(line))
    if args.markdown:
        fmt = lambda s: "%.2f (%.2f .. %.2f)" % (s["median"], s["min"], s["max"])
        print("| nq | int8 `search.search`, shortlist %d: median ms (min .. max) | recall@%d |\n|---|---|---|" % (S, k))
        for nq_key, v in line["reference"].items():
            print("| %s | %s | %.4f |" % (nq_key[3:], fmt(v), v["recall"]))
        print("\n| lists | nprobe | nq | route | search ms | coarse | plan | quantise | scan | select | rescore | certify | recall@%d | certified >= k |"
              "\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|" % k)
        for pkey, p in line["points"].items():
            lists, nprobe, nq = (part.split("=")[1] for part in pkey.split())
            for route in ("f32", "i8"):
                r = p[route]
                cells = ["%.2f" % r["stages"][s]["median"] if s in r["stages"] else "-" for s in ("coarse", "plan", "quantise", "scan", "select", "rescore", "certify")]
                print("| %s | %s | %s | %s | %s | %s | %.4f | %s |" % (lists, nprobe, nq, route, fmt(r["search"]), " | ".join(cells), r["recall"],
                                                                       "%.4f" % r["certified_share"] if route == "i8" else "-"))
        print("\nscan stage, median (min .. max) of %d calls:" % args.calls)
        for pkey, p in line["points"].items():
            print("- %s: fp32 %s, int8 %s" % (pkey, fmt(p["f32"]["stages"]["scan"]), fmt(p["i8"]["stages"]["scan"])))
        first = next(iter(line["points"].values()))
        print("\nbytes kept: fp32 lists %.2f GB (the rows); int8 lists %.2f GB (the rows, the codes and the scales)" % (
            first["f32"]["bytes"] / 1e9, first["i8"]["bytes"] / 1e9))
        if "condition" in line:
            print("condition at %s: %s" % (key, json.dumps(line["condition"])))


if __name__ == "__main__":
    main()
