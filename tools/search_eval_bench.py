#!/usr/bin/env python
"""The `search` criterion key (mdir_amd/score.py, CirDatasetAp.searched_map) on one MI355X, in one session and one process: what each
route costs in mAP, in recall and in time on the database and the partitions of profiles/r21_ivf.md through r25 (tools/ivf_bench.py:
N = 1 004 993 rows of D = 2048, synthetic and clustered, the same generator and seeds), 70 queries, at depth 100 and 1000.

Ground truth.  rOxford-shaped (bench.py, synth_gnd): per query 5 easy, 10 hard and 5 junk ids, disjoint, drawn among the first 4993
rows, and made relevant the way bench.py plants them -- the labelled row becomes normalise(query + b * N(0, 1)), with b chosen for THIS
database (its rows sit at cos ~0.83 of their centre, so the distractors of a query are its centre's other rows): easy 0.005, junk
0.003, hard 0.0148 (cos ~0.83 to the query) -- the hard ones lie inside the distractors' range, so that mAP < 1 and the depth matters.

Per route and depth: `searched_map` is called `--calls` times (the index is built anew each time, as the key does) and the last call is
reported: mAP E / M / H of the head, the label recall per level, recall@depth against the exact top-depth (`recall: true`,
ops.topk_overlap), and the laps `build_index` and `search` (host clock after a device synchronisation, as the key logs them).  Beside
them the full-ranking mAP (`compute_map_and_print_from_scores` on `scores_rowmajor`) and its time, from the same session.

The overlap kernel: `ops.topk_overlap` of two [nq, 1000] lists at one depth, nq = 70 and 2048, by HIP events after a warm-up call --
the wrapper (with its read-back of the largest id) and the launch alone -- beside the torch formulation, `torch.isin` per row.

Nothing here is a pass mark.  Prints one JSON line and, with --markdown, the tables of profiles/r29_search_eval.md."""
import argparse
import contextlib
import ctypes
import io
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

NQ, LABELLED = 70, 4993
NOISE = (("easy", 0.005), ("hard", 0.0148), ("junk", 0.003))


def synth_gnd():
    """bench.py's synth_gnd: easy 5 / hard 10 / junk 5 disjoint random ids per query among the first 4993 rows."""
    rng = np.random.default_rng(1)
    gnd = []
    for _ in range(NQ):
        ids = rng.choice(LABELLED, size=20, replace=False)
        gnd.append({"easy": np.sort(ids[:5]), "hard": np.sort(ids[5:15]), "junk": np.sort(ids[15:]), "bbx": None})
    return gnd


def plant(rows, queries, gnd):
    """bench.py's plant_positives on this database: every labelled row becomes normalise(query + b * N(0, 1))."""
    gen = torch.Generator(device=rows.device).manual_seed(50_000_000)
    for q, g in enumerate(gnd):
        for key, b in NOISE:
            ids = torch.from_numpy(g[key]).to(rows.device)
            v = queries[q][None, :] + b * torch.randn((len(ids), rows.shape[1]), generator=gen, device=rows.device)
            rows[ids] = v / v.norm(dim=1, keepdim=True)


def routes(depth, points):
    s = min(4 * depth, 4096)
    out = [("exact", {"index": "exact"}), ("i8 shard, shortlist %d" % s, {"index": "i8", "shortlist": s}),
           ("f16 shard, shortlist %d" % s, {"index": "f16", "shortlist": s})]
    for lists, nprobe in points:
        at = "%d lists, %d probes" % (lists, nprobe)
        base = {"lists": lists, "nprobe": nprobe, "iters": 5, "seed": 0}
        out += [("ivf f32, " + at, dict(base, index="ivf", storage="f32")),
                ("ivf i8, " + at, dict(base, index="ivf", storage="i8")),
                ("ivf i8, shortlist %d, %s" % (s, at), dict(base, index="ivf", storage="i8", shortlist=s)),
                ("ivfpq M = 64 (ADC), " + at, dict(base, index="ivfpq")),
                ("ivfpq M = 64, shortlist %d, %s" % (s, at), dict(base, index="ivfpq", shortlist=s)),
                ("ivfpq M = 64, refine i8, shortlist %d, %s" % (s, at), dict(base, index="ivfpq", refine="i8", shortlist=s)),
                ("ivfpq M = 64, refine i8, shortlist %d, rescore %d, %s" % (s, depth, at),
                 dict(base, index="ivfpq", refine="i8", shortlist=s, rescore=depth))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1004993)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--depths", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--points", type=str, nargs="+", default=["4096:8", "4096:32", "1024:128"], help="lists:nprobe")
    ap.add_argument("--centres", type=int, default=3000)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--overlap-nq", type=int, nargs="+", default=[70, 2048])
    ap.add_argument("--overlap-k", type=int, default=1000)
    ap.add_argument("--overlap-calls", type=int, default=20)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    from mdir_amd import _lib, evaluate, ops, score
    dev = torch.device("cuda:0")
    n, d = args.n, args.d
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
    queries = draw(NQ)
    gnd = synth_gnd()
    plant(rows, queries, gnd)
    say = lambda text: print(text, file=sys.stderr, flush=True)
    line = {"n": n, "d": d, "nq": NQ, "calls": args.calls, "device": torch.cuda.get_device_name(0), "noise": dict(NOISE), "full": {},
            "routes": {}, "overlap": {}}
    levels = ("easy", "medium", "hard")

    # the full ranking: scores of every row, positions of the labelled ids (the default path of the criterion)
    took = []
    for _ in range(args.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            avg, _ = evaluate.compute_map_and_print_from_scores("roxford5k", ops.scores_rowmajor(rows, queries, "ND"), gnd)
        torch.cuda.synchronize()
        took.append(time.perf_counter() - t0)
    line["full"] = {"map": {lv: avg["map_" + lv] for lv in levels}, "compute_score_s": took[-1]}
    say("full ranking: %s" % json.dumps(line["full"]))

    obj = score.CirDatasetAp.__new__(score.CirDatasetAp)
    obj.dataset, obj.gnd, obj.database_augmentation, obj.neighbours = "roxford5k", gnd, None, "exact"
    for depth in args.depths:
        for name, search in routes(depth, points):
            obj.search = score._search_params(dict(search, depth=depth, recall=True))
            for _ in range(args.calls):
                laps = {}
                torch.cuda.synchronize()
                t0 = [time.perf_counter()]

                def lap(what):
                    now = time.perf_counter()
                    laps[what], t0[0] = now - t0[0], now
                try:
                    with contextlib.redirect_stdout(io.StringIO()):
                        avg, _ = obj.searched_map(rows, queries, lap=lap)
                except Exception as err:                       # a route that cannot run at this point is reported, not hidden
                    laps = {"error": "%s: %s" % (type(err).__name__, err)}
                    break
                torch.cuda.synchronize()
                lap("evaluate_and_recall")
            if "error" in laps:
                line["routes"]["depth=%d %s" % (depth, name)] = laps
                say("depth=%d %s: %s" % (depth, name, laps["error"]))
                continue
            res = obj.last_search
            point = {"map": {lv: avg["map_" + lv] for lv in levels},
                     "label_recall": {lv: evaluate.label_recall(obj.last_stats[lv]) for lv in levels},
                     "recall_min": float(obj.last_recall.min()), "recall_mean": float(obj.last_recall.mean()), "laps_s": laps,
                     "scanned_median": float(res.scanned.float().median()) if hasattr(res, "scanned") else float(n),
                     "fallback": int(res.fallback.numel()) if hasattr(res, "fallback") else None,
                     "certified_min": int(res.certified.min()) if getattr(res, "certified", None) is not None else None}
            line["routes"]["depth=%d %s" % (depth, name)] = point
            say("depth=%d %s: %s" % (depth, name, json.dumps(point)))
            obj.last_search = obj.last_index = None
            torch.cuda.empty_cache()

    # the overlap kernel beside torch.isin per row
    k = args.overlap_k
    for nq in args.overlap_nq:
        rng = np.random.default_rng(nq)
        a = torch.from_numpy(np.stack([rng.permutation(4 * k)[:k] for _ in range(nq)]).astype(np.int64)).to(dev)
        b = torch.from_numpy(np.stack([rng.permutation(4 * k)[:k] for _ in range(nq)]).astype(np.int64)).to(dev)
        out = torch.empty((nq, 1), dtype=torch.int32, device=dev)
        depths = (ctypes.c_int32 * 1)(k)

        def launch():
            _lib.check(_lib.lib().mdx_topk_overlap(ctypes.c_void_p(a.data_ptr()), k, ctypes.c_void_p(b.data_ptr()), k, nq, depths, 1,
                                                   ctypes.c_void_p(out.data_ptr()), ops._stream()), "mdx_topk_overlap")
            return out

        def by_isin():
            return torch.stack([torch.isin(a[q], b[q]).sum() for q in range(nq)])
        forms = (("wrapper", lambda: ops.topk_overlap(a, b, [k])), ("launch", launch), ("isin_per_row", by_isin))
        want = by_isin().to(torch.int32)
        times = {}
        for name, fn in forms:
            assert torch.equal(fn().reshape(-1), want)          # the warm-up call
            times[name] = stats([timed(fn)[1] for _ in range(args.overlap_calls)])
        line["overlap"]["nq=%d k=%d" % (nq, k)] = times
        say("overlap nq=%d: %s" % (nq, json.dumps(times)))
    print(json.dumps(line))
    if args.markdown:
        pct = lambda m: " / ".join("%.2f" % (100 * m[lv]) for lv in levels)
        print("full ranking: mAP E / M / H %s, compute_score %.3f s\n" % (pct(line["full"]["map"]), line["full"]["compute_score_s"]))
        print("| depth | route | mAP E / M / H of the head | label recall E / M / H (%) | recall@depth: min | mean | scanned rows (median) | "
              "build_index (s) | search (s) | evaluation + recall pass (s) |\n|---|---|---|---|---|---|---|---|---|---|")
        for key, p in line["routes"].items():
            depth, name = key.split(" ", 1)
            if "error" in p:
                print("| %s | %s | not measured: %s |" % (depth.split("=")[1], name, p["error"]))
                continue
            print("| %s | %s | %s | %s | %.4f | %.4f | %d | %.3f | %.3f | %.3f |" % (
                depth.split("=")[1], name, pct(p["map"]), pct(p["label_recall"]), p["recall_min"], p["recall_mean"], p["scanned_median"],
                p["laps_s"]["build_index"], p["laps_s"]["search"], p["laps_s"]["evaluate_and_recall"]))
        fmt = lambda s: "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])
        print("\n| lists | `ops.topk_overlap` (ms): median (min .. max) | `mdx_topk_overlap` alone | `torch.isin` per row |\n|---|---|---|---|")
        for key, t in line["overlap"].items():
            print("| %s | %s | %s | %s |" % (key, fmt(t["wrapper"]), fmt(t["launch"]), fmt(t["isin_per_row"])))


if __name__ == "__main__":
    main()
