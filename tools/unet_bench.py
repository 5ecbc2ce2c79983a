#!/usr/bin/env python3
"""Time the U-Net generators (mdir_amd/unet.py) on the device: the fused route (library convolutions + mdx_bn_act_into, no
torch.cat) against the module route (MDIR_AMD_FUSED_UNET=0) of the same commit in the same process.

    python tools/unet_bench.py [--out FILE.json] [--rounds 5] [--reps 10] [--labels p2p_unet,outconv_dynint_unet] [--batches 1,8]

Protocol (that of tools/bench_extract.py): every shape is warmed up first; a figure is the time between two device events around
``reps`` calls, divided by ``reps``; the two routes ALTERNATE round by round, and what is printed per route is the median of the
rounds with their min .. max beside it -- the run-to-run spread a difference has to exceed.  Both routes are timed eagerly and as
one hipGraph replay (graphs.ShapeGraphs, as extraction runs them).  Then:

  * the U-Net's share of one extraction step of a SequentialNetwork beside a VGG16 trunk (features + GeM), per pyramid scale the
    label can take (pix2pix needs sides divisible by 2^(levels + 1): scale 1 only; the interpolating label all three);
  * the epilogue alone: mdx_bn_act_into on the first level's map into the lower half of its concat buffer, bytes moved (one
    read + one write per element) over the time per call of back-to-back launches -- an event time, not a profiler's kernel time.

Weights are random (seeded): the time does not depend on them.  Needs an MI355X; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
H, W = 768, 1024
SCALES = (1.0, 2 ** -0.5, 0.5)


def event_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(routes, rounds, reps):
    """``routes``: {name: fn}.  Each round times every route once, in turn; -> {name: (median ms, min ms, max ms)}."""
    for fn in routes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            times[name].append(event_time(fn, reps))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def with_route(net, fused):
    def call(x):
        os.environ["MDIR_AMD_FUSED_UNET"] = "1" if fused else "0"
        try:
            return net(x)
        finally:
            os.environ.pop("MDIR_AMD_FUSED_UNET", None)
    return call


def bench_label(label, batch, rounds, reps):
    from mdir_amd.graphs import ShapeGraphs
    from mdir_amd.network import initialize_model
    torch.manual_seed(0)
    net = initialize_model({"architecture": label, "in_channels": 3, "out_channels": 3}).eval().to(DEV)
    x = torch.randn(batch, 3, H, W, device=DEV)
    fused, plain = with_route(net, True), with_route(net, False)
    with torch.no_grad():
        a, b = fused(x), plain(x)
        diff = float((a - b).abs().max() / b.abs().max())
        eager = alternate({"fused": lambda: fused(x), "module": lambda: plain(x)}, rounds, reps)
        gf, gp = ShapeGraphs(fused, warmup=1), ShapeGraphs(plain, warmup=1)
        for g in (gf, gp):
            g(x)
            g(x)
        graph = alternate({"fused": lambda: gf(x), "module": lambda: gp(x)}, rounds, reps) if gf.graphs and gp.graphs else None
    return {"label": label, "batch": batch, "shape": [batch, 3, H, W], "max_rel_diff": diff, "eager_ms": eager, "graph_ms": graph}


def bench_share(label, rounds, reps):
    """One image, per scale: the generator and a VGG16 trunk (features + GeM + L2N), each as one graph replay where it captures."""
    from mdir_amd.graphs import ShapeGraphs
    from mdir_amd.network import initialize_model
    from mdir_amd.networks import init_network
    torch.manual_seed(0)
    net = initialize_model({"architecture": label, "in_channels": 3, "out_channels": 3}).eval().to(DEV)
    trunk = init_network({"architecture": "vgg16", "pooling": "gem", "whitening": False, "pretrained": False}).eval().to(DEV)
    need = 2 ** (sum(1 for _ in net.modules() if type(_).__name__ == "SkipLevel") + 1) if label != "outconv_dynint_unet" else 1
    rows = []
    with torch.no_grad():
        full = torch.randn(1, 3, H, W, device=DEV)
        for s in SCALES:
            x = full if s == 1.0 else F.interpolate(full, scale_factor=s, mode="bilinear", align_corners=False)
            if x.shape[2] % need or x.shape[3] % need:
                rows.append({"scale": s, "shape": list(x.shape), "skipped": "sides not divisible by %d" % need})
                continue
            gu, gt = ShapeGraphs(net, warmup=1), ShapeGraphs(trunk, warmup=1)
            for g in (gu, gt):
                g(x)
                g(x)
            t = alternate({"unet": lambda: gu(x), "trunk": lambda: gt(x)}, rounds, reps)
            rows.append({"scale": s, "shape": list(x.shape), "unet_ms": t["unet"], "trunk_ms": t["trunk"],
                         "unet_share": t["unet"][0] / (t["unet"][0] + t["trunk"][0]), "graphs": bool(gu.graphs and gt.graphs)})
    done = [r for r in rows if "unet_ms" in r]
    step = sum(r["unet_ms"][0] for r in done), sum(r["trunk_ms"][0] for r in done)
    return {"label": label, "scales": rows, "step_unet_ms": step[0], "step_trunk_ms": step[1], "step_unet_share": step[0] / sum(step)}


def bench_epilogue(batch, rounds, reps):
    from mdir_amd import ops
    c, h, w = 64, H // 2, W // 2                         # the first level's input of every pix2pix label
    x = torch.randn(batch, c, h, w, device=DEV)
    buf = torch.empty(batch, 2 * c, h, w, device=DEV)
    bias = torch.randn(c, device=DEV)
    stats = [torch.randn(c, device=DEV), torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV), bias]
    routes = {
        "bias+leaky into slice": lambda: ops.bn_act_into(x, buf[:, :c], None, None, None, bias, 0.0, ops.ACT_LEAKY, 0.2),
        "bn+relu into slice": lambda: ops.bn_act_into(x, buf[:, c:], *stats, 1e-5, ops.ACT_RELU, 0.0),
        "bias+relu in place": lambda: ops.bn_act_into(x, x, None, None, None, bias, 0.0, ops.ACT_RELU, 0.0),
        "torch: + bias, leaky_relu, cat": lambda: torch.cat([F.leaky_relu(x + bias.view(1, c, 1, 1), 0.2), x], dim=1),
    }
    t = alternate(routes, rounds, max(reps, 50))
    nbytes = 2 * 4 * x.numel()
    return {"shape": list(x.shape), "bytes_moved": nbytes,
            "ms": t, "GB_per_s": {k: nbytes / (v[0] * 1e-3) / 1e9 for k, v in t.items() if not k.startswith("torch")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--labels", default="p2p_unet,outconv_dynint_unet")
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/unet_bench.py needs an MI355X (ROCm) device: nothing is measured without one")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "routes": [], "share": [], "epilogue": []}
    fmt = lambda t: "%.3f ms (%.3f .. %.3f)" % t
    for label in args.labels.split(","):
        for batch in (int(b) for b in args.batches.split(",")):
            r = bench_label(label, batch, args.rounds, args.reps)
            result["routes"].append(r)
            print("%s x%d  eager: fused %s | module %s   graph: %s   max rel diff %.2g" % (
                label, batch, fmt(r["eager_ms"]["fused"]), fmt(r["eager_ms"]["module"]),
                "fused %s | module %s" % (fmt(r["graph_ms"]["fused"]), fmt(r["graph_ms"]["module"])) if r["graph_ms"] else "not captured",
                r["max_rel_diff"]), flush=True)
        s = bench_share(label, args.rounds, args.reps)
        result["share"].append(s)
        print("%s beside a VGG16 trunk, one image: U-Net %.3f ms, trunk %.3f ms over %d scale(s): share %.1f %%" % (
            label, s["step_unet_ms"], s["step_trunk_ms"], sum("unet_ms" in r for r in s["scales"]), 100 * s["step_unet_share"]), flush=True)
    for batch in (int(b) for b in args.batches.split(",")):
        e = bench_epilogue(batch, args.rounds, args.reps)
        result["epilogue"].append(e)
        for k, v in e["ms"].items():
            print("epilogue %s %s: %s%s" % (e["shape"], k, fmt(v), "  %.0f GB/s" % e["GB_per_s"][k] if k in e["GB_per_s"] else ""), flush=True)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
