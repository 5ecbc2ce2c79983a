#!/usr/bin/env python
"""The trainable tail beside the reference's op sequence on one MI355X, in one session: `autograd.PoolL2N` forward plus backward
(GeM p = 3 and p = 2.92) on 2048 x 24 x 32 and 512 x 48 x 64 maps, both tuple losses with their backward at D = 2048, N = 7 and
N = 35, and one `training.tuple_step` of ResNet101 on 7 images of 362 x 362.  The baseline of every leg is the same computation
written in plain torch ops (tests/train_restatement.py, the torch half: what the reference's layers do) on the same device; the
step's baseline shares the trunk and swaps only the tail and the loss.  HIP events around every call, a warm-up first, then the
median of `--calls` calls with the minimum and the maximum beside it; the legs take turns.  `--count-launches` counts the device kernels
of one call of every leg with torch.profiler instead (null where it gives no device events).  Prints one JSON line and, with
--markdown, the table of profiles/r19_train_tail.md."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def launches(fn):
    """Device kernels of one call, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-calls", type=int, default=5, help="calls of the ResNet101 tuple step (0: leave it out)")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--count-launches", action="store_true", help="count the kernels of every leg with torch.profiler instead of timing")
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20")
    import train_restatement as TR
    from mdir_amd import autograd, criterion, training
    from mdir_amd.networks import init_network
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    legs = {}
    for c, h, w in ((2048, 24, 32), (512, 48, 64)):
        x = torch.from_numpy((rng.random((1, c, h, w), dtype=np.float32) * (rng.random((1, c, h, w), dtype=np.float32) > 0.5))).to(dev)
        go = torch.randn(1, c, device=dev)
        for p in (3.0, 2.92):
            def hip(x=x, go=go, p=p):
                xr, pr = x.detach().requires_grad_(True), torch.tensor([p], device=dev, requires_grad=True)
                autograd.PoolL2N.apply(xr, pr, "gem", 1e-6, 1e-6).backward(go)

            def base(x=x, go=go, p=p):
                xr, pr = x.detach().requires_grad_(True), torch.tensor([p], device=dev, requires_grad=True)
                TR.tail_torch(xr, "gem", pr, 1e-6, 1e-6).backward(go)
            legs["PoolL2N gem p=%g fwd+bwd %dx%dx%d" % (p, c, h, w)] = (hip, base)
    for n, nq in ((7, 1), (35, 5)):
        cols = rng.standard_normal((2048, n))
        cols = torch.from_numpy((cols / np.linalg.norm(cols, axis=0) * rng.uniform(0.3, 0.8, n)).astype(np.float32)).to(dev)
        label = torch.tensor([-1.0, 1.0, 0, 0, 0, 0, 0] * nq, device=dev)
        for name, mod, fn in (("contrastive", criterion.ContrastiveLoss(), TR.contrastive_torch), ("triplet", criterion.TripletLoss(), TR.triplet_torch)):
            def hip(cols=cols, label=label, mod=mod):
                mod(cols.detach().requires_grad_(True), label).backward()

            def base(cols=cols, label=label, fn=fn):
                fn(cols.detach().requires_grad_(True), label).backward()
            legs["%s loss+bwd D=2048 N=%d" % (name, n)] = (hip, base)
    for _ in range(args.warmup):
        for hip, base in legs.values():
            hip()
            base()
    torch.cuda.synchronize()
    if args.count_launches:
        print(json.dumps({"launches": {k: {"hip": launches(hip), "torch": launches(base)} for k, (hip, base) in legs.items()}}))
        return

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)
    times = {k: ([], []) for k in legs}
    for _ in range(args.calls):                           # in turn: every leg sees the same clocks
        for name, (hip, base) in legs.items():
            times[name][0].append(timed(hip))
            times[name][1].append(timed(base))
    if args.step_calls > 0:
        torch.manual_seed(0)
        net = init_network({"architecture": "resnet101", "pooling": "gem", "whitening": True, "pretrained": False}).to(dev)
        net.train()
        net.apply(training.set_batchnorm_eval)
        images = [torch.rand(1, 3, 362, 362, device=dev) for _ in range(7)]
        target = torch.tensor([-1.0, 1.0, 0, 0, 0, 0, 0])
        crit = criterion.ContrastiveLoss()

        def hip_step():
            net.zero_grad(set_to_none=True)
            training.tuple_step(net, crit, images, target)

        def base_step():
            net.zero_grad(set_to_none=True)
            cols = [TR.tail_torch(net.features(im), "gem", net.pool.p, net.pool.eps, net.norm.eps, net.whiten.weight, net.whiten.bias).t()
                    for im in images]
            loss = TR.contrastive_torch(torch.cat(cols, dim=1), target.to(dev))
            loss.backward()
            float(loss.detach())
        name = "tuple_step ResNet101, 7 x 362 x 362"
        times[name] = ([], [])
        for _ in range(2):
            hip_step()
            base_step()
        for _ in range(args.step_calls):
            times[name][0].append(timed(hip_step))
            times[name][1].append(timed(base_step))

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    line = {"calls": args.calls, "warmup": args.warmup, "step_calls": args.step_calls, "device": torch.cuda.get_device_name(0),
            "ms": {k: {"hip": stats(a), "torch": stats(b)} for k, (a, b) in times.items()}}
    print(json.dumps(line))
    if args.markdown:
        print("| leg | HIP tail median ms (min .. max) | torch ops median ms (min .. max) |\n|---|---|---|")
        for k, v in line["ms"].items():
            print("| %s | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) |" % (
                k, v["hip"]["median"], v["hip"]["min"], v["hip"]["max"], v["torch"]["median"], v["torch"]["min"], v["torch"]["max"]))


if __name__ == "__main__":
    main()
