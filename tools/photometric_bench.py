#!/usr/bin/env python
"""The photometric input conversions beside each other on one MI355X, in one session: `u8_to_chw`, `clahe_u8_to_chw` (clip 4, grid 8),
`histmatch_u8_to_chw` (`eq` and a registered target) and `gamma_u8_to_chw` (target 0.5) on B uint8 images of H x W (default
8 x 768 x 1024, the block generator of the CLAHE tests with one `dark` factor per image).  HIP events around every call, a warm-up
first, then the median of `--calls` calls with the minimum and the maximum beside it; the calls of the five operators take turns.
Prints one JSON line and, with --markdown, the table of profiles/r18_photometric.md."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def images(b, h, w, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (b, h // 8 + 1, w // 8 + 1, 3))
    img = np.kron(base, np.ones((1, 8, 8, 1)))[:, :h, :w] + rng.normal(0, 12, (b, h, w, 3))
    dark = np.geomspace(1.0, 0.1, b).reshape(-1, 1, 1, 1)
    return np.clip(img * dark, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[8, 768, 1024], metavar=("B", "H", "W"))
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20")
    from mdir_amd import ops
    b, h, w = args.shape
    dev = torch.device("cuda:0")
    u8 = torch.from_numpy(images(b, h, w)).to(dev)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    hist = np.random.default_rng(11).random(256) ** 2
    hist[:5] = 0
    hist[-6:] = 0
    cdf = torch.from_numpy(np.cumsum(hist)).to(dev)
    legs = {"u8_to_chw": lambda: ops.u8_to_chw(u8, mean, std),
            "clahe_u8_to_chw (4, 8)": lambda: ops.clahe_u8_to_chw(u8, 4, 8, mean, std),
            "histmatch eq": lambda: ops.histmatch_u8_to_chw(u8, mean, std),
            "histmatch registered target": lambda: ops.histmatch_u8_to_chw(u8, mean, std, cdf),
            "gamma 0.5": lambda: ops.gamma_u8_to_chw(u8, 0.5, mean, std)}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.calls):                           # in turn: every operator sees the same clocks
        for name, fn in legs.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop))
    _, _, gamma, info = ops.gamma_u8_to_chw(u8, 0.5, mean, std, return_intermediates="solver")
    line = {"shape": [b, h, w], "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
            "ms": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in times.items()},
            "gamma": [round(float(g), 6) for g in gamma.cpu()], "secant_steps": [int(s) for s in info[:, 0].cpu()],
            "fallback": [int(s) for s in info[:, 1].cpu()]}
    clahe = line["ms"]["clahe_u8_to_chw (4, 8)"]["median"]
    line["times_clahe"] = {k: round(v["median"] / clahe, 3) for k, v in line["ms"].items()}
    print(json.dumps(line))
    if args.markdown:
        print("| call (B = %d, %d x %d) | median ms | min | max | x CLAHE |\n|---|---|---|---|---|" % (b, h, w))
        for k, v in line["ms"].items():
            print("| `%s` | %.4f | %.4f | %.4f | %.2f |" % (k, v["median"], v["min"], v["max"], line["times_clahe"][k]))
        print("\ngamma per image %s, secant steps %s, fallback %s" % (line["gamma"], line["secant_steps"], line["fallback"]))


if __name__ == "__main__":
    main()
