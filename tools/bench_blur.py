#!/usr/bin/env python3
"""GPU: Image.blur (crh_image_blur: k_image_blur_h + k_image_blur_v, allocation, tap upload and the wait included — the call is synchronous) on
random premultiplied images of 1024^2 and 4096^2, sigma 2, 8, 32 and 64 on both axes, BlurEdge.Pad and BlurEdge.Transparent. The cases are
interleaved window by window. Beside each case: a device-to-device copy of the same image (torch, the floor a memory-bound blur would approach)
timed the same way.
Prints one JSON line per case: {"case", "size", "sigma", "edge", "radius", "out_size", "ms_per_call" (median of --repeats windows of --steps
calls), "spread" (max - min of the windows), "copy_ms", "gmacs_per_s"}: taps x texels x 4 channels per second of the whole call, the horizontal
pass counted with (2 R + 1) x out_w x h x 4 and the vertical with (2 R + 1) x out_w x out_h x 4 multiply-adds.
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same --only,
--warmup, --steps and --repeats, and prints the median time of each kernel per case instead (nothing runs).
Usage: tools/bench_blur.py [--steps 10] [--warmup 2] [--repeats 5] [--only 4096_s64_pad,...] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SIZES = (1024, 4096)
SIGMAS = (2.0, 8.0, 32.0, 64.0)
EDGES = (("pad", 1), ("transparent", 0))


def cases_of(only):
    cases = [(f"{size}_s{int(sigma)}_{name}", size, sigma, edge) for size in SIZES for sigma in SIGMAS for name, edge in EDGES]
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def random_image(size, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(64, 256, (size, size, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def macs(size, radius, grown):
    out = size + 2 * radius if grown else size
    return (2 * radius + 1) * 4 * (out * size + out * out)


def from_trace(path, cases, calls):
    """The dispatches of the two kernels in start order: `calls` of each per case, in the order the tool ran the cases (warm-up first, case by
    case; then the windows, interleaved)."""
    rows = {"k_image_blur_h": [], "k_image_blur_v": []}
    with open(path) as f:
        for row in csv.DictReader(f):
            for kernel in rows:
                if kernel in row["Kernel_Name"]:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    warmup, steps, repeats = calls
    for kernel, found in rows.items():
        found.sort()
        assert len(found) == len(cases) * (warmup + steps * repeats), (kernel, len(found))
    for k, (name, size, sigma, edge) in enumerate(cases):
        line = {"case": name}
        for kernel, found in rows.items():
            timed = []
            for w in range(repeats):
                at = len(cases) * warmup + (w * len(cases) + k) * steps
                timed += [d for _, d in found[at:at + steps]]
            line[kernel + "_us"] = round(float(np.median(timed)) / 1e3, 1)
        radius = int(np.ceil(3.0 * sigma))
        line["kernels_gmacs_per_s"] = round(macs(size, radius, edge == 0) / ((line["k_image_blur_h_us"] + line["k_image_blur_v_us"]) * 1e-6) / 1e9, 1)
        print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. 4096_s64_pad")
    ap.add_argument("--from-trace", default=None, help="a rocprofv3 kernel trace (csv) of a run with the same arguments: summarise it")
    args = ap.parse_args()
    cases = cases_of(args.only)
    if args.from_trace:
        from_trace(args.from_trace, cases, (args.warmup, args.steps, args.repeats))
        return
    import torch
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    images = {size: R.Image(r, random_image(size, 7)) for size in SIZES if any(c[1] == size for c in cases)}
    copies = {size: (torch.randint(0, 255, (size * size * 4,), dtype=torch.uint8, device="cuda"), torch.empty(size * size * 4, dtype=torch.uint8, device="cuda")) for size in images}

    def blur(case):
        _, size, sigma, edge = case
        out = images[size].blur(sigma, sigma, edge)
        shape = (out.width, out.height)
        out.destroy()
        return shape

    def copy(size):
        src, dst = copies[size]
        dst.copy_(src)
        torch.cuda.synchronize()

    shapes = {}
    for case in cases:
        for _ in range(args.warmup):
            shapes[case[0]] = blur(case)
    for size in images:
        for _ in range(max(args.warmup, 1)):
            copy(size)
    windows = {case[0]: [] for case in cases}
    copy_windows = {size: [] for size in images}
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case in cases:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                blur(case)
            windows[case[0]].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for size in images:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                copy(size)
            copy_windows[size].append((time.perf_counter() - t0) * 1e3 / args.steps)
    for name, size, sigma, edge in cases:
        w = sorted(windows[name])
        ms = w[len(w) // 2]
        radius = int(np.ceil(3.0 * sigma))
        print(json.dumps({"case": name, "size": size, "sigma": sigma, "edge": "transparent" if edge == 0 else "pad", "radius": radius, "out_size": list(shapes.get(name, ())),
                          "ms_per_call": round(ms, 4), "spread": round(w[-1] - w[0], 4), "copy_ms": round(sorted(copy_windows[size])[len(w) // 2], 4),
                          "gmacs_per_s": round(macs(size, radius, edge == 0) / (ms * 1e-3) / 1e9, 1), "windows": [round(v, 4) for v in windows[name]]}))


if __name__ == "__main__":
    main()
