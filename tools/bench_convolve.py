#!/usr/bin/env python3
"""GPU: Image.convolve (crh_image_convolve: k_image_convolve, the allocation and the wait included — the call is synchronous) on a random
premultiplied image of 4096^2 under BlurEdge.Pad: dense kernels of order 3, 5, 9 and 15 with preserve_alpha off and on, and a sparse 3 x 3
(Sobel, 6 of 9 taps). The cases are interleaved window by window. Beside them, timed the same way in the same run: Image.color_filter with a
matrix on the same image (k_image_color_filter: the streaming kernel that moves the same bytes, the yardstick of the 3 x 3 case) and a
device-to-device copy of the same image (torch, the floor).
Prints one JSON line per case: {"case", "size", "order", "preserve_alpha", "taps" (non-zero), "ms_per_call" (median of --repeats windows of
--steps calls), "spread" (max - min of the windows), "color_filter_ms", "copy_ms", "ratio_to_color_filter", "gmad_per_s" (order^2 * channels
multiply-adds per texel over the whole call), "windows"}.
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same --only,
--warmup, --steps and --repeats, and prints the median time of k_image_convolve per case and of k_image_color_filter instead (nothing runs).
Usage: tools/bench_convolve.py [--size 4096] [--steps 10] [--warmup 2] [--repeats 5] [--only o3,o15_pa,...] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ORDERS = (3, 5, 9, 15)


def dense_kernel(order):
    """A tent: every entry non-zero, entries sum to the divisor (divisor=None)"""
    ramp = np.minimum(np.arange(order) + 1, order - np.arange(order)).astype(np.float64)
    return np.outer(ramp, ramp)


def cases_of(only):
    cases = [(f"o{order}" + ("_pa" if pa else ""), dense_kernel(order), pa) for order in ORDERS for pa in (False, True)]
    cases.append(("o3_sobel", np.array([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]), False))
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def random_image(size, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(64, 256, (size, size, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def from_trace(path, cases, calls):
    """The dispatches of k_image_convolve in start order: `calls` per case, in the order the tool ran the cases (warm-up first, case by case;
    then the windows, interleaved); k_image_color_filter's beside them."""
    rows = {"k_image_convolve": [], "k_image_color_filter": []}
    with open(path) as f:
        for row in csv.DictReader(f):
            for kernel in rows:
                if kernel in row["Kernel_Name"]:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    warmup, steps, repeats = calls
    for found in rows.values():
        found.sort()
    assert len(rows["k_image_convolve"]) == len(cases) * (warmup + steps * repeats), len(rows["k_image_convolve"])
    filter_us = round(float(np.median([d for _, d in rows["k_image_color_filter"][warmup:]])) / 1e3, 1) if rows["k_image_color_filter"] else None
    for k, (name, kernel, pa) in enumerate(cases):
        timed = []
        for w in range(repeats):
            at = len(cases) * warmup + (w * len(cases) + k) * steps
            timed += [d for _, d in rows["k_image_convolve"][at:at + steps]]
        print(json.dumps({"case": name, "k_image_convolve_us": round(float(np.median(timed)) / 1e3, 1), "k_image_color_filter_us": filter_us}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. o3,o15_pa,o3_sobel")
    ap.add_argument("--from-trace", default=None, help="a rocprofv3 kernel trace (csv) of a run with the same arguments: summarise it")
    args = ap.parse_args()
    cases = cases_of(args.only)
    if args.from_trace:
        from_trace(args.from_trace, cases, (args.warmup, args.steps, args.repeats))
        return
    import torch
    from contrast_renderer_amd import BlurEdge, ColorMatrix
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    size = args.size
    image = R.Image(r, random_image(size, 7))
    src, dst = torch.randint(0, 255, (size * size * 4,), dtype=torch.uint8, device="cuda"), torch.empty(size * size * 4, dtype=torch.uint8, device="cuda")
    matrix = ColorMatrix.saturate(0.5)

    def convolve(case):
        image.convolve(case[1], edge=BlurEdge.Pad, preserve_alpha=case[2]).destroy()

    def color_filter(_):
        image.color_filter(matrix).destroy()

    def copy(_):
        dst.copy_(src)
        torch.cuda.synchronize()

    def window(call, what, into):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call(what)
        into.append((time.perf_counter() - t0) * 1e3 / args.steps)

    for case in cases:
        for _ in range(args.warmup):
            convolve(case)
    for _ in range(max(args.warmup, 1)):
        color_filter(None)
        copy(None)
    windows = {case[0]: [] for case in cases}
    filter_windows, copy_windows = [], []
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case in cases:
            window(convolve, case, windows[case[0]])
        window(color_filter, None, filter_windows)
        window(copy, None, copy_windows)
    middle = lambda values: sorted(values)[len(values) // 2]  # noqa: E731
    filter_ms, copy_ms = middle(filter_windows), middle(copy_windows)
    for name, kernel, pa in cases:
        w = sorted(windows[name])
        ms = middle(w)
        order = kernel.shape[0]
        mads = order * order * (3 if pa else 4)
        print(json.dumps({"case": name, "size": size, "order": order, "preserve_alpha": pa, "taps": int(np.count_nonzero(kernel)), "ms_per_call": round(ms, 4), "spread": round(w[-1] - w[0], 4),
                          "color_filter_ms": round(filter_ms, 4), "copy_ms": round(copy_ms, 4), "ratio_to_color_filter": round(ms / filter_ms, 2),
                          "gmad_per_s": round(size * size * mads / (ms * 1e-3) / 1e9, 1), "windows": [round(v, 4) for v in windows[name]]}))


if __name__ == "__main__":
    main()
