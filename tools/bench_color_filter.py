#!/usr/bin/env python3
"""GPU: Image.color_filter (crh_image_color_filter: k_image_color_filter, the allocation of the result, the upload of the tables and the wait
included — the call is synchronous) on a random premultiplied image of 1024^2 and 4096^2 (16 bytes per access), 4094 x 4096 (8 bytes) and
4095 x 4096 (4 bytes): a matrix alone (hueRotate 90), tables alone (invert) and both. The cases are interleaved window by window. Beside them,
from the same run and timed the same way, two yardsticks per size: a device-to-device copy of an image of that size (torch; 8 bytes per texel,
as the filter) and Image.composite NORMAL + SRC_OVER of two such images at (0, 0) (12 bytes per texel).
Prints one JSON line per case: {"case", "size", "ms_per_call" (median of --repeats windows of --steps calls), "spread" (max - min of the
windows), "copy_ms", "composite_ms", "windows"}.
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same --only,
--warmup, --steps and --repeats, and prints per case the median time of the kernel alone, of the copy's and the composite's kernels alone,
the ratios and the bytes per second (nothing runs).
Usage: tools/bench_color_filter.py [--steps 10] [--warmup 2] [--repeats 5] [--only 4096_matrix,...] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = (("1024", 1024, 1024), ("4096", 4096, 4096), ("4094", 4094, 4096), ("4095", 4095, 4096))
KINDS = ("matrix", "tables", "both")


def cases_of(only):
    """(name, width, height, kind)"""
    cases = [(f"{shape}_{kind}", w, h, kind) for shape, w, h in SHAPES for kind in KINDS]
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def random_image(w, h, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (h, w, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (h, w, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def from_trace(path, cases, calls):
    """The dispatches in start order. k_image_color_filter: `warmup` per case, case by case, then the windows, interleaved, `steps` per case.
    k_image_composite and the copies (torch's device-to-device copy is the runtime's __amd_rocclr_copyBuffer) the same per size, size by size."""
    found = {"k_image_color_filter": [], "k_image_composite": [], "copyBuffer": []}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key in found:
                if key in row["Kernel_Name"]:
                    found[key].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    warmup, steps, repeats = calls
    shapes = sorted({(c[1], c[2]) for c in cases})

    def medians(entries, n, warm):
        """-> per slot k of n the median duration in us over the windows, or None when the count is not what this tool launches"""
        entries = sorted(entries)
        if len(entries) != n * (warm + steps * repeats):
            return None
        out = []
        for k in range(n):
            timed = []
            for w in range(repeats):
                at = n * warm + (w * n + k) * steps
                timed += [d for _, d in entries[at:at + steps]]
            out.append(float(np.median(timed)) / 1e3)
        return out

    kernel = medians(found["k_image_color_filter"], len(cases), warmup)
    assert kernel is not None, len(found["k_image_color_filter"])
    composite = medians(found["k_image_composite"], len(shapes), warmup)
    # The upload of the tables is a __amd_rocclr_copyBuffer too. The yardstick's copies of window w lie behind the window's last composite and
    # before the next window's first filter: `steps` per size, size by size (another count: the runtime split or merged copies — no figure
    # rather than a wrong one).
    copy = None
    if composite:
        filters, composites, copy_us = sorted(found["k_image_color_filter"]), sorted(found["k_image_composite"]), [[] for _ in shapes]
        for w in range(repeats):
            last = composites[len(shapes) * (warmup + (w + 1) * steps) - 1][0]
            nxt = filters[len(cases) * (warmup + (w + 1) * steps)][0] if w + 1 < repeats else float("inf")
            between = [d for t, d in sorted(found["copyBuffer"]) if last < t < nxt]
            if len(between) == steps * len(shapes):
                for k in range(len(shapes)):
                    copy_us[k] += between[k * steps:(k + 1) * steps]
        if all(copy_us):
            copy = [float(np.median(v)) / 1e3 for v in copy_us]
    for k, (name, width, height, kind) in enumerate(cases):
        us, s = kernel[k], shapes.index((width, height))
        line = {"case": name, "k_image_color_filter_us": round(us, 1), "filter_gb_per_s": round(8.0 * width * height / (us * 1e-6) / 1e9, 1)}
        if copy:
            line.update({"copy_us": round(copy[s], 1), "copy_gb_per_s": round(8.0 * width * height / (copy[s] * 1e-6) / 1e9, 1), "ratio_to_copy": round(us / copy[s], 2)})
        if composite:
            line.update({"k_image_composite_us": round(composite[s], 1), "ratio_to_composite": round(us / composite[s], 2)})
        print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. 4096_matrix")
    ap.add_argument("--from-trace", default=None, help="a rocprofv3 kernel trace (csv) of a run with the same arguments: summarise it")
    args = ap.parse_args()
    cases = cases_of(args.only)
    if args.from_trace:
        from_trace(args.from_trace, cases, (args.warmup, args.steps, args.repeats))
        return
    import torch
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    shapes = sorted({(c[1], c[2]) for c in cases})
    images = {shape: (R.Image(r, random_image(*shape, 7)), R.Image(r, random_image(*shape, 8))) for shape in shapes}
    copies = {(w, h): (torch.randint(0, 255, (w * h * 4,), dtype=torch.uint8, device="cuda"), torch.empty(w * h * 4, dtype=torch.uint8, device="cuda")) for w, h in shapes}
    matrix = R.ColorMatrix.hue_rotate(90)
    tables = np.tile(np.arange(255, -1, -1, dtype=np.uint8), 4)
    arguments = {"matrix": (matrix, None), "tables": (None, tables), "both": (matrix, tables)}

    def color_filter(case):
        _, w, h, kind = case
        images[(w, h)][0].color_filter(*arguments[kind]).destroy()

    def composite(shape):
        backdrop, source = images[shape]
        backdrop.composite(source).destroy()

    def copy(shape):
        src, dst = copies[shape]
        dst.copy_(src)
        torch.cuda.synchronize()

    for case in cases:
        for _ in range(args.warmup):
            color_filter(case)
    for shape in shapes:
        for _ in range(args.warmup):
            composite(shape)
    for shape in shapes:
        for _ in range(max(args.warmup, 1)):
            copy(shape)
    windows = {case[0]: [] for case in cases}
    yardsticks = {(fn, shape): [] for fn in (composite, copy) for shape in shapes}
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case in cases:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                color_filter(case)
            windows[case[0]].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for fn in (composite, copy):
            for shape in shapes:
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn(shape)
                yardsticks[(fn, shape)].append((time.perf_counter() - t0) * 1e3 / args.steps)
    for name, w, h, kind in cases:
        v = sorted(windows[name])
        mid = len(v) // 2
        print(json.dumps({"case": name, "size": [w, h], "ms_per_call": round(v[mid], 4), "spread": round(v[-1] - v[0], 4), "copy_ms": round(sorted(yardsticks[(copy, (w, h))])[mid], 4),
                          "composite_ms": round(sorted(yardsticks[(composite, (w, h))])[mid], 4), "windows": [round(x, 4) for x in windows[name]]}))


if __name__ == "__main__":
    main()
