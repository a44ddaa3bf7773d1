#!/usr/bin/env python3
"""GPU: Image.composite (crh_image_composite: k_image_composite, the allocation of the result and the wait included — the call is synchronous)
on two random premultiplied images of 1024^2 and 4096^2: NORMAL + SRC_OVER, MULTIPLY + SRC_OVER and HARD_LIGHT + SRC_ATOP at opacity 0.6, the
source at (0, 0) and at (3, 5). Behind them the access-width variants of the kernel at NORMAL + SRC_OVER: 4096 wide with the source at (4, 5)
(16 bytes per access on both sides, shifted), 4094 wide (8 bytes) and 4095 wide (4 bytes). The cases are interleaved window by window. Beside
each case: a device-to-device copy of an image of the same size (torch; it moves 8 bytes per texel where the composite moves 12) timed the same way.
Prints one JSON line per case: {"case", "size", "mode", "op", "offset", "ms_per_call" (median of --repeats windows of --steps calls), "spread"
(max - min of the windows), "copy_ms", "windows"}.
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same --only,
--warmup, --steps and --repeats, and prints per case the median time of the kernel alone, of the copy's kernel alone, their ratio and the
bytes per second both move (nothing runs).
Usage: tools/bench_composite.py [--steps 10] [--warmup 2] [--repeats 5] [--only 4096_normal_over_0,...] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SIZES = (1024, 4096)
COMBOS = (("normal_over", 0, 3), ("multiply_over", 1, 3), ("hardlight_atop", 6, 9))  # (name, crh_blend_mode, crh_composite_op)
OFFSETS = (("0", (0, 0)), ("35", (3, 5)))
VARIANTS = (("4096_normal_over_45", 4096, 4096, (4, 5)), ("4094_normal_over_0", 4094, 4096, (0, 0)), ("4095_normal_over_0", 4095, 4096, (0, 0)))
OPACITY = 0.6


def cases_of(only):
    """(name, width, height, mode, op, offset)"""
    cases = [(f"{size}_{combo}_{off}", size, size, mode, op, offset) for size in SIZES for combo, mode, op in COMBOS for off, offset in OFFSETS]
    cases += [(name, w, h, 0, 3, offset) for name, w, h, offset in VARIANTS]
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def random_image(w, h, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (h, w, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (h, w, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def from_trace(path, cases, calls):
    """The dispatches of k_image_composite in start order: `warmup` per case, case by case, then the windows, interleaved, `steps` per case. The
    copies of a window (torch's device-to-device copy is the runtime's __amd_rocclr_copyBuffer) lie between the window's last composite and the next
    window's first: `steps` per size, size by size."""
    kernel, copies = [], []
    with open(path) as f:
        for row in csv.DictReader(f):
            entry = (int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
            if "k_image_composite" in row["Kernel_Name"]:
                kernel.append(entry)
            elif "copyBuffer" in row["Kernel_Name"]:
                copies.append(entry)
    warmup, steps, repeats = calls
    kernel.sort()
    copies.sort()
    assert len(kernel) == len(cases) * (warmup + steps * repeats), len(kernel)
    shapes = sorted({(c[1], c[2]) for c in cases})
    copy_us = {shape: [] for shape in shapes}
    for w in range(repeats):
        last = kernel[len(cases) * warmup + (w + 1) * len(cases) * steps - 1][0]
        nxt = kernel[len(cases) * warmup + (w + 1) * len(cases) * steps][0] if w + 1 < repeats else float("inf")
        found = [d for t, d in copies if last < t < nxt]
        if len(found) == steps * len(shapes):  # (otherwise the runtime split or merged copies: no figure rather than a wrong one)
            for k, shape in enumerate(shapes):
                copy_us[shape] += found[k * steps:(k + 1) * steps]
    for k, (name, width, height, mode, op, offset) in enumerate(cases):
        timed = []
        for w in range(repeats):
            at = len(cases) * warmup + (w * len(cases) + k) * steps
            timed += [d for _, d in kernel[at:at + steps]]
        us = float(np.median(timed)) / 1e3
        line = {"case": name, "k_image_composite_us": round(us, 1), "composite_gb_per_s": round(12.0 * width * height / (us * 1e-6) / 1e9, 1)}
        if copy_us[(width, height)]:
            c = float(np.median(copy_us[(width, height)])) / 1e3
            line.update({"copy_us": round(c, 1), "copy_gb_per_s": round(8.0 * width * height / (c * 1e-6) / 1e9, 1), "ratio_to_copy": round(us / c, 2)})
        print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. 4096_normal_over_0")
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

    def composite(case):
        _, w, h, mode, op, offset = case
        backdrop, source = images[(w, h)]
        backdrop.composite(source, op, mode, OPACITY, offset).destroy()

    def copy(shape):
        src, dst = copies[shape]
        dst.copy_(src)
        torch.cuda.synchronize()

    for case in cases:
        for _ in range(args.warmup):
            composite(case)
    for shape in shapes:
        for _ in range(max(args.warmup, 1)):
            copy(shape)
    windows = {case[0]: [] for case in cases}
    copy_windows = {shape: [] for shape in shapes}
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case in cases:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                composite(case)
            windows[case[0]].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for shape in shapes:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                copy(shape)
            copy_windows[shape].append((time.perf_counter() - t0) * 1e3 / args.steps)
    for name, w, h, mode, op, offset in cases:
        v = sorted(windows[name])
        print(json.dumps({"case": name, "size": [w, h], "mode": mode, "op": op, "offset": list(offset), "ms_per_call": round(v[len(v) // 2], 4), "spread": round(v[-1] - v[0], 4),
                          "copy_ms": round(sorted(copy_windows[(w, h)])[len(v) // 2], 4), "windows": [round(x, 4) for x in windows[name]]}))


if __name__ == "__main__":
    main()
