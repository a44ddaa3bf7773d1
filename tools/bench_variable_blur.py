#!/usr/bin/env python3
"""GPU: Image.variable_blur (crh_image_variable_blur: the 256 tap sets of each axis built on the host, their upload, the allocation,
k_image_variable_blur_h + k_image_variable_blur_v and the wait — the call is synchronous) against Image.blur at the same sigma in the
same session, on random premultiplied images of 1024^2 and 4096^2, BlurEdge.Pad, sigma 8 and 64 on both axes (sigma 0 at mask code 0).
Per size and sigma:
  blur      Image.blur(sigma): the yardstick, the existing call
  uniform   a mask of code 255 everywhere: the same work as blur, every wave on the wave-uniform path — the price of generality
  one_set   the same mask with sigma at code 0 = sigma at code 255: one tap set instead of 256, so uniform - one_set is what building
            and uploading the tap sets (about 200 KB at sigma 64) costs
  ramp      the mask's alpha ramps from 0 at the top to 255 at the bottom: the progressive blur, roughly half the work
  noise     random mask bytes: every lane its own level, no uniform wave — the worst divergence
The cases are interleaved window by window. Beside each: a device-to-device copy of the same image (torch), the memory floor, timed the
same way.
Prints one JSON line per case: {"case", "size", "sigma", "kind", "ms_per_call" (median of --repeats windows of --steps calls), "spread"
(max - min of the windows), "copy_ms", "ratio_to_blur", "windows"}.
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same
--only, --warmup, --steps and --repeats, and prints the median time of each kernel per case instead (nothing runs).
Usage: tools/bench_variable_blur.py [--steps 10] [--warmup 2] [--repeats 5] [--only 4096_s64_noise,...] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SIZES = (1024, 4096)
SIGMAS = (8.0, 64.0)
KINDS = ("blur", "uniform", "one_set", "ramp", "noise")


def cases_of(only):
    cases = [(f"{size}_s{int(sigma)}_{kind}", size, sigma, kind) for size in SIZES for sigma in SIGMAS for kind in KINDS]
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def random_image(size, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(64, 256, (size, size, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def mask_of(kind, size):
    mask = np.zeros((size, size, 4), dtype=np.uint8)
    if kind == "ramp":
        mask[..., 3] = (np.arange(size) * 255 // (size - 1)).astype(np.uint8)[:, None]
    elif kind == "noise":
        mask[..., 3] = np.random.RandomState(11).randint(0, 256, (size, size)).astype(np.uint8)
    else:
        mask[..., 3] = 255
    return mask


def kernels_of(kind):
    return ("k_image_blur_h", "k_image_blur_v") if kind == "blur" else ("k_image_variable_blur_h", "k_image_variable_blur_v")


def from_trace(path, cases, calls):
    """The dispatches of each kernel in start order: `calls` of each per case that runs it, in the order the tool ran the cases (warm-up
    first, case by case; then the windows, interleaved)."""
    names = ("k_image_blur_h", "k_image_blur_v", "k_image_variable_blur_h", "k_image_variable_blur_v")
    rows = {kernel: [] for kernel in names}
    with open(path) as f:
        for row in csv.DictReader(f):
            for kernel in names:
                if kernel in row["Kernel_Name"]:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    warmup, steps, repeats = calls
    for kernel, found in rows.items():
        found.sort()
        mine = [c for c in cases if kernel in kernels_of(c[3])]
        assert len(found) == len(mine) * (warmup + steps * repeats), (kernel, len(found))
    for name, _, _, kind in cases:
        line = {"case": name}
        for kernel in kernels_of(kind):
            mine = [c[0] for c in cases if kernel in kernels_of(c[3])]
            k, timed = mine.index(name), []
            for w in range(repeats):
                at = len(mine) * warmup + (w * len(mine) + k) * steps
                timed += [d for _, d in rows[kernel][at:at + steps]]
            line[kernel + "_us"] = round(float(np.median(timed)) / 1e3, 1)
        print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. 4096_s64_noise")
    ap.add_argument("--from-trace", default=None, help="a rocprofv3 kernel trace (csv) of a run with the same arguments: summarise it")
    args = ap.parse_args()
    cases = cases_of(args.only)
    if args.from_trace:
        from_trace(args.from_trace, cases, (args.warmup, args.steps, args.repeats))
        return
    import torch
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    sizes = [size for size in SIZES if any(c[1] == size for c in cases)]
    images = {size: R.Image(r, random_image(size, 7)) for size in sizes}
    masks = {}
    for _, size, _, kind in cases:
        key = ("uniform" if kind == "one_set" else kind, size)
        if kind != "blur" and key not in masks:
            masks[key] = R.Image(r, mask_of(key[0], size))
    copies = {size: (torch.randint(0, 255, (size * size * 4,), dtype=torch.uint8, device="cuda"), torch.empty(size * size * 4, dtype=torch.uint8, device="cuda")) for size in sizes}

    def call(case):
        _, size, sigma, kind = case
        if kind == "blur":
            out = images[size].blur(sigma, sigma, R.BlurEdge.Pad)
        elif kind == "one_set":
            out = images[size].variable_blur(masks["uniform", size], sigma, sigma)
        else:
            out = images[size].variable_blur(masks[kind, size], sigma)
        out.destroy()

    def copy(size):
        src, dst = copies[size]
        dst.copy_(src)
        torch.cuda.synchronize()

    for case in cases:
        for _ in range(args.warmup):
            call(case)
    for size in sizes:
        for _ in range(max(args.warmup, 1)):
            copy(size)
    windows = {case[0]: [] for case in cases}
    copy_windows = {size: [] for size in sizes}
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case in cases:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call(case)
            windows[case[0]].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for size in sizes:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                copy(size)
            copy_windows[size].append((time.perf_counter() - t0) * 1e3 / args.steps)
    median = {name: sorted(w)[len(w) // 2] for name, w in windows.items()}
    for name, size, sigma, kind in cases:
        w = sorted(windows[name])
        yardstick = median.get(f"{size}_s{int(sigma)}_blur")
        print(json.dumps({"case": name, "size": size, "sigma": sigma, "kind": kind, "ms_per_call": round(median[name], 4), "spread": round(w[-1] - w[0], 4),
                          "copy_ms": round(sorted(copy_windows[size])[len(w) // 2], 4), "ratio_to_blur": round(median[name] / yardstick, 3) if yardstick else None,
                          "windows": [round(v, 4) for v in windows[name]]}))


if __name__ == "__main__":
    main()
