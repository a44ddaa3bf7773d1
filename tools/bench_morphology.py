#!/usr/bin/env python3
"""GPU: Image.morphology (crh_image_morphology: k_image_morph_h + k_image_morph_v, the allocations and the wait included — the call is synchronous)
on random premultiplied images of 1024^2 and 4096^2, radius 2, 8, 32, 64 and 192 on both axes: Dilate under BlurEdge.Pad and under
BlurEdge.Transparent, and Erode under BlurEdge.Pad. The cases are interleaved window by window. Beside each case, timed the same way in the same
run: a device-to-device copy of the same image (torch, the floor), and Image.blur at the same radius (sigma = radius / 3, ceil(3 sigma) = radius) and edge — blur's
windowed kernels cost in proportion to the radius, so it is the yardstick.
Prints one JSON line per case: {"case", "size", "radius", "op", "edge", "out_size", "ms_per_call" (median of --repeats windows of --steps calls),
"spread" (max - min of the windows), "copy_ms", "blur_ms", "blur_spread", "gtexels_per_s" (texels of the result per second of the whole call)}.
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same --only,
--warmup, --steps and --repeats, and prints the median time of each kernel per case instead (nothing runs).
Usage: tools/bench_morphology.py [--steps 10] [--warmup 2] [--repeats 5] [--only 4096_r192_dilate_pad,...] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SIZES = (1024, 4096)
RADII = (2, 8, 32, 64, 192)
KINDS = (("dilate_pad", 1, 1), ("dilate_transparent", 1, 0), ("erode_pad", 0, 1))  # (name, op, edge)


def cases_of(only):
    cases = [(f"{size}_r{radius}_{name}", size, radius, op, edge) for size in SIZES for radius in RADII for name, op, edge in KINDS]
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def random_image(size, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(64, 256, (size, size, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def sigma_of(radius):
    """The largest f32 sigma whose blur radius ceil(3 sigma) is `radius` (radius / 3 rounded to f32 may lie above it)."""
    sigma = np.float32(radius / 3.0)
    if int(np.ceil(3.0 * float(sigma))) > radius:
        sigma = np.nextafter(sigma, np.float32(0))
    assert int(np.ceil(3.0 * float(sigma))) == radius, (radius, sigma)
    return float(sigma)


def blurs_of(cases):
    return sorted({(size, radius, edge) for _, size, radius, _, edge in cases})


def from_trace(path, cases, calls):
    """The dispatches of the two morphology kernels in start order: `calls` of each per case, in the order the tool ran the cases (warm-up
    first, case by case; then the windows, interleaved). Every case here has both radii above zero, so every call runs both kernels. Where the
    run timed Image.blur as well (no --no-blur), its two kernels' medians at the case's size, radius and edge stand beside them."""
    rows = {"k_image_morph_h": [], "k_image_morph_v": [], "k_image_blur_h": [], "k_image_blur_v": []}
    with open(path) as f:
        for row in csv.DictReader(f):
            for kernel in rows:
                if kernel in row["Kernel_Name"]:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    warmup, steps, repeats = calls
    blurs = blurs_of(cases) if rows["k_image_blur_h"] else []
    for kernel, found in rows.items():
        found.sort()
        runs = blurs if "blur" in kernel else cases
        assert len(found) == len(runs) * (warmup + steps * repeats), (kernel, len(found))

    def median_us(kernel, runs, k):
        timed = []
        for w in range(repeats):
            at = len(runs) * warmup + (w * len(runs) + k) * steps
            timed += [d for _, d in rows[kernel][at:at + steps]]
        return round(float(np.median(timed)) / 1e3, 1)

    for k, (name, size, radius, op, edge) in enumerate(cases):
        line = {"case": name}
        for kernel in ("k_image_morph_h", "k_image_morph_v"):
            line[kernel + "_us"] = median_us(kernel, cases, k)
        if blurs:
            for kernel in ("k_image_blur_h", "k_image_blur_v"):
                line[kernel + "_us"] = median_us(kernel, blurs, blurs.index((size, radius, edge)))
        print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. 4096_r192_dilate_pad")
    ap.add_argument("--from-trace", default=None, help="a rocprofv3 kernel trace (csv) of a run with the same arguments: summarise it")
    ap.add_argument("--no-blur", action="store_true", help="do not time Image.blur beside the cases (a run under the profiler: only the morphology kernels are wanted)")
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
    blurs = [] if args.no_blur else blurs_of(cases)

    def morphology(case):
        _, size, radius, op, edge = case
        out = images[size].morphology(op, radius, radius, edge)
        shape = (out.width, out.height)
        out.destroy()
        return shape

    def blur(which):
        size, radius, edge = which
        images[size].blur(sigma_of(radius), sigma_of(radius), edge).destroy()  # ceil(3 sigma) = radius

    def copy(size):
        src, dst = copies[size]
        dst.copy_(src)
        torch.cuda.synchronize()

    def window(call, what, into):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call(what)
        into.append((time.perf_counter() - t0) * 1e3 / args.steps)

    shapes = {}
    for case in cases:
        for _ in range(args.warmup):
            shapes[case[0]] = morphology(case)
    for which in blurs:
        for _ in range(args.warmup):
            blur(which)
    for size in images:
        for _ in range(max(args.warmup, 1)):
            copy(size)
    windows = {case[0]: [] for case in cases}
    blur_windows = {which: [] for which in blurs}
    copy_windows = {size: [] for size in images}
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case in cases:
            window(morphology, case, windows[case[0]])
        for which in blurs:
            window(blur, which, blur_windows[which])
        for size in images:
            window(copy, size, copy_windows[size])
    middle = lambda values: sorted(values)[len(values) // 2]  # noqa: E731
    for name, size, radius, op, edge in cases:
        w = sorted(windows[name])
        ms = middle(w)
        out = shapes.get(name, (size, size))
        line = {"case": name, "size": size, "radius": radius, "op": "dilate" if op else "erode", "edge": "transparent" if edge == 0 else "pad", "out_size": list(out),
                "ms_per_call": round(ms, 4), "spread": round(w[-1] - w[0], 4), "copy_ms": round(middle(copy_windows[size]), 4)}
        if not args.no_blur:
            b = sorted(blur_windows[(size, radius, edge)])
            line["blur_ms"], line["blur_spread"] = round(middle(b), 4), round(b[-1] - b[0], 4)
        line["gtexels_per_s"] = round(out[0] * out[1] / (ms * 1e-3) / 1e9, 2)
        line["windows"] = [round(v, 4) for v in windows[name]]
        print(json.dumps(line))


if __name__ == "__main__":
    main()
