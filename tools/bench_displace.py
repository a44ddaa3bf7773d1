#!/usr/bin/env python3
"""GPU: Image.displace (crh_image_displace: k_image_displace, the allocation and the wait included — the call is synchronous) at 4096^2 for
both filters, TRANSPARENT and REPEAT, and three maps: `constant` (every texel the same code, scale 32: a pure translation, the coalesced
best case), `turbulence` (2 octaves of fractal noise at base frequency 0.01, scale 32, channels R and G: the realistic case) and `noise`
(white noise per texel, scale 1024: every fetch up to 512 texels away in its own row, the worst case). The source is a random image. The
cases are interleaved window by window. Beside them, timed the same way in the same run: Image.color_filter with a matrix and no tables
(k_image_color_filter: a stream of 8 bytes per texel; displace moves at least 12), Image.turbulence of the realistic map
(k_image_turbulence, the anchor) and a device-to-device copy of an image of the size (torch, the floor).
Prints one JSON line per case: {"case", "size", "filter", "edge", "map", "ms_per_call" (median of --repeats windows of --steps calls),
"best_ms", "spread" (max - min of the windows), "color_filter_ms", "turbulence_ms", "copy_ms", "ratio_to_color_filter", "gtexel_per_s",
"windows"}.
--library FILE loads another build of the library (one compiled with -DCRH_DISPLACE_ROWS=... or -DCRH_DISPLACE_EDGE_TEMPLATE=1: how the
variants of DESIGN.md were measured).
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same --only,
--warmup, --steps and --repeats, and prints the median time of k_image_displace per case and of the two reference kernels instead
(nothing runs).
Usage: tools/bench_displace.py [--size 4096] [--steps 5] [--warmup 2] [--repeats 5] [--only linear_transparent_turbulence,...] [--library FILE] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FILTERS = ("nearest", "linear")
EDGES = ("transparent", "repeat")
MAPS = ("constant", "turbulence", "noise")
SCALES = {"constant": 32.0, "turbulence": 32.0, "noise": 1024.0}


def cases_of(only):
    cases = [(f"{filter}_{edge}_{map}", filter, edge, map) for filter in FILTERS for edge in EDGES for map in MAPS]
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def random_image(size, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (size, size, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def from_trace(path, cases, calls):
    """The dispatches of k_image_displace in start order: `calls` per case, in the order the tool ran the cases (warm-up first, case by
    case; then the windows, interleaved); the two reference kernels beside them (the first k_image_turbulence made the map: left out)."""
    rows = {"k_image_displace": [], "k_image_color_filter": [], "k_image_turbulence": []}
    with open(path) as f:
        for row in csv.DictReader(f):
            for kernel in rows:
                if kernel in row["Kernel_Name"]:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    warmup, steps, repeats = calls
    for found in rows.values():
        found.sort()
    assert len(rows["k_image_displace"]) == len(cases) * (warmup + steps * repeats), len(rows["k_image_displace"])
    reference = {kernel: round(float(np.median([d for _, d in rows[kernel][1 + warmup:]])) / 1e3, 1) if len(rows[kernel]) > 1 + warmup else None for kernel in ("k_image_color_filter", "k_image_turbulence")}
    for k, case in enumerate(cases):
        timed = []
        for w in range(repeats):
            at = len(cases) * warmup + (w * len(cases) + k) * steps
            timed += [d for _, d in rows["k_image_displace"][at:at + steps]]
        us = round(float(np.median(timed)) / 1e3, 1)
        print(json.dumps({"case": case[0], "k_image_displace_us": us, "k_image_color_filter_us": reference["k_image_color_filter"], "k_image_turbulence_us": reference["k_image_turbulence"],
                          "ratio_to_color_filter": round(us / reference["k_image_color_filter"], 2) if reference["k_image_color_filter"] else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. linear_transparent_turbulence,nearest_repeat_noise")
    ap.add_argument("--library", default=None, help="another build of libcontrast_hip.so to load")
    ap.add_argument("--from-trace", default=None, help="a rocprofv3 kernel trace (csv) of a run with the same arguments: summarise it")
    args = ap.parse_args()
    cases = cases_of(args.only)
    if args.from_trace:
        from_trace(args.from_trace, cases, (args.warmup, args.steps, args.repeats))
        return
    import torch
    from contrast_renderer_amd import _ffi
    if args.library:
        _ffi.LIB_PATH = os.path.abspath(args.library)
    from contrast_renderer_amd import BlurEdge, Channel, ColorMatrix, Filter, TurbulenceKind
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    size = args.size
    source = R.Image(r, random_image(size, 7))
    constant = np.empty((size, size, 4), dtype=np.uint8)
    constant[:] = (200, 90, 0, 255)  # scale 32: 32 * (200 / 255 - 1/2) = 9.1 texels right, 32 * (90 / 255 - 1/2) = 4.7 texels up

    def noise_map():
        return R.Image.turbulence(r, size, size, 0.01, 2, 11, TurbulenceKind.FractalNoise)

    maps = {"constant": R.Image(r, constant), "turbulence": noise_map(), "noise": R.Image(r, random_image(size, 8))}
    filters, edges = {"nearest": Filter.Nearest, "linear": Filter.Linear}, {"transparent": BlurEdge.Transparent, "repeat": BlurEdge.Repeat}
    matrix = ColorMatrix.saturate(0.4)
    src, dst = torch.randint(0, 255, (size * size * 4,), dtype=torch.uint8, device="cuda"), torch.empty(size * size * 4, dtype=torch.uint8, device="cuda")

    def displace(case):
        source.displace(maps[case[3]], SCALES[case[3]], Channel.R, Channel.G, filters[case[1]], edges[case[2]]).destroy()

    def color_filter(_):
        source.color_filter(matrix).destroy()

    def turbulence(_):
        noise_map().destroy()

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
            displace(case)
    for _ in range(max(args.warmup, 1)):
        color_filter(None)
        turbulence(None)
        copy(None)
    windows = {case[0]: [] for case in cases}
    filter_windows, turbulence_windows, copy_windows = [], [], []
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case in cases:
            window(displace, case, windows[case[0]])
        window(color_filter, None, filter_windows)
        window(turbulence, None, turbulence_windows)
        window(copy, None, copy_windows)
    middle = lambda values: sorted(values)[len(values) // 2]  # noqa: E731
    filter_ms, turbulence_ms, copy_ms = middle(filter_windows), middle(turbulence_windows), middle(copy_windows)
    for name, filter, edge, map in cases:
        w = sorted(windows[name])
        ms = middle(w)
        print(json.dumps({"case": name, "size": size, "filter": filter, "edge": edge, "map": map, "ms_per_call": round(ms, 4), "best_ms": round(w[0], 4), "spread": round(w[-1] - w[0], 4),
                          "color_filter_ms": round(filter_ms, 4), "turbulence_ms": round(turbulence_ms, 4), "copy_ms": round(copy_ms, 4), "ratio_to_color_filter": round(ms / filter_ms, 2),
                          "gtexel_per_s": round(size * size / (ms * 1e-3) / 1e9, 2), "windows": [round(v, 4) for v in windows[name]]}))


if __name__ == "__main__":
    main()
