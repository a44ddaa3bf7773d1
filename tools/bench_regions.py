#!/usr/bin/env python3
"""GPU: Image.statistics, Image.crop and the trimmed shadow chain (crh_image_statistics, crh_image_crop; the calls are synchronous, so a
call's time holds its allocation and its wait) on 4096^2 images.
  stats_noise, stats_zero, stats_constant   Image.statistics of turbulence noise, of an all-transparent image and of an opaque constant one
  filter_noise, filter_zero, filter_constant  Image.color_filter (a matrix) of the same images: the yardstick, 8 bytes per texel moved where
                                            the statistics read 4
  crop_wide, crop_narrow                    Image.crop of the noise to 4096^2 at x = 0 (16-byte source loads) and x = 1 (4-byte loads)
  copy                                      a device-to-device copy of 4096^2 texels (torch), what crh_image_create_from_frame does
The cases are interleaved window by window. Prints one JSON line per case: {"case", "ms_per_call" (median of --repeats windows of --steps
calls), "spread" (max - min of the windows), "windows"}, then the chain the README shows on a 4096^2 snapshot with 300 x 200 texels of
content — blur(8), flood, composite under the layer — on the full image and behind trim() (statistics and crop included), wall time:
{"case": "chain_full" | "chain_trimmed", ...}.
CRH_STATS_VARIANT=0 (a plain LDS histogram) or 1 (+ zero texels counted in a register) in the environment runs k_image_stats' other arms.
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same
--warmup, --steps, --repeats and --no-chain, and prints per case the median time of the kernel alone with the spread of its window
medians, the ratios the design records, and the bytes per second (nothing runs).
Usage: tools/bench_regions.py [--steps 10] [--warmup 2] [--repeats 5] [--no-chain] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SIZE = 4096
INPUTS = ("noise", "zero", "constant")
# (case, the kernel whose dispatch is the case's), in the order of a window; the copy is torch's, the runtime's __amd_rocclr_copyBuffer
CASES = [(f"stats_{i}", "k_image_stats") for i in INPUTS] + [(f"filter_{i}", "k_image_color_filter") for i in INPUTS] + [("crop_wide", "k_image_crop"), ("crop_narrow", "k_image_crop"), ("copy", "copyBuffer")]


def kernel_of(name):
    """the key of CASES a dispatch belongs to (k_image_stats_merge is its own)"""
    for key in ("k_image_stats_merge", "k_image_stats", "k_image_color_filter", "k_image_crop", "copyBuffer"):
        if key in name:
            return key
    return None


def from_trace(path, warmup, steps, repeats):
    """The dispatches of a kernel in start order are its cases' in CASES' order: `warmup` per case, case by case, then the windows, `steps`
    per case. The copies of window w are the copyBuffer dispatches between the window's last k_image_crop and the next window's first
    k_image_stats (the statistics' 4116 bytes to the host and the uploads are copies, too): another count gives no figure, not a wrong one."""
    found = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            key = kernel_of(row["Kernel_Name"])
            if key:
                found.setdefault(key, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    for key in found:
        found[key].sort()
    windows = {}
    for kernel in ("k_image_stats", "k_image_stats_merge", "k_image_color_filter", "k_image_crop"):
        names = [c for c, k in CASES if k == kernel.replace("_merge", "")]
        entries, n = found.get(kernel, []), len(names)
        assert len(entries) == n * (warmup + steps * repeats), (kernel, len(entries))
        for k, name in enumerate(names):
            label = name + ("_merge" if kernel.endswith("_merge") else "")
            windows[label] = [float(np.median([d for _, d in entries[n * warmup + (w * n + k) * steps:][:steps]])) / 1e3 for w in range(repeats)]
    crops, stats, copies = found["k_image_crop"], found["k_image_stats"], found.get("copyBuffer", [])
    copy_windows = []
    for w in range(repeats):
        last = crops[2 * (warmup + (w + 1) * steps) - 1][0]
        nxt = stats[3 * (warmup + (w + 1) * steps)][0] if w + 1 < repeats else float("inf")
        between = [d for t, d in copies if last < t < nxt]
        if len(between) == steps:
            copy_windows.append(float(np.median(between)) / 1e3)
    if len(copy_windows) == repeats:
        windows["copy"] = copy_windows
    median = {k: float(np.median(v)) for k, v in windows.items()}
    texels = SIZE * SIZE
    for name, v in windows.items():
        moved = 4.0 if name.startswith("stats") and not name.endswith("merge") else 8.0
        line = {"case": name, "kernel_us": round(median[name], 1), "spread_us": round(max(v) - min(v), 1), "windows_us": [round(x, 1) for x in v]}
        if not name.endswith("_merge"):
            line["gb_per_s"] = round(moved * texels / (median[name] * 1e-6) / 1e9, 1)
        if name.startswith("stats_") and not name.endswith("_merge"):
            line["ratio_to_color_filter"] = round(median[name] / median["filter_" + name[6:]], 2)
            line["ratio_to_noise"] = round(median[name] / median["stats_noise"], 2)
        if name.startswith("crop_") and "copy" in median:
            line["ratio_to_copy"] = round(median[name] / median["copy"], 2)
        print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-chain", action="store_true", help="leave the shadow chain out (a run under rocprofv3: its kernels would count)")
    ap.add_argument("--from-trace", default=None, help="a rocprofv3 kernel trace (csv) of a run with the same arguments: summarise it")
    args = ap.parse_args()
    if args.from_trace:
        from_trace(args.from_trace, args.warmup, args.steps, args.repeats)
        return
    import torch
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    noise = R.Image.turbulence(r, SIZE, SIZE, 0.02, octaves=3, seed=1)
    images = {"noise": noise, "zero": R.Image(r, np.zeros((SIZE, SIZE, 4), dtype=np.uint8)), "constant": R.Image(r, np.full((SIZE, SIZE, 4), (40, 80, 120, 255), dtype=np.uint8))}
    src, dst = torch.randint(0, 255, (SIZE * SIZE * 4,), dtype=torch.uint8, device="cuda"), torch.empty(SIZE * SIZE * 4, dtype=torch.uint8, device="cuda")
    matrix = R.ColorMatrix.hue_rotate(90)

    def run(case):
        kind, _, what = case.partition("_")
        if kind == "stats":
            images[what].statistics()
        elif kind == "filter":
            images[what].color_filter(matrix).destroy()
        elif kind == "crop":
            noise.crop(0 if what == "wide" else 1, 0, SIZE, SIZE).destroy()
        else:
            dst.copy_(src)
            torch.cuda.synchronize()

    for case, _ in CASES:
        for _ in range(args.warmup):
            run(case)
    windows = {case: [] for case, _ in CASES}
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case, _ in CASES:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run(case)
            windows[case].append((time.perf_counter() - t0) * 1e3 / args.steps)
    for case, _ in CASES:
        v = sorted(windows[case])
        print(json.dumps({"case": case, "ms_per_call": round(v[len(v) // 2], 4), "spread": round(v[-1] - v[0], 4), "windows": [round(x, 4) for x in windows[case]]}))
    if args.no_chain:
        return
    # the chain the README shows: a 4096^2 snapshot with 300 x 200 texels of content
    content = R.Image.turbulence(r, 300, 200, 0.05, octaves=2, seed=3, opaque=True)
    layer = content.crop(-1900, -2000, SIZE, SIZE)
    flood = R.ColorMatrix.flood(0, 0, 0, .5)

    def chain(trim):
        part = layer.trim() if trim else layer
        shadow = part.blur(8).color_filter(flood)
        # the shadow under the layer, 6 texels right and down: the offset of the shadow's texel (0, 0) on the layer
        out = layer.composite(shadow, R.CompositeOp.DstOver, offset=(6 - part.origin[0] + layer.origin[0] - shadow.origin[0], 6 - part.origin[1] + layer.origin[1] - shadow.origin[1]))
        return out

    full, trimmed = chain(False).download_level(0), chain(True).download_level(0)
    assert np.array_equal(full, trimmed) and full[..., 3].max() == 255 and (full[..., 3] == 0).mean() > 0.9
    chains = {False: [], True: []}
    for _ in range(args.repeats):
        for trim in (False, True):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                chain(trim).destroy()
            chains[trim].append((time.perf_counter() - t0) * 1e3 / args.steps)
    for trim in (False, True):
        v = sorted(chains[trim])
        print(json.dumps({"case": "chain_trimmed" if trim else "chain_full", "ms_per_call": round(v[len(v) // 2], 4), "spread": round(v[-1] - v[0], 4), "windows": [round(x, 4) for x in chains[trim]]}))


if __name__ == "__main__":
    main()
