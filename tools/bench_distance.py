#!/usr/bin/env python3
"""GPU: Image.distance_field (crh_image_distance_field: k_image_distance_v + k_image_distance_h, the allocations and the wait included — the
call is synchronous) at 4096^2, OUTSIDE under BlurEdge.Pad (the result keeps the size), spreads 4, 32 and 255, on three sources: `glyphs` (a
rendered layer of text, alpha >= 128 the shape: the realistic case), `empty` (nothing inside: "none" through both passes) and `full`
(everything inside: every scan ends at once). The cases are interleaved window by window. Beside them, timed the same way in the same run,
the two yardsticks: Image.color_filter with a matrix and no tables (k_image_color_filter: a stream of 8 bytes per texel) and Image.dilate
at the equal radius, capped at 192 (k_image_morph_h + k_image_morph_v), on the glyph layer under the same edge.
Prints one JSON line per case: {"case", "size", "source", "spread", "ms_per_call" (median of --repeats windows of --steps calls),
"best_ms", "window_range_ms" (max - min of the windows: a stray slow window shows here and not in the median), "color_filter_ms", "dilate_ms", "ratio_to_color_filter", "ratio_to_dilate", "windows"}.
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same --only,
--warmup, --steps and --repeats, and prints the median time of the two distance kernels per case and of the yardsticks' kernels instead
(nothing runs): the kernels alone.
Usage: tools/bench_distance.py [--size 4096] [--glyphs 12000] [--steps 5] [--warmup 2] [--repeats 5] [--only glyphs_s32,...] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SOURCES = ("glyphs", "empty", "full")
SPREADS = (4, 32, 255)
MAX_RADIUS = 192  # CRH_MAX_MORPHOLOGY_RADIUS


def cases_of(only):
    cases = [(f"{source}_s{spread}", source, spread) for source in SOURCES for spread in SPREADS]
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def radii_of(cases):
    return sorted({min(spread, MAX_RADIUS) for _, _, spread in cases})


def from_trace(path, cases, calls):
    """The dispatches of the two distance kernels in start order: `calls` of each per case, in the order the tool ran the cases (warm-up
    first, case by case; then the windows, interleaved); the yardsticks' kernels beside them, dilate's per radius in the same order."""
    rows = {"k_image_distance_v": [], "k_image_distance_h": [], "k_image_color_filter": [], "k_image_morph_h": [], "k_image_morph_v": []}
    with open(path) as f:
        for row in csv.DictReader(f):
            for kernel in rows:
                if kernel in row["Kernel_Name"]:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    warmup, steps, repeats = calls
    radii = radii_of(cases)
    for kernel, found in rows.items():
        found.sort()
        runs, warm = (len(cases), warmup) if "distance" in kernel else (len(radii) if "morph" in kernel else 1, max(warmup, 1))
        assert len(found) == runs * (warm + steps * repeats), (kernel, len(found))

    def median_us(kernel, runs, k, warm):
        timed = []
        for w in range(repeats):
            at = runs * warm + (w * runs + k) * steps
            timed += [d for _, d in rows[kernel][at:at + steps]]
        return round(float(np.median(timed)) / 1e3, 1)

    stream = median_us("k_image_color_filter", 1, 0, max(warmup, 1))
    for k, (name, source, spread) in enumerate(cases):
        v, h = median_us("k_image_distance_v", len(cases), k, warmup), median_us("k_image_distance_h", len(cases), k, warmup)
        at = radii.index(min(spread, MAX_RADIUS))
        dilate = round(median_us("k_image_morph_h", len(radii), at, max(warmup, 1)) + median_us("k_image_morph_v", len(radii), at, max(warmup, 1)), 1)
        print(json.dumps({"case": name, "k_image_distance_v_us": v, "k_image_distance_h_us": h, "distance_us": round(v + h, 1), "k_image_color_filter_us": stream,
                          "dilate_radius": min(spread, MAX_RADIUS), "dilate_us": dilate, "ratio_to_color_filter": round((v + h) / stream, 2), "ratio_to_dilate": round((v + h) / dilate, 2)}))


def glyph_layer(r, R, size, n_glyphs):
    """A frame of text drawn by the library -> its bytes on the device as an Image"""
    from contrast_renderer_amd import scenes
    sc = scenes.scene_glyphs(n_glyphs, (size, size))
    renderer = R.Renderer(R.Configuration(msaa_sample_count=sc["msaa"], clip_nesting_counter_bits=4, winding_counter_bits=4), device=0)
    scene = R.Scene(renderer, sc["batch"], tessellate=True)
    scene.check()
    scene.set_instances(sc["transforms"], sc["colors"])
    frame = R.Frame(renderer, size, size)
    scene.tessellate()
    frame.clear()
    scene.render(frame)
    return R.Image(r, frame.download())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--glyphs", type=int, default=12000, help="glyph instances on the layer")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. glyphs_s32,empty_s255")
    ap.add_argument("--from-trace", default=None, help="a rocprofv3 kernel trace (csv) of a run with the same arguments: summarise it")
    args = ap.parse_args()
    cases = cases_of(args.only)
    if args.from_trace:
        from_trace(args.from_trace, cases, (args.warmup, args.steps, args.repeats))
        return
    from contrast_renderer_amd import BlurEdge, ColorMatrix, DistanceMode
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    size = args.size
    glyphs = glyph_layer(r, R, size, args.glyphs)
    covered = float((glyphs.download_level(0)[..., 3] >= 128).mean())
    sources = {"glyphs": glyphs, "empty": R.Image(r, np.zeros((size, size, 4), dtype=np.uint8)), "full": R.Image(r, np.full((size, size, 4), 255, dtype=np.uint8))}
    matrix = ColorMatrix.saturate(0.4)
    radii = radii_of(cases)

    def distance(case):
        sources[case[1]].distance_field(case[2], DistanceMode.Outside, edge=BlurEdge.Pad).destroy()

    def color_filter(_):
        glyphs.color_filter(matrix).destroy()

    def dilate(radius):
        glyphs.dilate(radius, radius, BlurEdge.Pad).destroy()

    def window(call, what, into):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call(what)
        into.append((time.perf_counter() - t0) * 1e3 / args.steps)

    for case in cases:
        for _ in range(args.warmup):
            distance(case)
    for _ in range(max(args.warmup, 1)):
        color_filter(None)
    for radius in radii:
        for _ in range(max(args.warmup, 1)):
            dilate(radius)
    windows = {case[0]: [] for case in cases}
    filter_windows, dilate_windows = [], {radius: [] for radius in radii}
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case in cases:
            window(distance, case, windows[case[0]])
        window(color_filter, None, filter_windows)
        for radius in radii:
            window(dilate, radius, dilate_windows[radius])
    middle = lambda values: sorted(values)[len(values) // 2]  # noqa: E731
    filter_ms = middle(filter_windows)
    for name, source, spread in cases:
        w = sorted(windows[name])
        ms, dilate_ms = middle(w), middle(dilate_windows[min(spread, MAX_RADIUS)])
        print(json.dumps({"case": name, "size": size, "source": source, "spread": spread, **({"glyph_coverage": round(covered, 4)} if source == "glyphs" else {}), "ms_per_call": round(ms, 4), "best_ms": round(w[0], 4),
                          "window_range_ms": round(w[-1] - w[0], 4), "color_filter_ms": round(filter_ms, 4), "dilate_radius": min(spread, MAX_RADIUS), "dilate_ms": round(dilate_ms, 4),
                          "ratio_to_color_filter": round(ms / filter_ms, 2), "ratio_to_dilate": round(ms / dilate_ms, 2), "windows": [round(v, 4) for v in windows[name]]}))


if __name__ == "__main__":
    main()
