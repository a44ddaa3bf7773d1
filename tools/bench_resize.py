#!/usr/bin/env python3
"""GPU: Image.resize (crh_image_resize: k_image_resize_h + k_image_resize_v, the table upload, the allocations and the wait included — the
call is synchronous) of a 4096^2 source, `glyphs` (a rendered layer of text) or `turbulence` (crh_image_turbulence noise), under each
filter at x0.5, x0.37, x0.1 and x2 on both axes. The cases are interleaved window by window. Beside them, timed the same way in the
same run, the yardsticks: Image.color_filter with a matrix and no tables over the source (k_image_color_filter: the floor for reading it
once), Image.blur under BlurEdge.Pad at the radius whose 2 R + 1 taps are the case's taps per output texel (k_image_blur_h +
k_image_blur_v, at the source's size) and, for box x0.5, the first level of Image.generate_mipmaps (k_image_downsample).
Prints one JSON line per case: {"case", "size", "source", "filter", "scale", "out", "taps" (the largest window of an axis), "ms_per_call"
(median of --repeats windows of --steps calls), "best_ms", "window_range_ms", "color_filter_ms", "blur_radius", "blur_ms",
"ratio_to_color_filter", "windows"}.
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same
arguments and prints the median time of the two resize kernels per case and of the yardsticks' kernels instead (nothing runs): the
kernels alone.
Usage: tools/bench_resize.py [--size 4096] [--source glyphs] [--steps 3] [--warmup 1] [--repeats 5] [--only lanczos3_x0.5,...] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FILTERS = ("box", "triangle", "catmull_rom", "mitchell", "lanczos3")
SUPPORT = {"box": 0.5, "triangle": 1.0, "catmull_rom": 2.0, "mitchell": 2.0, "lanczos3": 3.0}
SCALES = (0.5, 0.37, 0.1, 2.0)
MAX_RADIUS = 192  # CRH_MAX_BLUR_RADIUS


def taps_of(name, size, out):
    """the window of an output in the middle of the axis: floor(c + r s) - floor(c - r s) + 1"""
    s = max(1.0, size / out)
    c = ((out // 2 + 0.5) * size) / out
    return int(math.floor(c + SUPPORT[name] * s)) - int(math.floor(c - SUPPORT[name] * s)) + 1


def cases_of(only, size):
    cases = []
    for filter, name in enumerate(FILTERS):
        for scale in SCALES:
            out = max(1, int(round(size * scale)))
            taps = taps_of(name, size, out)
            cases.append((f"{name}_x{scale:g}", filter, scale, out, taps, min(MAX_RADIUS, max(1, (taps - 1) // 2))))
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def radii_of(cases):
    return sorted({c[5] for c in cases})


def levels_of(size):
    return int(math.floor(math.log2(size))) + 1


def from_trace(path, cases, calls, size):
    """The dispatches of each kernel in start order: per group (the resize cases, the colour filter, the blur radii, the mip chain)
    `warmup` calls per member first, member by member, then the windows, interleaved."""
    rows = {"k_image_resize_h": [], "k_image_resize_v": [], "k_image_color_filter": [], "k_image_blur_h": [], "k_image_blur_v": [], "k_image_downsample": []}
    with open(path) as f:
        for row in csv.DictReader(f):
            for kernel in rows:
                if kernel in row["Kernel_Name"]:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    warmup, steps, repeats = calls
    radii = radii_of(cases)
    mips = any(c[0] == "box_x0.5" for c in cases)
    per_chain = levels_of(size) - 1  # dispatches of k_image_downsample per call: the first is level 1
    for kernel, found in rows.items():
        found.sort()
        runs = len(cases) if "resize" in kernel else len(radii) if "blur" in kernel else 1
        expect = runs * (warmup + steps * repeats) * (per_chain if "downsample" in kernel else 1)
        assert len(found) == (expect if mips or "downsample" not in kernel else 0), (kernel, len(found), expect)

    def median_us(kernel, runs, k, stride=1):
        timed = []
        for w in range(repeats):
            at = runs * warmup + (w * runs + k) * steps
            timed += [d for _, d in rows[kernel][at * stride:(at + steps) * stride:stride]]
        return round(float(np.median(timed)) / 1e3, 1)

    stream = median_us("k_image_color_filter", 1, 0)
    for k, (name, filter, scale, out, taps, radius) in enumerate(cases):
        h, v = median_us("k_image_resize_h", len(cases), k), median_us("k_image_resize_v", len(cases), k)
        at = radii.index(radius)
        blur_h, blur_v = median_us("k_image_blur_h", len(radii), at), median_us("k_image_blur_v", len(radii), at)
        line = {"case": name, "out": out, "taps": taps, "k_image_resize_h_us": h, "k_image_resize_v_us": v, "resize_us": round(h + v, 1), "k_image_color_filter_us": stream,
                "blur_radius": radius, "k_image_blur_h_us": blur_h, "k_image_blur_v_us": blur_v, "ratio_to_color_filter": round((h + v) / stream, 2),
                # per output texel of each horizontal kernel: out x size for the resize, size x size for the blur
                "h_per_texel_to_blur_h": round((h / (out * size)) / (blur_h / (size * size)), 2)}
        if name == "box_x0.5":
            line["k_image_downsample_level1_us"] = median_us("k_image_downsample", 1, 0, per_chain)
        print(json.dumps(line))


def glyph_layer(R, size, n_glyphs):
    """A frame of text drawn by the library -> its bytes"""
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
    return frame.download()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--source", default="glyphs", choices=("glyphs", "turbulence"))
    ap.add_argument("--glyphs", type=int, default=12000, help="glyph instances on the layer")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. lanczos3_x0.5,box_x0.1")
    ap.add_argument("--from-trace", default=None, help="a rocprofv3 kernel trace (csv) of a run with the same arguments: summarise it")
    args = ap.parse_args()
    size = args.size
    cases = cases_of(args.only, size)
    if args.from_trace:
        from_trace(args.from_trace, cases, (args.warmup, args.steps, args.repeats), size)
        return
    from contrast_renderer_amd import BlurEdge, ColorMatrix, ResizeFilter
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    if args.source == "glyphs":
        bytes_ = glyph_layer(R, size, args.glyphs)
        source = R.Image(r, bytes_)
    else:
        source = R.Image.turbulence(r, size, size, base_frequency=0.02, octaves=4)
        bytes_ = source.download_level(0)
    matrix = ColorMatrix.saturate(0.4)
    radii = radii_of(cases)
    mips = any(c[0] == "box_x0.5" for c in cases)

    def resize(case):
        source.resize(case[3], case[3], ResizeFilter(case[1])).destroy()

    def color_filter(_):
        source.color_filter(matrix).destroy()

    def blur(radius):
        source.blur(radius / 3.0, edge=BlurEdge.Pad).destroy()

    def mipmaps(_):
        fresh = R.Image(r, bytes_)  # (a chain is made once per image: the upload is outside the window's clock only in the trace)
        fresh.generate_mipmaps()
        fresh.destroy()

    def window(call, what, into):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call(what)
        into.append((time.perf_counter() - t0) * 1e3 / args.steps)

    groups = [(resize, cases), (color_filter, [None]), (blur, radii)] + ([(mipmaps, [None])] if mips else [])
    for call, members in groups:
        for member in members:
            for _ in range(args.warmup):
                call(member)
    windows = {id(call): [[] for _ in members] for call, members in groups}
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for call, members in groups:
            for k, member in enumerate(members):
                window(call, member, windows[id(call)][k])
    middle = lambda values: sorted(values)[len(values) // 2]  # noqa: E731
    filter_ms = middle(windows[id(color_filter)][0])
    for k, (name, filter, scale, out, taps, radius) in enumerate(cases):
        w = sorted(windows[id(resize)][k])
        ms, blur_ms = middle(w), middle(windows[id(blur)][radii.index(radius)])
        print(json.dumps({"case": name, "size": size, "source": args.source, "filter": FILTERS[filter], "scale": scale, "out": out, "taps": taps, "ms_per_call": round(ms, 4), "best_ms": round(w[0], 4),
                          "window_range_ms": round(w[-1] - w[0], 4), "color_filter_ms": round(filter_ms, 4), "blur_radius": radius, "blur_ms": round(blur_ms, 4),
                          "ratio_to_color_filter": round(ms / filter_ms, 2), "windows": [round(v, 4) for v in windows[id(resize)][k]]}))


if __name__ == "__main__":
    main()
