#!/usr/bin/env python3
"""GPU: Image.lighting (crh_image_lighting: k_image_lighting, the allocation and the wait included — the call is synchronous) at 4096^2 under
BlurEdge.Pad for each (op, light) pair, on two height fields: `random` (every alpha random: no texel has a zero gradient) and `layer` (a
blurred disc, as a bump map is: flat nearly everywhere). The cases are interleaved window by window. Beside them, timed the same way in the
same run: Image.convolve with a dense 3 x 3 kernel (k_image_convolve, the stencil that moves the same bytes), Image.color_filter with a
matrix (k_image_color_filter: the streaming kernel) and a device-to-device copy of the same image (torch, the floor).
Prints one JSON line per case: {"case", "size", "op", "light", "field", "ms_per_call" (median of --repeats windows of --steps calls),
"best_ms" (the fastest window: a window now and then holds an allocation of several milliseconds), "spread" (max - min of the windows),
"convolve3_ms", "color_filter_ms", "copy_ms", "ratio_to_convolve3", "gtexel_per_s", "windows"}.
--library FILE loads another build of the library (one compiled with -DCRH_LIGHTING_ROWS=... or -DCRH_LIGHTING_FLAT_SKIP=0: how the
variants of DESIGN.md were measured).
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same --only,
--warmup, --steps and --repeats, and prints the median time of k_image_lighting per case and of k_image_convolve and k_image_color_filter
instead (nothing runs).
Usage: tools/bench_lighting.py [--size 4096] [--steps 10] [--warmup 2] [--repeats 5] [--only diffuse_distant_random,...] [--library FILE] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

OPS = ("diffuse", "specular")
LIGHTS = ("distant", "point", "spot")
FIELDS = ("random", "layer")


def cases_of(only):
    cases = [(f"{op}_{light}_{field}", op, light, field) for field in FIELDS for op in OPS for light in LIGHTS]
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def random_image(size, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (size, size, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def disc_image(size):
    jj, ii = np.mgrid[0:size, 0:size]
    inside = np.hypot(ii + 0.5 - size / 2.0, jj + 0.5 - size / 2.0) <= 0.35 * size
    return np.repeat((inside * 255).astype(np.uint8)[..., None], 4, axis=2)


def from_trace(path, cases, calls):
    """The dispatches of k_image_lighting in start order: `calls` per case, in the order the tool ran the cases (warm-up first, case by case;
    then the windows, interleaved); k_image_convolve's and k_image_color_filter's beside them."""
    rows = {"k_image_lighting": [], "k_image_convolve": [], "k_image_color_filter": []}
    with open(path) as f:
        for row in csv.DictReader(f):
            for kernel in rows:
                if kernel in row["Kernel_Name"]:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    warmup, steps, repeats = calls
    for found in rows.values():
        found.sort()
    assert len(rows["k_image_lighting"]) == len(cases) * (warmup + steps * repeats), len(rows["k_image_lighting"])
    beside = {kernel: round(float(np.median([d for _, d in rows[kernel][warmup:]])) / 1e3, 1) if rows[kernel] else None for kernel in ("k_image_convolve", "k_image_color_filter")}
    for k, case in enumerate(cases):
        timed = []
        for w in range(repeats):
            at = len(cases) * warmup + (w * len(cases) + k) * steps
            timed += [d for _, d in rows["k_image_lighting"][at:at + steps]]
        print(json.dumps({"case": case[0], "k_image_lighting_us": round(float(np.median(timed)) / 1e3, 1), "k_image_convolve_us": beside["k_image_convolve"],
                          "k_image_color_filter_us": beside["k_image_color_filter"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. diffuse_distant_random,specular_spot_layer")
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
    from contrast_renderer_amd import BlurEdge, ColorMatrix, DistantLight, LightingOp, PointLight, SpotLight
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    size = args.size
    fields = {"random": R.Image(r, random_image(size, 7)), "layer": R.Image(r, disc_image(size)).blur(8.0, edge=BlurEdge.Pad)}
    lights = {"distant": DistantLight(225.0, 40.0), "point": PointLight(0.3 * size, 0.2 * size, 0.25 * size),
              "spot": SpotLight((0.1 * size, 0.1 * size, 0.5 * size), (0.55 * size, 0.5 * size, 0.0), 4.0, 35.0)}
    ops = {"diffuse": LightingOp.Diffuse, "specular": LightingOp.Specular}
    src, dst = torch.randint(0, 255, (size * size * 4,), dtype=torch.uint8, device="cuda"), torch.empty(size * size * 4, dtype=torch.uint8, device="cuda")
    matrix = ColorMatrix.saturate(0.5)
    dense = [[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]]

    def lighting(case):
        fields[case[3]].lighting(lights[case[2]], ops[case[1]], 5.0, 1.0, 20.0, (1.0, 0.9, 0.8), BlurEdge.Pad).destroy()

    def convolve(_):
        fields["random"].convolve(dense, edge=BlurEdge.Pad).destroy()

    def color_filter(_):
        fields["random"].color_filter(matrix).destroy()

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
            lighting(case)
    for _ in range(max(args.warmup, 1)):
        convolve(None)
        color_filter(None)
        copy(None)
    windows = {case[0]: [] for case in cases}
    convolve_windows, filter_windows, copy_windows = [], [], []
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case in cases:
            window(lighting, case, windows[case[0]])
        window(convolve, None, convolve_windows)
        window(color_filter, None, filter_windows)
        window(copy, None, copy_windows)
    middle = lambda values: sorted(values)[len(values) // 2]  # noqa: E731
    convolve_ms, filter_ms, copy_ms = middle(convolve_windows), middle(filter_windows), middle(copy_windows)
    for name, op, light, field in cases:
        w = sorted(windows[name])
        ms = middle(w)
        print(json.dumps({"case": name, "size": size, "op": op, "light": light, "field": field, "ms_per_call": round(ms, 4), "best_ms": round(w[0], 4), "spread": round(w[-1] - w[0], 4),
                          "convolve3_ms": round(convolve_ms, 4), "color_filter_ms": round(filter_ms, 4), "copy_ms": round(copy_ms, 4), "ratio_to_convolve3": round(ms / convolve_ms, 2),
                          "gtexel_per_s": round(size * size / (ms * 1e-3) / 1e9, 2), "windows": [round(v, 4) for v in windows[name]]}))


if __name__ == "__main__":
    main()
