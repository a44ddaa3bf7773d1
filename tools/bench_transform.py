#!/usr/bin/env python3
"""GPU: Image.resample (crh_image_transform: k_image_transform, the allocation and the wait included — the call is synchronous) on a
random 4096^2 image under the TRANSPARENT edge, for each filter (nearest, linear, cubic) and five matrices: `identity`, `rotate_30`
(about the middle, into a result of the source's size), `turn_90`, `scale_0.5` (the layer at half its size: a 2048^2 result that reads
every other texel) and `perspective` (a tilt about the top edge, w from 1 to 1.41 down the image). Beside them, timed the same way in
the same process, the yardsticks, which are existing code: Image.displace with scale (0, 0) under LINEAR and NEAREST (k_image_displace:
the same gather plus a map read), Image.color_filter with a matrix and no tables (k_image_color_filter: a stream of 8 bytes per texel)
and a device-to-device copy of an image of the size (torch, the floor). The cases are interleaved window by window; a window is as many
calls as fill --window-ms (measured in the warm-up), at least 3.
Prints one JSON line per case: {"case", "library", "round", "size", "result", "ms_per_call" (median of --repeats windows), "best_ms",
"spread" (max - min of the windows), "steps", "ratio_to_displace" (of the best windows, to displace of the same filter; cubic to
LINEAR's), "ratio_to_color_filter" (likewise), "gtexel_per_s" (result texels), "windows"}.
--libraries A,B,... measures several builds of the library (one compiled with -DCRH_TRANSFORM_BLOCK=64 or 16: how the lane mappings of
DESIGN.md were compared), each in a fresh child process, alternating them --rounds times in this one call; `default` is the package's.
Usage: tools/bench_transform.py [--size 4096] [--window-ms 250] [--warmup 2] [--repeats 5] [--only linear_rotate_30,...] [--libraries default,FILE,...] [--rounds 2]"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FILTERS = ("nearest", "linear", "cubic")
MATRICES = ("identity", "rotate_30", "turn_90", "scale_0.5", "perspective")
YARDSTICKS = ("displace_nearest", "displace_linear", "color_filter", "copy")


def matrix_of(name, size):
    """-> (result -> source matrix, result size)"""
    c, s, half = math.cos(math.radians(30.0)), math.sin(math.radians(30.0)), size / 2.0
    return {"identity": ((1, 0, 0, 0, 1, 0, 0, 0, 1), size), "rotate_30": ((c, -s, half - c * half + s * half, s, c, half - s * half - c * half, 0, 0, 1), size),
            "turn_90": ((0, 1, 0, -1, 0, size, 0, 0, 1), size), "scale_0.5": ((2, 0, 0, 0, 2, 0, 0, 0, 1), size // 2),
            "perspective": ((1, 0, 0, 0, 1, 0, 0, 0.41 / size, 1), size)}[name]


def random_image(size, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (size, size, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def measure(args, library, round_index):
    import torch
    from contrast_renderer_amd import _ffi
    if library != "default":
        _ffi.LIB_PATH = os.path.abspath(library)
    from contrast_renderer_amd import BlurEdge, Channel, ColorMatrix, Filter, TransformFilter
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    size = args.size
    source = R.Image(r, random_image(size, 7))
    map_image = R.Image(r, random_image(size, 8))
    filters = {"nearest": TransformFilter.Nearest, "linear": TransformFilter.Linear, "cubic": TransformFilter.Cubic}
    matrix = ColorMatrix.saturate(0.4)
    src, dst = torch.randint(0, 255, (size * size * 4,), dtype=torch.uint8, device="cuda"), torch.empty(size * size * 4, dtype=torch.uint8, device="cuda")

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    calls = {}
    for filter in FILTERS:
        for name in MATRICES:
            m, result = matrix_of(name, size)
            calls[f"{filter}_{name}"] = (lambda m=m, result=result, filter=filter: source.resample(m, result, result, filters[filter], BlurEdge.Transparent).destroy(), result)
    calls["displace_nearest"] = (lambda: source.displace(map_image, 0.0, Channel.R, Channel.G, Filter.Nearest, BlurEdge.Transparent).destroy(), size)
    calls["displace_linear"] = (lambda: source.displace(map_image, 0.0, Channel.R, Channel.G, Filter.Linear, BlurEdge.Transparent).destroy(), size)
    calls["color_filter"] = (lambda: source.color_filter(matrix).destroy(), size)
    calls["copy"] = (copy, size)
    names = [n for n in calls if n in YARDSTICKS or not args.only or n in args.only.split(",")]
    steps = {}
    for name in names:  # the warm-up, which also sizes the window
        for _ in range(args.warmup):
            calls[name][0]()
        t0 = time.perf_counter()
        calls[name][0]()
        steps[name] = max(3, int(math.ceil(args.window_ms / max((time.perf_counter() - t0) * 1e3, 1e-3))))
    windows = {name: [] for name in names}
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for name in names:
            t0 = time.perf_counter()
            for _ in range(steps[name]):
                calls[name][0]()
            windows[name].append((time.perf_counter() - t0) * 1e3 / steps[name])
    middle = lambda values: sorted(values)[len(values) // 2]  # noqa: E731
    yard = {name: min(windows[name]) for name in YARDSTICKS}  # the ratios are of best windows: a slow window (an allocation that stalls, other work on the machine) is not the kernel's
    for name in names:
        w, ms, result = sorted(windows[name]), middle(windows[name]), calls[name][1]
        displace = yard["displace_nearest"] if name.startswith("nearest") or name == "displace_nearest" else yard["displace_linear"]
        print(json.dumps({"case": name, "library": os.path.basename(library), "round": round_index, "size": size, "result": result, "ms_per_call": round(ms, 4), "best_ms": round(w[0], 4),
                          "spread": round(w[-1] - w[0], 4), "steps": steps[name], "ratio_to_displace": round(w[0] / displace, 3), "ratio_to_color_filter": round(w[0] / yard["color_filter"], 3),
                          "gtexel_per_s": round(result * result / (ms * 1e-3) / 1e9, 2), "windows": [round(v, 4) for v in windows[name]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. linear_rotate_30,cubic_turn_90 (the yardsticks always run)")
    ap.add_argument("--libraries", default="default", help="comma-separated builds of libcontrast_hip.so; `default` is the package's")
    ap.add_argument("--rounds", type=int, default=1, help="how often the list of libraries is gone through, each build in a fresh process each time")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        measure(args, args.child, args.round)
        return
    libraries = args.libraries.split(",")
    if libraries == ["default"] and args.rounds == 1:
        measure(args, "default", 0)
        return
    for round_index in range(args.rounds):
        for library in libraries:  # one process at a time: a fresh child per build, so that no two builds share a process
            forwarded = [a for a in sys.argv[1:]]
            status = subprocess.run([sys.executable, os.path.abspath(__file__)] + forwarded + ["--child", library, "--round", str(round_index)], timeout=600).returncode
            if status != 0:
                sys.exit(f"{library} (round {round_index}) ended with status {status}: nothing more is started")


if __name__ == "__main__":
    main()
