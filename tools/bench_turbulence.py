#!/usr/bin/env python3
"""GPU: Image.turbulence (crh_image_turbulence: the tables built on the host and uploaded, k_image_turbulence, the allocation and the wait
included — the call is synchronous) at 4096^2 for each (kind, opaque, stitched) and 1, 4 and 10 octaves, at a base frequency of 0.01 cells
per texel and a fractional offset. The cases are interleaved window by window. Beside them, timed the same way in the same run:
Image.lighting, specular under a spot light on a random height field (k_image_lighting<specular, spot>: the sibling that binary64
instruction issue bounds) and a device-to-device copy of an image of the size (torch, the floor).
Prints one JSON line per case: {"case", "size", "kind", "opaque", "stitch", "octaves", "ms_per_call" (median of --repeats windows of --steps
calls), "best_ms", "spread" (max - min of the windows), "specular_spot_ms", "copy_ms", "ratio_to_specular_spot", "gtexel_per_s", "windows"}.
--library FILE loads another build of the library (one compiled with -DCRH_TURBULENCE_ROWS=... or -DCRH_TURBULENCE_PLAIN_MODULO=1: how the
variants of DESIGN.md were measured).
--from-trace FILE reads the kernel trace (csv) of a run of this tool under `rocprofv3 --kernel-trace --stats -f csv` with the same --only,
--warmup, --steps and --repeats, and prints the median time of k_image_turbulence per case and of k_image_lighting instead (nothing runs).
Usage: tools/bench_turbulence.py [--size 4096] [--steps 5] [--warmup 2] [--repeats 5] [--only fractal_rgba_plain_10,...] [--library FILE] [--from-trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KINDS = ("fractal", "turbulence")
OCTAVES = (1, 4, 10)


def cases_of(only):
    cases = [(f"{kind}_{'opaque' if opaque else 'rgba'}_{'stitched' if stitch else 'plain'}_{octaves}", kind, opaque, stitch, octaves)
             for kind in KINDS for opaque in (False, True) for stitch in (False, True) for octaves in OCTAVES]
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    return cases


def random_image(size, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (size, size, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def from_trace(path, cases, calls):
    """The dispatches of k_image_turbulence in start order: `calls` per case, in the order the tool ran the cases (warm-up first, case by
    case; then the windows, interleaved); k_image_lighting's beside them."""
    rows = {"k_image_turbulence": [], "k_image_lighting": []}
    with open(path) as f:
        for row in csv.DictReader(f):
            for kernel in rows:
                if kernel in row["Kernel_Name"]:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    warmup, steps, repeats = calls
    for found in rows.values():
        found.sort()
    assert len(rows["k_image_turbulence"]) == len(cases) * (warmup + steps * repeats), len(rows["k_image_turbulence"])
    lighting = round(float(np.median([d for _, d in rows["k_image_lighting"][warmup:]])) / 1e3, 1) if rows["k_image_lighting"] else None
    for k, case in enumerate(cases):
        timed = []
        for w in range(repeats):
            at = len(cases) * warmup + (w * len(cases) + k) * steps
            timed += [d for _, d in rows["k_image_turbulence"][at:at + steps]]
        print(json.dumps({"case": case[0], "k_image_turbulence_us": round(float(np.median(timed)) / 1e3, 1), "k_image_lighting_specular_spot_us": lighting}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated case names, e.g. fractal_rgba_plain_10,turbulence_opaque_stitched_4")
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
    from contrast_renderer_amd import BlurEdge, LightingOp, SpotLight, TurbulenceKind
    from contrast_renderer_amd import renderer as R
    r = R.Renderer(R.Configuration(), device=0)
    size = args.size
    field = R.Image(r, random_image(size, 7))
    spot = SpotLight((0.1 * size, 0.1 * size, 0.5 * size), (0.55 * size, 0.5 * size, 0.0), 4.0, 35.0)
    kinds = {"fractal": TurbulenceKind.FractalNoise, "turbulence": TurbulenceKind.Turbulence}
    src, dst = torch.randint(0, 255, (size * size * 4,), dtype=torch.uint8, device="cuda"), torch.empty(size * size * 4, dtype=torch.uint8, device="cuda")

    def turbulence(case):
        R.Image.turbulence(r, size, size, (0.01, 0.013), case[4], 11, kinds[case[1]], case[3], case[2], (0.5, 0.25)).destroy()

    def lighting(_):
        field.lighting(spot, LightingOp.Specular, 5.0, 1.0, 20.0, (1.0, 0.9, 0.8), BlurEdge.Pad).destroy()

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
            turbulence(case)
    for _ in range(max(args.warmup, 1)):
        lighting(None)
        copy(None)
    windows = {case[0]: [] for case in cases}
    lighting_windows, copy_windows = [], []
    for _ in range(args.repeats):  # the cases interleaved window by window: drift of the clock hits them alike
        for case in cases:
            window(turbulence, case, windows[case[0]])
        window(lighting, None, lighting_windows)
        window(copy, None, copy_windows)
    middle = lambda values: sorted(values)[len(values) // 2]  # noqa: E731
    lighting_ms, copy_ms = middle(lighting_windows), middle(copy_windows)
    for name, kind, opaque, stitch, octaves in cases:
        w = sorted(windows[name])
        ms = middle(w)
        print(json.dumps({"case": name, "size": size, "kind": kind, "opaque": opaque, "stitch": stitch, "octaves": octaves, "ms_per_call": round(ms, 4), "best_ms": round(w[0], 4),
                          "spread": round(w[-1] - w[0], 4), "specular_spot_ms": round(lighting_ms, 4), "copy_ms": round(copy_ms, 4), "ratio_to_specular_spot": round(ms / lighting_ms, 2),
                          "gtexel_per_s": round(size * size / (ms * 1e-3) / 1e9, 2), "windows": [round(v, 4) for v in windows[name]]}))


if __name__ == "__main__":
    main()
