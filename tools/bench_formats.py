#!/usr/bin/env python3
"""GPU: the S10k step (10 000 cubic fills at 4096^2, msaa 1: clear + render_resident + synchronize) per frame format.
Prints one JSON line per format: {"format", "ms_per_step" (median of --repeats windows of --steps steps), "spread" (max - min of the windows)}.
Usage: tools/bench_formats.py [--steps 50] [--warmup 10] [--repeats 5] [--formats RGBA8,BGRA8,RGBA8_SRGB,RGBA8_SRGB_ATTACHMENT]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from contrast_renderer_amd import renderer as R, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--formats", default="RGBA8,BGRA8,RGBA8_SRGB,RGBA8_SRGB_ATTACHMENT")
    args = ap.parse_args()
    sc = scenes.scene_cubic_fill(n_paths=10000, size=(4096, 4096))
    r = R.Renderer(R.Configuration(msaa_sample_count=sc["msaa"], winding_counter_bits=sc["winding_bits"]), device=0)
    scene = R.Scene(r, sc["batch"])
    assert scene.status() == 0
    scene.set_instances(sc["transforms"], sc["colors"])
    names = args.formats.split(",")
    frames = {name: R.Frame(r, sc["width"], sc["height"], getattr(R, "FORMAT_" + name)) for name in names}

    def step(frame):
        frame.clear()
        scene.render(frame)

    for frame in frames.values():
        for _ in range(args.warmup):
            step(frame)
        frame.synchronize()
    windows = {name: [] for name in names}
    for _ in range(args.repeats):  # the formats interleaved window by window: drift of the clock hits them alike
        for name, frame in frames.items():
            frame.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(frame)
            frame.synchronize()
            windows[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    for name in names:
        w = sorted(windows[name])
        print(json.dumps({"format": name, "ms_per_step": round(w[len(w) // 2], 4), "spread": round(w[-1] - w[0], 4), "windows": [round(v, 4) for v in windows[name]]}))


if __name__ == "__main__":
    main()
