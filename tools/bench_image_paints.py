#!/usr/bin/env python3
"""GPU: the S10k step (10 000 cubic fills at 4096^2, msaa 1: clear + render_resident + synchronize) with solid colours, a gradient and image paints.
Five variants, interleaved window by window: solid colours on the fast path; every instance with a 2-stop linear gradient (k_raster_paint); every
instance with an image paint of a 256x256 image, NEAREST and LINEAR, and LINEAR with a 2048x2048 image (16 MiB of texels: beyond an XCD's L2)
— the three on k_raster_image. The images are random premultiplied texels, REPEAT on both axes, about four texels per path unit turned by 0.4 rad.
A build without image paints (the parent commit) runs the first two variants only: the baseline the others are read against.
Prints one JSON line per variant: {"variant", "ms_per_step" (median of --repeats windows of --steps steps), "spread" (max - min of the windows)}.
Usage: tools/bench_image_paints.py [--steps 40] [--warmup 10] [--repeats 5] [--only image_256_linear,...]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from contrast_renderer_amd import renderer as R, scenes  # noqa: E402
from contrast_renderer_amd.renderer import Paint  # noqa: E402


def random_image(size, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(64, 256, (size, size, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated variant names (a kernel trace of one variant)")
    args = ap.parse_args()
    sc = scenes.scene_cubic_fill(n_paths=10000, size=(4096, 4096))
    n = len(np.asarray(sc["colors"]).reshape(-1, 4))
    linear = [Paint.linear((-1.0, -1.0), (1.0, 1.0), [(0.0, (1.0, 0.2, 0.1, 1.0)), (1.0, (0.1, 0.3, 1.0, 0.6))])]
    variants = {"solid_fast_path": None, "linear_2_stops": lambda r: linear}
    if hasattr(R, "ImagePaint"):
        def textured(size, filter):
            def make(r):
                s = 4.0 * size / 256.0  # the image spans the same path distance at either size: texels per path unit scale with it
                c, k = s * math.cos(0.4), s * math.sin(0.4)
                return [R.ImagePaint(R.Image(r, random_image(size, 7)), (c, -k, size / 2.0, k, c, size / 2.0), filter, R.Spread.Repeat, R.Spread.Repeat)]
            return make
        variants.update({"image_256_nearest": textured(256, R.Filter.Nearest), "image_256_linear": textured(256, R.Filter.Linear),
                         "image_2048_linear": textured(2048, R.Filter.Linear)})
    if args.only:
        variants = {name: variants[name] for name in args.only.split(",")}
    runs = {}
    for name, paints in variants.items():
        r = R.Renderer(R.Configuration(msaa_sample_count=sc["msaa"], winding_counter_bits=sc["winding_bits"]), device=0)
        scene = R.Scene(r, sc["batch"])
        assert scene.status() == 0
        scene.set_instances(sc["transforms"], sc["colors"])
        if paints:
            scene.set_paints(paints(r), [0] * n)
        runs[name] = (r, scene, R.Frame(r, sc["width"], sc["height"]))

    def step(scene, frame):
        frame.clear()
        scene.render(frame)

    for _, scene, frame in runs.values():
        for _ in range(args.warmup):
            step(scene, frame)
        frame.synchronize()
    windows = {name: [] for name in runs}
    for _ in range(args.repeats):  # the variants interleaved window by window: drift of the clock hits them alike
        for name, (_, scene, frame) in runs.items():
            frame.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(scene, frame)
            frame.synchronize()
            windows[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    for name in runs:
        w = sorted(windows[name])
        print(json.dumps({"variant": name, "ms_per_step": round(w[len(w) // 2], 4), "spread": round(w[-1] - w[0], 4), "windows": [round(v, 4) for v in windows[name]]}))


if __name__ == "__main__":
    main()
