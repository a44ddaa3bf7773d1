#!/usr/bin/env python3
"""GPU: the S10k step (10 000 cubic fills at 4096^2, msaa 1: clear + render_resident + synchronize) with mipmapped image paints.
Seven variants, interleaved window by window: solid colours on the fast path; every instance with an image paint of a 2048x2048 image, LINEAR
(k_raster_image) and LINEAR | MIPMAP (k_raster_mip), at three placements — magnified for every instance (half a texel per pixel where the scene
draws largest in texels: lod 0, k_raster_mip skips the second level's fetch), the placement of tools/bench_image_paints.py (32 texels per path
unit: the scene's instances span 8 to 128 pixels per unit, so lod 0 to 2), and minified (eight texels per pixel or more: lod 3 to 7, two levels
and eight texels per sample; plain LINEAR aliases there). The image is random premultiplied texels, REPEAT on both axes, turned by 0.4 rad.
Prints one JSON line per variant: {"variant", "ms_per_step" (median of --repeats windows of --steps steps), "spread" (max - min of the windows)}.
Usage: tools/bench_mipmaps.py [--steps 40] [--warmup 10] [--repeats 5] [--only minified_linear_mipmap,...]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from contrast_renderer_amd import renderer as R, scenes  # noqa: E402

SIZE = 2048


def random_image(size, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(64, 256, (size, size, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)


def pixels_per_unit(transforms):
    """-> (the smallest, the largest) scale of path units to pixels among the instances (4096^2 frame)."""
    t = np.asarray(transforms, dtype=np.float64).reshape(-1, 16)
    sv = np.array([np.linalg.svd(np.array([[m[0], m[4]], [m[1], m[5]]]) * 2048.0, compute_uv=False) for m in t])
    return float(sv.min()), float(sv.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated variant names (a kernel trace of one variant)")
    args = ap.parse_args()
    sc = scenes.scene_cubic_fill(n_paths=10000, size=(4096, 4096))
    n = len(np.asarray(sc["colors"]).reshape(-1, 4))
    usual = 4.0 * SIZE / 256.0                          # texels per path unit of tools/bench_image_paints.py
    smallest, largest = pixels_per_unit(sc["transforms"])
    magnified = 0.5 * smallest                          # half a texel per pixel for the instance drawn smallest, fewer for the others
    minified = 8.0 * largest                            # eight texels per pixel for the instance drawn largest, more for the others
    pixels = random_image(SIZE, 7)

    def textured(texels_per_unit, filter, mipmaps):
        def make(r):
            image = R.Image(r, pixels)
            if mipmaps:
                image.generate_mipmaps()
            c, k = texels_per_unit * math.cos(0.4), texels_per_unit * math.sin(0.4)
            return [R.ImagePaint(image, (c, -k, SIZE / 2.0, k, c, SIZE / 2.0), filter, R.Spread.Repeat, R.Spread.Repeat)]
        return make
    variants = {"solid_fast_path": None,
                "magnified_linear": textured(magnified, R.Filter.Linear, False),
                "magnified_linear_mipmap": textured(magnified, R.Filter.LinearMipmap, True),
                "image_2048_linear": textured(usual, R.Filter.Linear, False),
                "image_2048_linear_mipmap": textured(usual, R.Filter.LinearMipmap, True),
                "minified_linear": textured(minified, R.Filter.Linear, False),
                "minified_linear_mipmap": textured(minified, R.Filter.LinearMipmap, True)}
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
