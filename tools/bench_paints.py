#!/usr/bin/env python3
"""GPU: the S10k step (10 000 cubic fills at 4096^2, msaa 1: clear + render_resident + synchronize) with solid colours and with gradient paints.
Six variants, interleaved window by window: solid colours on the fast path; solid colours on k_raster_blend (an additive blend state); every
instance with a 2-stop linear paint; every instance with an 8-stop radial REFLECT paint; every instance with a 4-stop conic PAD paint over a
full turn; every instance with an 8-stop conic REFLECT paint over a quarter turn (the four painted ones on k_raster_paint under "over").
Prints one JSON line per variant: {"variant", "ms_per_step" (median of --repeats windows of --steps steps), "spread" (max - min of the windows)}.
--label TEXT adds "build": TEXT to every line, for files that hold the lines of several builds. --variants a,b runs those alone (a library
from before the conic kind runs the first four). The instantiation of k_raster_paint that is measured follows the scene, the sample count and
the target: --scene strokes draws the dashed-stroke scene (2 000 paths) in place of S10k, --msaa N the scene at N samples, --format attachment
a target that rounds every write; each is then part of "build".
Usage: tools/bench_paints.py [--steps 40] [--warmup 10] [--repeats 5] [--label TEXT] [--variants a,b] [--scene fills|strokes] [--msaa N] [--format rgba8|attachment]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from contrast_renderer_amd import renderer as R, scenes  # noqa: E402
from contrast_renderer_amd.renderer import BlendComponent, BlendFactor, BlendOperation, BlendState, ColorTargetState, Paint, Spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default=None)
    ap.add_argument("--variants", default=None)
    ap.add_argument("--scene", choices=["fills", "strokes"], default="fills")
    ap.add_argument("--msaa", type=int, default=1)
    ap.add_argument("--format", choices=["rgba8", "attachment"], default="rgba8")
    args = ap.parse_args()
    sc = scenes.scene_cubic_fill(n_paths=10000, size=(4096, 4096)) if args.scene == "fills" else scenes.scene_dashed_strokes(msaa=args.msaa)
    sc["msaa"] = args.msaa
    fmt = R.FORMAT_RGBA8 if args.format == "rgba8" else R.FORMAT_RGBA8_ATTACHMENT
    label = args.label if (args.scene, args.msaa, args.format) == ("fills", 1, "rgba8") else f"{args.label or ''} [{args.scene}, msaa {args.msaa}, {args.format}]".strip()
    n = len(np.asarray(sc["colors"]).reshape(-1, 4))
    add = BlendComponent(BlendFactor.One, BlendFactor.One, BlendOperation.Add)
    rng = np.random.RandomState(1)
    linear = [Paint.linear((-1.0, -1.0), (1.0, 1.0), [(0.0, (1.0, 0.2, 0.1, 1.0)), (1.0, (0.1, 0.3, 1.0, 0.6))])]
    radial = [Paint.radial((0.0, 0.0), 0.5, [(i / 7.0, tuple(float(v) for v in rng.uniform(0.2, 1.0, 4))) for i in range(8)], Spread.Reflect)]
    conic_turn = conic_quarter = None
    if args.variants is None or "conic" in args.variants:
        conic_turn = [Paint.conic((0.0, 0.0), 0.0, float(np.float32(2.0 * np.pi)), [(i / 3.0, tuple(float(v) for v in rng.uniform(0.2, 1.0, 4))) for i in range(4)])]
        conic_quarter = [Paint.conic((0.0, 0.0), 0.5, 0.5 + 0.5 * np.pi, [(i / 7.0, tuple(float(v) for v in rng.uniform(0.2, 1.0, 4))) for i in range(8)], Spread.Reflect)]
    variants = {"solid_fast_path": (None, None), "solid_blend_additive": (ColorTargetState(BlendState(add, add)), None),
                "linear_2_stops": (None, linear), "radial_8_stops_reflect": (None, radial),
                "conic_4_stops_pad_turn": (None, conic_turn), "conic_8_stops_reflect_quarter": (None, conic_quarter)}
    if args.variants is not None:
        variants = {name: variants[name] for name in args.variants.split(",")}
    runs = {}
    for name, (blending, paints) in variants.items():
        r = R.Renderer(R.Configuration(msaa_sample_count=sc["msaa"], winding_counter_bits=sc["winding_bits"], blending=blending), device=0)
        scene = R.Scene(r, sc["batch"])
        assert scene.status() == 0
        scene.set_instances(sc["transforms"], sc["colors"])
        if paints:
            scene.set_paints(paints, [0] * n)
        runs[name] = (r, scene, R.Frame(r, sc["width"], sc["height"], format=fmt))

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
        print(json.dumps({**({"build": label} if label else {}), "variant": name, "ms_per_step": round(w[len(w) // 2], 4), "spread": round(w[-1] - w[0], 4), "windows": [round(v, 4) for v in windows[name]]}))


if __name__ == "__main__":
    main()
