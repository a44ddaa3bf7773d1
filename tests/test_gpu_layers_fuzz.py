"""Stateful fuzz of the image and layer pipeline on the GPU: the op sequences of tests/layers_model.py replayed on one Renderer — images created,
snapshot from frames in whatever state, made of noise, blurred, composited, colour filtered, eroded and dilated, convolved, lit, displaced,
turned into distance fields, resized, mipmapped, destroyed behind the call that read them, loaded back into frames and drawn as image paints
through tables that outlive their images, between clears, uploads, plain passes, re-uploads of a Scene that holds a paint table and calls
that the library refuses, which must leave the pool and the image they named as they were. The host model has an exact expectation for
every step, so every download is compared byte for byte, with no tolerance and no excluded texel."""
import os

import numpy as np
import pytest

from contrast_renderer_amd import Path, batch_from_shapes
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import (BlurEdge, Channel, ContrastError, DistanceMode, DistantLight, Filter, Image, ImagePaint, LightingOp, MorphologyOp, PointLight,
                                            ResizeFilter, SpotLight, TurbulenceKind)

import layers_model as L
import lighting_model as LM
from test_gpu_blending import last_pass, no_pins  # noqa: F401

pytestmark = pytest.mark.gpu
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _seeds():
    return range(int(os.environ.get("CRH_FUZZ_LAYER_SEEDS", "12")))


def blit_scene(r, width, height):
    """test_gpu_image_paints._blit for a frame that is no square: one rectangle over the whole frame, path coordinates = pixel coordinates."""
    scene = R.Scene(r, batch_from_shapes([([], [Path.from_rect((width / 2.0, height / 2.0), (width / 2.0, height / 2.0))])]))
    t = np.zeros(16, dtype=np.float32)
    t[0], t[5], t[10], t[15], t[12], t[13] = 2.0 / width, -2.0 / height, 1.0, 1.0, -1.0, 1.0
    return scene, t.reshape(1, 16)


def white_paint_of(r, white):
    image = Image(r, np.full((white["size"][1], white["size"][0], 4), 255, dtype=np.uint8))
    if white["mip"]:
        image.generate_mipmaps()
    return image, ImagePaint(image, white["matrix"], white["filter"], *white["spreads"])


def light_of(light):
    """The library's light of an op's `light`, the keyword arguments of lighting_model.Light."""
    if light["kind"] == LM.DISTANT:
        return DistantLight(light["azimuth"], light["elevation"])
    if light["kind"] == LM.POINT:
        return PointLight(*light["position"])
    return SpotLight(tuple(light["position"]), tuple(light["points_at"]), light["spot_exponent"], light["cone_angle"])


def describe(op):
    """The op's dictionary with its arrays named by shape: what a failure message prints."""
    return {k: (f"<{v.dtype} {v.shape}>" if isinstance(v, np.ndarray) else (tuple(describe({0: x})[0] for x in v) if isinstance(v, tuple) else v)) for k, v in op.items()}


@pytest.mark.parametrize("seed", _seeds())
def test_random_layer_pipelines_against_a_host_model(seed, oracle_lib, no_pins):
    setup, ops = L.generate(seed)
    model = L.Model(setup)
    batch = model.batch
    w, h = setup["width"], setup["height"]
    r = R.Renderer(R.Configuration(msaa_sample_count=setup["msaa"]), device=0)
    frames = [R.Frame(r, w, h, fmt) for fmt in L.FORMATS]
    for f in frames:
        f.clear()
    solid = R.Scene(r, batch.slice_shapes(*setup["slice"]))
    assert solid.status() == 0
    blits = [blit_scene(r, w, h) for _ in frames]
    white = np.float32([[1.0, 1.0, 1.0, 1.0]])
    pool = []

    def compare(got, expect, step, op, what):
        assert got.shape == expect.shape, f"seed {seed} op {step} {describe(op)}: {what} has the shape {got.shape}, not {expect.shape}"
        bad = (got != expect).any(axis=2)
        assert not bad.any(), (f"seed {seed} op {step} {describe(op)}: {what}: {int(bad.sum())} of {bad.size} texels differ, "
                               f"first at (row, column) {tuple(int(v) for v in np.argwhere(bad)[0])}")

    def render_solid(op):
        frame = frames[op["frame"]]
        if "instances" in op:
            solid.render(frame, *op["instances"])
        else:
            solid.render(frame)
        return last_pass(frame)

    for step, op in enumerate(ops):
        kind = op["kind"]
        where = f"seed {seed} op {step} {describe(op)}"
        expect = model.apply(op)
        if kind == "create":
            pool.append(Image(r, op["pixels"]))
        elif kind == "snapshot":
            pool.append(Image.from_frame(frames[op["frame"]]))
        elif kind == "blur":
            pool.append(pool[op["image"]].blur(op["sigma"][0], op["sigma"][1], BlurEdge(op["edge"])))
        elif kind == "composite":
            pool.append(pool[op["image"]].composite(pool[op["source"]], op["op"], op["mode"], op["opacity"], op["offset"]))
        elif kind == "color_filter":
            pool.append(pool[op["image"]].color_filter(op["matrix"], op["tables"]))
        elif kind == "morphology":
            pool.append(pool[op["image"]].morphology(MorphologyOp(op["op"]), op["radius"][0], op["radius"][1], BlurEdge(op["edge"])))
        elif kind == "convolve":
            pool.append(pool[op["image"]].convolve(op["kernel"], op["divisor"], op["bias"], op["target"], BlurEdge(op["edge"]), op["preserve_alpha"]))
        elif kind == "lighting":
            pool.append(pool[op["image"]].lighting(light_of(op["light"]), LightingOp(op["op"]), op["surface_scale"], op["constant"], op["specular_exponent"], op["color"], BlurEdge(op["edge"])))
        elif kind == "turbulence":
            pool.append(Image.turbulence(r, op["size"][0], op["size"][1], op["frequency"], op["octaves"], op["seed"], TurbulenceKind(op["noise"]), op["stitch"], op["opaque"], op["offset"]))
        elif kind == "displace":
            pool.append(pool[op["image"]].displace(pool[op["map"]], op["scale"], Channel(op["channels"][0]), Channel(op["channels"][1]), Filter(op["filter"]), BlurEdge(op["edge"])))
        elif kind == "distance_field":
            pool.append(pool[op["image"]].distance_field(op["spread"], DistanceMode(op["mode"]), Channel(op["channel"]), op["threshold"], BlurEdge(op["edge"])))
        elif kind == "resize":
            pool.append(pool[op["image"]].resize(op["size"][0], op["size"][1], ResizeFilter(op["filter"])))
        elif kind == "refused":  # plain integers: the enumerations have no member for what the header refuses
            image, how = pool[op["image"]], op["arguments"]
            with pytest.raises(ContrastError) as refused:
                if op["call"] == "distance_field":
                    image.distance_field(how["spread"], how["mode"], how["channel"], how["threshold"], how["edge"])
                else:
                    image.resize(how["size"][0], how["size"][1], how["filter"])
            assert refused.value.status == op["status"], f"{where}: the status is {refused.value.status}"
            assert len(pool) == len(model.pool), where
            compare(image.download_level(0), expect[0], step, op, "the image a refused call named")
        elif kind == "mipmaps":
            pool[op["image"]].generate_mipmaps()
        elif kind == "check_image":
            image = pool[op["image"]]
            assert image.origin == op["origin"], f"{where}: the origin is {image.origin}, not {op['origin']}"
            assert image.levels == len(expect), f"{where}: {image.levels} levels, not {len(expect)}"
            for level, e in enumerate(expect):
                compare(image.download_level(level), e, step, op, f"level {level}")
        elif kind == "destroy_image":
            pool.pop(op["image"]).destroy()
        elif kind == "clear":
            frames[op["frame"]].clear()
        elif kind == "solid":
            tap = render_solid(op)
            assert tap["general"] == 0 and tap["raster"] != "none", f"{where}: {tap}"  # no table: the pass is not a painted one
        elif kind == "upload":
            frames[op["frame"]].upload(op["pixels"])
        elif kind == "load_image":
            frames[op["frame"]].load_image(pool[op["image"]])
        elif kind == "download":
            compare(frames[op["frame"]].download(), expect[0], step, op, f"frame {op['frame']}")
        elif kind in ("set_table", "replace_table", "blit_mip"):
            blits[op["frame"]][0].set_paints([ImagePaint(pool[op["image"]], IDENTITY, Filter(op["filter"]))], [0])
        elif kind == "clear_table":
            blits[op["frame"]][0].set_paints([], [])
        if kind in ("blit", "blit_mip"):
            scene, t = blits[op["frame"]]
            scene.render(frames[op["frame"]], t, white)
            tap = last_pass(frames[op["frame"]])
            assert tap["general"] == 1 and tap["raster"] == "ops", f"{where}: {tap}"
        elif kind == "white_paint":
            image, paint = white_paint_of(r, op["white"])
            solid.set_paints([paint], [0] * solid.n_shapes)
            image.destroy()
            tap = render_solid(op)
            assert tap["general"] == 1 and tap["raster"] == "ops", f"{where}: {tap}"
            solid.set_paints([], [])
        elif kind == "reupload":
            image, paint = white_paint_of(r, op["white"])
            solid.set_paints([paint], [-1] * op["assoc_first"] + [0] * (op["assoc_length"] - op["assoc_first"]))
            solid = R.Scene(r, batch.slice_shapes(*op["slice"]), existing=solid)  # the table and the association stay with the Scene
            assert solid.status() == 0, where
            tap = render_solid(op)
            assert tap["general"] == L.Model.expected_general(op) and tap["raster"] != "none", f"{where}: {tap}"
            solid.set_paints([], [])
            image.destroy()
    assert len(pool) == len(model.pool)
