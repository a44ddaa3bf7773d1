"""The randomised oracle sweep through every general triangle kernel: test_gpu_fuzz.random_case(seed) drawn with the tables of
tests/painted_fuzz_model.py — gradients and conic paints whose stops carry one colour (k_raster_paint), white images with and without mipmaps
(k_raster_image, k_raster_mip), opaque colours under the blend state REPLACE (k_raster_blend) — and compared with the oracle's image of the
solid scene byte for byte: no tolerance and no excluded pixel. A painted pass clamps source and result to [0, 1] (include/contrast_hip.h);
random_case's colours lie inside, which the generator asserts."""
import functools
import os

import numpy as np
import pytest

from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image, ImagePaint

import painted_fuzz_model as PM
from test_gpu_blending import REPLACE, last_pass, no_pins  # noqa: F401
from test_gpu_fuzz import random_case

pytestmark = pytest.mark.gpu
FORMAT_NAMES = {R.FORMAT_RGBA8: "RGBA8", R.FORMAT_RGBA8_ATTACHMENT: "RGBA8_ATTACHMENT", R.FORMAT_BGRA8: "BGRA8", R.FORMAT_BGRA8_ATTACHMENT: "BGRA8_ATTACHMENT"}
SKIP_REASON = "the reference cannot tessellate this scene (covered by test_random_scene_matches_the_oracle)"


def _seeds(name, default):
    return range(int(os.environ.get(name, default)))


@functools.lru_cache(maxsize=None)
def oracle_of(seed):
    from oracle.binding import Oracle
    return Oracle(random_case(seed)["batch"])


@functools.lru_cache(maxsize=None)
def oracle_images(seed, opaque, attachment8):
    """-> (RGBA8 image, depth or None) of the single pass of random_case(seed), its colours made opaque for the replace variants: rendered once
    per session, shared by the tests and left unchanged (read only)."""
    from oracle.binding import render_pass
    c = random_case(seed)
    colours = np.array(c["colors"], dtype=np.float32, copy=True)
    if opaque:
        colours[:, 3] = 1.0
    image, depth = render_pass(oracle_of(seed), c["width"], c["height"], c["msaa"], c["winding_bits"], 2, 2, c["transforms"], colours,
                               [tuple(int(v) for v in d) for d in c["draws"]], depth=c["depth"], attachment8=attachment8, **c["state"])
    image.setflags(write=False)
    if depth is not None:
        depth.setflags(write=False)
    return image, depth


def expectation(seed, variant, fmt):
    """What a frame of format `fmt` must hold after the variant's pass: the oracle's image of variant["case"], with attachment8 for the attachment
    formats and channels 0 and 2 swapped for the BGRA ones (as tests/test_gpu_formats.py compares them)."""
    opaque = variant["blending"] == "replace"
    assert not opaque or bool((variant["case"]["colors"][:, 3] == 1.0).all())
    image, depth = oracle_images(seed, opaque, fmt in PM.ATTACHMENT_FORMATS)
    return PM.expectation_of(image, fmt), depth


def configuration(c, blending, msaa=None):
    return R.Configuration(msaa_sample_count=msaa or c["msaa"], clip_nesting_counter_bits=2, winding_counter_bits=c["winding_bits"], alpha_layer_count=2,
                           cull_mode=c["state"].get("cull_mode", 0), depth_compare=c["state"].get("depth_compare", 0),
                           depth_write_enabled=bool(c["state"].get("depth_write", 0)), blending=REPLACE if blending == "replace" else None)


def install(r, scene, variant):
    """The variant's table on the Scene -> the Images behind it (the table keeps their pixels: they may be destroyed at once)."""
    images = []
    for spec in variant["images"]:
        image = Image(r, np.full((spec["size"][1], spec["size"][0], 4), 255, dtype=np.uint8))
        if spec["mip"]:
            image.generate_mipmaps()
        images.append(image)
    table = [ImagePaint(images[p["image"]], p["matrix"], p["filter"], *p["spreads"]) if PM.is_image_paint(p) else p for p in variant["table"]]
    scene.set_paints(table, variant["assoc"])
    return images


def differing(image, expect):
    bad = (image != expect).any(axis=2)
    first = tuple(int(v) for v in np.argwhere(bad)[0]) if bad.any() else None
    return f"{int(bad.sum())} of {bad.size} pixels differ, first at (row, column) {first}: {image[first].tolist() if first else None} for {expect[first].tolist() if first else None}"


def draw(frame, scene, c, colours, draws=None):
    frame.clear()
    if c["depth"] is not None:
        frame.upload_depth(c["depth"])
    scene.render_draws(frame, c["transforms"], colours, c["draws"] if draws is None else draws)


# ---------------------------------------------------------------- a. every variant, both formats, against the oracle

@pytest.mark.parametrize("seed", _seeds("CRH_FUZZ_PAINTED_SEEDS", PM.DEFAULT_SEEDS))
def test_a_random_scene_through_every_general_kernel_matches_the_oracle(seed, oracle_lib):
    """Every variant of random_case(seed) into FORMAT_RGBA8 and the seed's second format, each pass twice (the second with its buffers sized),
    and between variants a plain solid pass with the table cleared: frame and depth attachment equal the oracle's, and every pass ran the
    general kernel. One Renderer serves "over" and one REPLACE."""
    import torch
    assert torch.cuda.is_available()
    c = random_case(seed)
    o = oracle_of(seed)
    stage = {}
    for blending in ("over", "replace"):
        r = R.Renderer(configuration(c, blending), device=0)
        scene = R.Scene(r, c["batch"])
        assert scene.status() == o.status()
        stage[blending] = dict(renderer=r, scene=scene, frames={})
    if o.status() != 0:
        pytest.skip(SKIP_REASON)

    def frame_of(blending, fmt):
        frames = stage[blending]["frames"]
        if fmt not in frames:
            frames[fmt] = R.Frame(stage[blending]["renderer"], c["width"], c["height"], fmt)
        return frames[fmt]

    def check(frame, variant, fmt, what, general):
        expect, expect_depth = expectation(seed, variant, fmt)
        image = frame.download()
        where = f"seed {seed} variant {variant['name']} format {FORMAT_NAMES[fmt]} {what}"
        assert np.array_equal(image, expect), f"{where}: {differing(image, expect)}"
        if c["depth"] is not None:
            assert np.array_equal(frame.download_depth(), expect_depth), f"{where}: the depth attachment differs"
        tap = last_pass(frame)
        if general:
            assert tap["general"] == 1 and tap["raster"] == "ops", f"{where}: {tap}"

    for variant in PM.variants_of(seed):
        r, scene = stage[variant["blending"]]["renderer"], stage[variant["blending"]]["scene"]
        images = install(r, scene, variant)
        for fmt in variant["formats"]:
            frame = frame_of(variant["blending"], fmt)
            for round_ in range(2):
                draw(frame, scene, c, variant["colors"])
                check(frame, variant, fmt, f"pass {round_}", True)
        for image in images:
            image.destroy()
        # a table leaves nothing behind: cleared, the plain solid pass of this renderer is the oracle's again
        scene.set_paints([], [])
        frame = frame_of(variant["blending"], R.FORMAT_RGBA8)
        draw(frame, scene, c, variant["case"]["colors"])
        check(frame, dict(variant, name=variant["name"] + " (then no table)"), R.FORMAT_RGBA8, "solid pass", variant["blending"] == "replace")


# ---------------------------------------------------------------- b. one carried pass state, a different kernel per piece

@pytest.mark.parametrize("seed", _seeds("CRH_FUZZ_PAINTED_SPLIT_SEEDS", "24"))
def test_a_pass_that_keeps_its_state_goes_on_in_another_kernel(seed, oracle_lib):
    """The recorded pass of random_case(seed) cut into two to five pieces at random draws with frame.keep_pass_state(), as
    test_a_random_pass_cut_into_pieces_at_random_draws_gives_the_same_frame cuts it; in front of each piece the Scene's table becomes the next
    of a random permutation of {none, gradient, conic, image, mip}, so that consecutive pieces run k_raster_tile<OPS>, k_raster_paint,
    k_raster_image and k_raster_mip over one carried state (state_stencil, state_alpha, state_color) — mid-clip, mid-opacity-group, between a
    Stencil and its Color. The frame is the single pass's oracle image, byte for byte, in two rounds with a clear between them. The images of a
    piece's table are destroyed before the next piece is submitted: the table keeps the pixels."""
    import torch
    assert torch.cuda.is_available()
    c = random_case(seed)
    o = oracle_of(seed)
    if o.status() != 0:
        pytest.skip(SKIP_REASON)
    rng = np.random.RandomState(7600 + seed)
    r = R.Renderer(configuration(c, "over"), device=0)
    scene = R.Scene(r, c["batch"])
    assert scene.status() == 0
    expect, expect_depth = oracle_images(seed, False, False)
    variants = {v["name"]: v for v in PM.variants_of(seed)}
    plain = dict(name="none", table=[], images=[], assoc=[], colors=c["colors"])
    draws = c["draws"]
    pieces = min(len(draws), int(rng.randint(2, 6)))
    cuts = sorted(rng.choice(np.arange(1, len(draws)), size=pieces - 1, replace=False).tolist())
    bounds = [0] + cuts + [len(draws)]
    frame = R.Frame(r, c["width"], c["height"])
    for round_ in range(2):
        order = [("none", "gradient", "conic", "image", "mip")[k] for k in rng.permutation(5)][:pieces]
        frame.clear()
        if c["depth"] is not None:
            frame.upload_depth(c["depth"])
        frame.keep_pass_state()
        for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            v = plain if order[k] == "none" else variants[order[k]]
            images = install(r, scene, v)
            for image in images[::2]:  # some before the piece is submitted, the rest behind it and before the next
                image.destroy()
            scene.render_draws(frame, c["transforms"], v["colors"], draws[a:b])
            for image in images[1::2]:
                image.destroy()
        image = frame.download()
        where = f"seed {seed} cuts {cuts} tables {order} round {round_}"
        assert np.array_equal(image, expect), f"{where}: {differing(image, expect)}"
        if c["depth"] is not None:
            assert np.array_equal(frame.download_depth(), expect_depth), f"{where}: the depth attachment differs"
        scene.set_paints([], [])


# ---------------------------------------------------------------- c. sample counts the oracle does not draw

@pytest.mark.parametrize("seed", PM.CONSISTENCY_SEEDS)
def test_sample_counts_2_and_8_agree_with_the_solid_general_pass(seed, oracle_lib, no_pins):
    """A consistency check, not ground truth: the oracle draws 1 and 4 samples only. At msaa_sample_count 2 and 8, on the plain and clip kinds,
    every variant's frame equals the frame the same Renderer draws from the same draws with no table (for the replace variants: the frame of
    the "over" Renderer with the opaque colours), byte for byte, in RGBA8 and BGRA8."""
    c = random_case(seed)
    assert PM.kind_of(seed) in (0, 3) and oracle_of(seed).status() == 0
    variants = PM.variants_of(seed)
    opaque = next(v for v in variants if v["name"] == "replace")["case"]["colors"]
    for msaa in (2, 8):
        stage = {}
        for blending in ("over", "replace"):
            r = R.Renderer(configuration(c, blending, msaa), device=0)
            scene = R.Scene(r, c["batch"])
            assert scene.status() == 0
            stage[blending] = (r, scene, {fmt: R.Frame(r, c["width"], c["height"], fmt) for fmt in (R.FORMAT_RGBA8, R.FORMAT_BGRA8)})
        reference = {}
        for fmt, frame in stage["over"][2].items():
            for what, colours in (("over", c["colors"]), ("replace", opaque)):
                draw(frame, stage["over"][1], c, colours)
                reference[(what, fmt)] = frame.download()
        for what in ("over", "replace"):
            assert np.array_equal(reference[(what, R.FORMAT_BGRA8)], reference[(what, R.FORMAT_RGBA8)][..., PM.SWAP])
        for variant in variants:
            r, scene, frames = stage[variant["blending"]]
            images = install(r, scene, variant)
            for fmt, frame in frames.items():
                draw(frame, scene, c, variant["colors"])
                image, expect = frame.download(), reference[(variant["blending"], fmt)]
                tap = last_pass(frame)
                assert tap["general"] == 1 and tap["raster"] == "ops", tap
                assert np.array_equal(image, expect), f"seed {seed} msaa {msaa} variant {variant['name']} format {FORMAT_NAMES[fmt]}: {differing(image, expect)}"
            for image in images:
                image.destroy()
            scene.set_paints([], [])
