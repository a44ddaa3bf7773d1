"""crh_image_lighting (include/contrast_hip.h) on the GPU: k_image_lighting byte for byte against the numpy model of tests/lighting_model.py —
random alpha fields and one smooth field (a blurred disc, so that gradients of every size occur), sizes inside one tile, sizes that cross
tile borders, the widest index range — with the source untouched, the bevel chain on the device step by step, and the refused calls."""
import ctypes as C

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, CompositeOp, ContrastError, DistantLight, LightingOp, PointLight, SpotLight, _ffi, batch_from_shapes, lighting_texels
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image

import blur_model
import composite_model as CM
import lighting_model as M
from lighting_model import Light
from test_gpu_blending import no_pins, stack  # noqa: F401

pytestmark = pytest.mark.gpu

# k_image_lighting's tile is 64 x 16 texels (LightingTile in csrc/image_filter.hip, Tile::W x Tile::H of csrc/image_geometry.hpp) and its halo one texel on every side.
# (1, 1), (1, 7), (7, 1) and (3, 2) lie inside one tile, the first three narrower than the stencil, so the staged texels are wrapped ones;
# (64, 16) fills one tile exactly. (65, 300) crosses the first tile border in x by one texel (the halo alone) and the 18th in y by 12;
# (300, 17) crosses the fourth in x by 44 and the first in y by one; (129, 33) crosses the second border of both axes by one.
SMALL = [(1, 1), (1, 7), (7, 1), (3, 2), (64, 16)]
LARGE = [(65, 300), (300, 17), (129, 33)]
EDGES = [BlurEdge.Transparent, BlurEdge.Pad, BlurEdge.Repeat, BlurEdge.Reflect]
OPERANDS = {M.DIFFUSE: (3.0, 0.9, 1.0, (1.0, 0.5, 0.25)), M.SPECULAR: (-2.0, 1.5, 12.0, (0.3, 1.0, 0.7))}  # op -> surface_scale, constant, specular_exponent, colour


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


_made = {}


def made_once(key, make):
    if key not in _made:
        _made[key] = make()
        if isinstance(_made[key], np.ndarray):
            _made[key].setflags(write=False)
    return _made[key]


def pixels_of(w, h):
    """Random texels of a size, made once and never written."""
    return made_once((w, h), lambda: M.random_pixels(np.random.RandomState(w + 3 * h), w, h))


def smooth_of(w, h):
    """A white disc under a Gaussian blur (the blur's own model): flat inside and outside, every slope between."""
    def make():
        jj, ii = np.mgrid[0:h, 0:w]
        disc = np.hypot((ii + 0.5 - w / 2.0) / (0.35 * w), (jj + 0.5 - h / 2.0) / (0.35 * h)) <= 1.0
        return np.ascontiguousarray(blur_model.blur_sigma(np.repeat((disc * 255).astype(np.uint8)[..., None], 4, axis=2), 0.05 * w + 1.0, 0.05 * h + 1.0, blur_model.PAD))
    return made_once(("smooth", w, h), make)


def lights_of(w, h):
    """One light of every kind for a size: a distant one, a point light above the image, a spot whose cone cuts through the image."""
    return [Light(M.DISTANT, azimuth=225.0, elevation=35.0), Light(M.POINT, position=(0.3 * w, 0.6 * h, 4.5)),
            Light(M.SPOT, position=(-2.0, -1.0, 6.0), points_at=(0.6 * w, 0.5 * h, 0.0), spot_exponent=3.0, cone_angle=25.0)]


def mirror_light(light):
    if light.kind == M.DISTANT:
        return DistantLight(light.azimuth, light.elevation)
    if light.kind == M.POINT:
        return PointLight(*light.position)
    return SpotLight(light.position, light.points_at, light.spot_exponent, light.cone_angle)


def check(image, expect, source, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == source.origin, (what, image.width, image.height, image.origin)
    assert image.levels == 1, what
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"


def run_and_check(source, pixels, light, op, edge, what):
    s, k, se, colour = OPERANDS[op]
    expect = M.lighting(pixels, light, op, s, k, se, colour, int(edge))
    check(source.lighting(mirror_light(light), LightingOp(op), s, k, se, colour, edge), expect, source, what)
    return expect


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
@pytest.mark.parametrize("size", SMALL, ids=[f"{w}x{h}" for w, h in SMALL])
def test_the_lighting_equals_the_model(size, edge, renderer, no_pins):
    """Every op and light, on a random and on a smooth field."""
    for pixels in (pixels_of(*size), smooth_of(*size)):
        source = Image(renderer, pixels)
        for light in lights_of(*size):
            for op in M.OPS:
                run_and_check(source, pixels, light, op, edge, (size, light, op, edge.name))
        assert np.array_equal(source.download_level(0), pixels) and source.levels == 1  # the source is untouched


@pytest.mark.parametrize("size", LARGE, ids=[f"{w}x{h}" for w, h in LARGE])
def test_sizes_that_cross_tile_borders(size, renderer, no_pins):
    """Both ops on a random and on a smooth field, the lights and the edges in turn."""
    for n, pixels in enumerate((pixels_of(*size), smooth_of(*size))):
        source = Image(renderer, pixels)
        for turn in range(4):
            for op in M.OPS:
                light, edge = lights_of(*size)[(turn + op + n) % 3], EDGES[(turn + n) % 4]
                run_and_check(source, pixels, light, op, edge, (size, light, op, edge.name))
        assert np.array_equal(source.download_level(0), pixels) and source.levels == 1


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
def test_the_widest_index_range(edge, renderer, no_pins):
    """(16384, 2) and (2, 16384): 256 tiles in x, 1024 in y, the largest row and column indices, under a point light far outside the image."""
    wide = pixels_of(16384, 2)
    tall = made_once("tall", lambda: np.ascontiguousarray(pixels_of(16384, 2).transpose(1, 0, 2)))
    far = Light(M.POINT, position=(-900000.0, 1048576.0, 250000.0))
    for pixels, what in ((wide, "16384x2"), (tall, "2x16384")):
        source = Image(renderer, pixels)
        for op in M.OPS:
            run_and_check(source, pixels, far, op, edge, (what, "far", op, edge.name))
        h, w = pixels.shape[:2]
        near = Light(M.SPOT, position=(w - 1.0, h - 1.0, 9.0), points_at=(w - 0.5 * min(w, 80), h - 0.5 * min(h, 80), 0.0), spot_exponent=2.0, cone_angle=60.0)  # over the last tile
        run_and_check(source, pixels, near, M.SPECULAR if int(edge) % 2 else M.DIFFUSE, edge, (what, "near", edge.name))
        assert np.array_equal(source.download_level(0), pixels) and source.levels == 1


def test_flat_fields_and_the_shortcuts(renderer, no_pins):
    """A field that is flat nearly everywhere (whole waves take the distant light's constant texel) with single raised texels, at a tile
    border among them; the shortcuts and the default arguments."""
    pixels = np.zeros((40, 200, 4), dtype=np.uint8)
    pixels[..., 3] = 90
    for j, i in ((0, 0), (15, 63), (16, 64), (39, 199), (20, 100), (17, 128)):
        pixels[j, i, 3] = 255
    source = Image(renderer, pixels)
    for light in lights_of(200, 40):
        for op in M.OPS:
            for edge in EDGES:
                run_and_check(source, pixels, light, op, edge, ("flat", light, op, edge.name))
    sun = DistantLight(300.0, 20.0)
    check(source.lighting(sun), M.lighting(pixels, Light(M.DISTANT, azimuth=300.0, elevation=20.0)), source, "defaults")
    check(source.diffuse_lighting(sun, 2.0, 0.5, (1.0, 0.0, 0.5), BlurEdge.Repeat), M.lighting(pixels, Light(M.DISTANT, azimuth=300.0, elevation=20.0), M.DIFFUSE, 2.0, 0.5, 1.0, (1.0, 0.0, 0.5), M.REPEAT),
          source, "diffuse_lighting")
    check(source.specular_lighting(PointLight(50.0, 20.0, 10.0), 2.0, 1.5, 40.0), M.lighting(pixels, Light(M.POINT, position=(50.0, 20.0, 10.0)), M.SPECULAR, 2.0, 1.5, 40.0), source,
          "specular_lighting")
    assert np.array_equal(source.specular_lighting(PointLight(50.0, 20.0, 10.0), 2.0, 1.5, 40.0).download_level(0),
                          lighting_texels(pixels, PointLight(50.0, 20.0, 10.0), LightingOp.Specular, 2.0, 1.5, 40.0))  # the host function runs the same rule


def test_the_bevel_chain_on_the_device(no_pins):
    """A drawn frame -> Image.from_frame -> blur -> specular_lighting -> composite(SRC_IN) with the layer -> composite(PLUS) onto the layer ->
    Frame.load_image -> download: every step against its model, fed the previous model's bytes."""
    r = R.Renderer(R.Configuration(), device=0)
    size = 96
    shapes, transforms, colours, _ = stack(seed=3, size=size, n=6, radius=(10, 30), alpha=(0.5, 1.0))
    scene = R.Scene(r, batch_from_shapes(shapes))
    frame = R.Frame(r, size, size)
    frame.clear()
    scene.render(frame, transforms, colours)
    drawn = frame.download()
    assert 0.1 < (drawn[..., 3] > 0).mean() < 0.95
    layer = Image.from_frame(frame)
    check(layer, drawn, layer, "the snapshot")
    bump = layer.blur(2.0, edge=BlurEdge.Pad)
    bump_model = blur_model.blur_sigma(drawn, 2.0, 2.0, blur_model.PAD)
    check(bump, bump_model, layer, "the bump map")
    lamp = Light(M.POINT, position=(20.0, 10.0, 40.0))
    shine = bump.specular_lighting(PointLight(20.0, 10.0, 40.0), 6.0, 1.2, 18.0, (1.0, 0.95, 0.8))
    shine_model = M.lighting(bump_model, lamp, M.SPECULAR, 6.0, 1.2, 18.0, (1.0, 0.95, 0.8), M.PAD)
    check(shine, shine_model, bump, "the highlights")
    assert (shine_model[..., 3] > 0).any()
    masked = layer.composite(shine, CompositeOp.SrcIn)
    masked_model = CM.composite(drawn, shine_model, CM.SRC_IN, CM.NORMAL, 255, 0, 0)
    check(masked, masked_model, layer, "the highlights inside the shape")
    lit = layer.composite(masked, CompositeOp.Plus)
    lit_model = CM.composite(drawn, masked_model, CM.PLUS, CM.NORMAL, 255, 0, 0)
    check(lit, lit_model, layer, "the lit layer")
    assert not np.array_equal(lit_model, drawn)
    frame.load_image(lit)
    assert np.array_equal(frame.download(), lit_model)
    assert np.array_equal(layer.download_level(0), drawn) and np.array_equal(bump.download_level(0), bump_model)  # no source was modified


def test_the_lighting_refuses_what_it_cannot_do(renderer, no_pins):
    lib = _ffi.load_library()
    pixels = pixels_of(7, 1)
    source = Image(renderer, pixels)
    out = C.c_void_p(0x1234)

    def how_of(**changes):
        how = _ffi.LightingC()
        how.op, how.light, how.edge, how.surface_scale, how.constant, how.specular_exponent = 1, 2, 1, 1.0, 1.0, 2.0
        how.color, how.position, how.points_at = (C.c_float * 3)(1.0, 1.0, 1.0), (C.c_float * 3)(1.0, 1.0, 3.0), (C.c_float * 3)(2.0, 1.0, 0.0)
        how.spot_exponent, how.cone_angle = 1.0, 30.0
        for name, value in changes.items():
            setattr(how, name, (C.c_float * 3)(*value) if isinstance(value, tuple) else value)
        return how

    good = how_of()
    assert lib.crh_image_lighting(None, C.byref(good), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_lighting(source.handle, None, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_lighting(source.handle, C.byref(good), None) == _ffi.ERR_INVALID_ARGUMENT
    for how, text in ((how_of(op=2), "op is above CRH_LIGHTING_SPECULAR"), (how_of(light=3), "light is above CRH_LIGHT_SPOT"), (how_of(edge=4), "edge is above CRH_BLUR_EDGE_REFLECT"),
                      (how_of(surface_scale=300.0), "surface_scale is outside [-256, 256]"), (how_of(constant=-1.0), "constant is outside [0, 256]"),
                      (how_of(specular_exponent=0.5), "specular_exponent is outside [1, 128]"), (how_of(color=(1.0, 2.0, 0.0)), "a colour is outside [0, 1]"),
                      (how_of(light=0, azimuth=4000.0), "azimuth or elevation is outside [-3600, 3600]"), (how_of(position=(0.0, 0.0, 2e6)), "a position is outside [-2^20, 2^20]"),
                      (how_of(points_at=(1.0, 1.0, 3.0)), "points_at is position"), (how_of(spot_exponent=200.0), "spot_exponent is outside [0, 128]"),
                      (how_of(cone_angle=120.0), "cone_angle is neither 0 nor in (0, 90]")):
        assert lib.crh_image_lighting(source.handle, C.byref(how), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234, text
        assert lib.crh_last_error().decode() == "crh_lighting_validate: " + text
    assert lib.crh_image_lighting(source.handle, C.byref(how_of(surface_scale=float("nan"))), C.byref(out)) == _ffi.ERR_NON_FINITE and out.value == 0x1234
    assert lib.crh_image_lighting(source.handle, C.byref(how_of(position=(0.0, float("inf"), 0.0))), C.byref(out)) == _ffi.ERR_NON_FINITE and out.value == 0x1234
    with pytest.raises(ContrastError):
        source.lighting(DistantLight(), edge=4)
    with pytest.raises(ContrastError):
        source.lighting(SpotLight((1.0, 2.0, 3.0), (1.0, 2.0, 3.0)))
    with pytest.raises(ContrastError):
        source.lighting("sun")
    # the limits themselves are served
    limit = Light(M.SPOT, position=(1048576.0, -1048576.0, 0.0), points_at=(0.0, 0.0, -1048576.0), spot_exponent=128.0, cone_angle=90.0)
    check(source.lighting(mirror_light(limit), LightingOp.Specular, -256.0, 256.0, 128.0, (1.0, 1.0, 1.0), BlurEdge.Reflect),
          M.lighting(pixels, limit, M.SPECULAR, -256.0, 256.0, 128.0, (1.0, 1.0, 1.0), M.REFLECT), source, "the limits themselves")
    assert np.array_equal(source.download_level(0), pixels)
