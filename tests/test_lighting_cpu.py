"""crh_image_lighting without a GPU: the model of tests/lighting_model.py against what defines it (libm and the plain SVG formula);
crh_lighting_texels (host only, the rule of csrc/lighting.hpp that the kernel runs) and the Python mirror byte for byte against the model;
every consequence the header states; the errors with their statuses and texts; the Python / C++ / Rust mirrors; and one run of the rule as
a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, ContrastError, DistantLight, LightingOp, PointLight, SpotLight, _ffi, lighting_texels
from contrast_renderer_amd import renderer as R

import lighting_model as M
from lighting_model import Light

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_lighting_validate", "crh_lighting_texels", "crh_image_lighting")
SIZES = [(1, 1), (1, 7), (7, 1), (3, 2), (33, 17)]
SAME_SIZE = (M.PAD, M.REPEAT, M.REFLECT)
SCALES = (0.0, 1.0, -3.0, 256.0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


_made = {}


def made_once(key, make):
    if key not in _made:
        _made[key] = make()
        if isinstance(_made[key], np.ndarray):
            _made[key].setflags(write=False)
    return _made[key]


def pixels_of(w, h):
    """Random texels of a size, made once and never written."""
    return made_once((w, h), lambda: M.random_pixels(np.random.RandomState(5 * w + h), w, h))


def lights_of(w, h):
    """One light of every kind for a size: a distant one, a point light above the image, a spot whose cone cuts through the image."""
    return [Light(M.DISTANT, azimuth=225.0, elevation=35.0), Light(M.POINT, position=(0.3 * w, 0.6 * h, 4.5)),
            Light(M.SPOT, position=(-2.0, -1.0, 6.0), points_at=(0.6 * w, 0.5 * h, 0.0), spot_exponent=3.0, cone_angle=25.0)]


def how_of(lamp, op=M.DIFFUSE, surface_scale=1.0, constant=1.0, specular_exponent=1.0, color=(1.0, 1.0, 1.0), edge=M.PAD, **changes):
    how = _ffi.LightingC()
    how.op, how.light, how.edge = op, lamp.kind, edge
    how.surface_scale, how.constant, how.specular_exponent = surface_scale, constant, specular_exponent
    how.color = (C.c_float * 3)(*color)
    how.azimuth, how.elevation = lamp.azimuth, lamp.elevation
    how.position, how.points_at = (C.c_float * 3)(*lamp.position), (C.c_float * 3)(*lamp.points_at)
    how.spot_exponent, how.cone_angle = lamp.spot_exponent, lamp.cone_angle
    for name, value in changes.items():
        setattr(how, name, (C.c_float * 3)(*value) if isinstance(value, tuple) else value)
    return how


def library(lib, pixels, light, *args, **kwargs):
    h, w = pixels.shape[:2]
    how = how_of(light, *args, **kwargs)
    out = np.full((h, w, 4), 0xAB, dtype=np.uint8)
    assert lib.crh_lighting_texels(w, h, pixels.ctypes.data, C.byref(how), out.ctypes.data) == _ffi.OK, lib.crh_last_error()
    return out


def mirror_light(light):
    if light.kind == M.DISTANT:
        return DistantLight(light.azimuth, light.elevation)
    if light.kind == M.POINT:
        return PointLight(*light.position)
    return SpotLight(light.position, light.points_at, light.spot_exponent, light.cone_angle)


def same(got, expect, what):
    assert got.shape == expect.shape, (what, got.shape, expect.shape)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def test_the_model_is_the_definition():
    """The transcriptions of crh_d_sincos and crh_d_pow, rounded to f32, within 1 ulp(f32) of libm (the bound crh_fmath.h states for itself),
    and the whole model within 0.5 + 1e-6 code of the plain SVG formula on random inputs."""
    rng = np.random.RandomState(11)
    for a in list(rng.uniform(-70.0, 70.0, 400)) + [0.0, M.rad(90.0), M.rad(-90.0), M.rad(3600.0), M.rad(-3600.0), M.rad(180.0), M.rad(45.0)]:
        s, c = M.d_sincos(float(a))
        assert abs(float(np.float32(s)) - math.sin(a)) <= ulp32(math.sin(a)) and abs(float(np.float32(c)) - math.cos(a)) <= ulp32(math.cos(a)), a
    bases = np.concatenate([rng.uniform(0.0, 1.0, 3000), 10.0 ** rng.uniform(-300.0, 0.0, 1000), [0.0, 1.0, 0.5, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, 2.2250738585072014e-308]])
    for e in (0.0, 1.0, 2.0, 0.5, 17.3, 128.0, float(np.float32(1.1))):
        got = M.d_pow(bases, e)
        for b, g in zip(bases, got):
            want = math.pow(b, e)
            assert abs(float(np.float32(g)) - float(np.float32(want))) <= ulp32(want) or (want < 1e-45 and float(np.float32(g)) <= 1.5e-45), (b, e, g, want)
    assert np.array_equal(M.d_exp(np.array([0.0])), [1.0]) and M.d_pow(np.array([0.25]), 0.5)[0] == pytest.approx(0.5, rel=1e-15)
    worst = 0.0
    for w, h in ((33, 17), (7, 4)):
        for trial in range(6):
            pixels = M.random_pixels(rng, w, h) if trial % 2 else M.smooth_pixels(w, h)
            lights = [Light(M.DISTANT, azimuth=rng.uniform(-360, 360), elevation=rng.uniform(-20, 90)),
                      Light(M.POINT, position=(rng.uniform(-5, w + 5), rng.uniform(-5, h + 5), rng.uniform(-2, 20))),
                      Light(M.SPOT, position=(rng.uniform(-5, w + 5), rng.uniform(-5, h + 5), rng.uniform(1, 20)), points_at=(rng.uniform(0, w), rng.uniform(0, h), 0.0),
                            spot_exponent=rng.uniform(0, 8), cone_angle=(0.0, 30.0, 60.0)[trial % 3])]
            for light in lights:
                for op in M.OPS:
                    for edge in M.EDGES:
                        args = dict(op=op, surface_scale=rng.uniform(-8, 8), constant=rng.uniform(0, 2), specular_exponent=rng.uniform(1, 40), color=tuple(rng.uniform(0, 1, 3)), edge=edge)
                        worst = max(worst, float(np.abs(M.lighting(pixels, light, **args).astype(np.float64) - M.svg(pixels, light, **args)).max()))
    assert worst <= 0.5 + 1e-6, worst


def operands():
    """(op, surface_scale, constant, specular_exponent, colour): every scale with both ops, the exponents at both ends"""
    out = []
    for n, s in enumerate(SCALES):
        out.append((M.DIFFUSE, s, (1.0, 0.7, 2.5, 0.3)[n], 1.0, (1.0, 0.5, 0.25)))
        out.append((M.SPECULAR, s, (1.0, 1.5, 0.8, 4.0)[n], (1.0, 128.0, 20.0, 7.5)[n], (0.2, 1.0, 0.6)))
    return out


@pytest.mark.parametrize("edge", M.EDGES, ids=[BlurEdge(e).name for e in M.EDGES])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_library_and_the_python_mirror_equal_the_model(lib, size, edge):
    pixels = pixels_of(*size)
    for light in lights_of(*size):
        for op, s, k, se, colour in operands():
            expect = M.lighting(pixels, light, op, s, k, se, colour, edge)
            same(library(lib, pixels, light, op, s, k, se, colour, edge), expect, (size, light, op, s, edge))
            same(lighting_texels(pixels, mirror_light(light), LightingOp(op), s, k, se, colour, BlurEdge(edge)), expect, ("mirror", size, light, op, s, edge))


def test_spot_exponents_cones_and_lights_in_and_below_the_surface(lib):
    w, h = 33, 17
    pixels = pixels_of(w, h)
    smooth = made_once("smooth", lambda: M.smooth_pixels(w, h))
    spots = [Light(M.SPOT, position=(10.0, 5.0, 8.0), points_at=(20.0, 9.0, 0.0), spot_exponent=e, cone_angle=cone) for e in (0.0, 128.0) for cone in (0.0, 20.0, 90.0)]
    spots.append(Light(M.SPOT, position=(16.5, 8.5, 3.0), points_at=(16.5, 8.5, 10.0), spot_exponent=1.0))  # it shines away from the surface: m <= 0 everywhere
    for source in (pixels, smooth):
        for light in spots:
            expect = M.lighting(source, light, M.DIFFUSE, 2.0, 1.0, 1.0, (1.0, 1.0, 1.0), M.PAD)
            if light.cone_angle == 20.0:  # the cone cuts through the image
                assert (expect[..., :3] == 0).all(axis=2).any() and (expect[..., :3] != 0).any()
            for op in M.OPS:
                for edge in M.EDGES:
                    same(library(lib, source, light, op, 2.0, 1.0, 30.0, (1.0, 0.5, 0.75), edge), M.lighting(source, light, op, 2.0, 1.0, 30.0, (1.0, 0.5, 0.75), edge), (light, op, edge))
        # a light inside the surface: its position is exactly (i + 0.5, j + 0.5, s A / 255) of texel (4, 2), so len == 0 there
        inside = source.copy()
        inside[2, 4, 3] = 255
        for s in (2.0, 0.0):
            at = Light(M.POINT, position=(4.5, 2.5, s))
            assert M.f32(s) * 255.0 / 255.0 == s
            for op in M.OPS:
                same(library(lib, inside, at, op, s, 1.0, 2.0), M.lighting(inside, at, op, s, 1.0, 2.0), ("inside", s, op))
            spot = Light(M.SPOT, position=(4.5, 2.5, s), points_at=(20.0, 9.0, -1.0), spot_exponent=2.0, cone_angle=80.0)
            same(library(lib, inside, spot, M.SPECULAR, s, 1.0, 2.0), M.lighting(inside, spot, M.SPECULAR, s, 1.0, 2.0), ("inside, spot", s))
        lit = library(lib, inside, Light(M.POINT, position=(4.5, 2.5, 2.0)), M.DIFFUSE, 2.0)
        assert tuple(lit[2, 4]) == (0, 0, 0, 255)  # L = (0, 0, 0) there
        # a light below the surface, and one far outside the image at the coordinate limit
        for light in (Light(M.POINT, position=(12.0, 7.0, -5.0)), Light(M.POINT, position=(-1048576.0, 1048576.0, 1048576.0)),
                      Light(M.SPOT, position=(12.0, 7.0, -5.0), points_at=(12.0, 8.0, 0.0), spot_exponent=1.0)):
            for op in M.OPS:
                same(library(lib, source, light, op, 1.0, 1.0, 4.0), M.lighting(source, light, op, 1.0, 1.0, 4.0), (light, op))
    below = M.lighting(pixels, Light(M.POINT, position=(12.0, 7.0, -5.0)), M.DIFFUSE)
    assert (below[..., :3] == 0).mean() > 0.5  # most of the surface faces away from it


def test_flat_fields_zero_scale_and_light_from_straight_above(lib):
    rng = np.random.RandomState(3)
    kd, colour = 0.75, (1.0, 0.5, 0.2)
    code = lambda t: 255 if t >= 1.0 else int(math.floor(t * 255.0 + 0.5))  # noqa: E731
    for alpha in (0, 1, 128, 255):
        flat = np.ascontiguousarray(np.concatenate([rng.randint(0, 256, (6, 19, 3)), np.full((6, 19, 1), alpha)], axis=2).astype(np.uint8))
        for edge in SAME_SIZE:
            for elevation in (35.0, 90.0, -10.0):
                light = Light(M.DISTANT, azimuth=77.0, elevation=elevation)
                lz = M.d_sincos(M.rad(elevation))[0]
                if elevation == 90.0:
                    assert lz == 1.0
                got = library(lib, flat, light, M.DIFFUSE, 5.0, kd, 1.0, colour, edge)
                expect = [code(M.f32(kd) * max(lz, 0.0) * M.f32(c)) for c in colour] + [255]
                assert (got == np.array(expect, dtype=np.uint8)).all(), (alpha, edge, elevation, got[0, 0], expect)
            got = library(lib, flat, Light(M.DISTANT, azimuth=10.0, elevation=90.0), M.SPECULAR, 5.0, kd, 9.0, colour, edge)
            expect = [code(M.f32(kd) * M.f32(c)) for c in colour]
            assert (got == np.array(expect + [max(expect)], dtype=np.uint8)).all(), (alpha, edge, got[0, 0], expect)
            for light in lights_of(19, 6)[1:]:  # point and spot lights over a flat field: the model (the image is not constant)
                same(library(lib, flat, light, M.SPECULAR, 5.0, kd, 9.0, colour, edge), M.lighting(flat, light, M.SPECULAR, 5.0, kd, 9.0, colour, edge), (alpha, light, edge))
    pixels = pixels_of(33, 17)  # s == 0: a constant image whatever the alpha and the edge
    for edge in M.EDGES:
        for op in M.OPS:
            got = library(lib, pixels, Light(M.DISTANT, azimuth=200.0, elevation=50.0), op, 0.0, 0.9, 3.0, colour, edge)
            assert (got == got[0, 0]).all() and got[0, 0, 0] > 0, (edge, op)
            same(got, M.lighting(pixels, Light(M.DISTANT, azimuth=200.0, elevation=50.0), op, 0.0, 0.9, 3.0, colour, edge), ("s == 0", edge, op))


def test_a_zero_constant_and_the_colour_channels_of_the_source(lib):
    pixels = pixels_of(33, 17)
    other = pixels.copy()
    other[..., :3] = 255 - other[..., :3]
    for light in lights_of(33, 17):
        for edge in M.EDGES:
            assert (library(lib, pixels, light, M.DIFFUSE, 3.0, 0.0, 1.0, (1.0, 1.0, 1.0), edge) == np.array([0, 0, 0, 255], dtype=np.uint8)).all()
            assert (library(lib, pixels, light, M.SPECULAR, 3.0, 0.0, 5.0, (1.0, 1.0, 1.0), edge) == 0).all()
            for op in M.OPS:
                got = library(lib, pixels, light, op, 3.0, 1.2, 5.0, (1.0, 0.4, 0.7), edge)
                same(library(lib, other, light, op, 3.0, 1.2, 5.0, (1.0, 0.4, 0.7), edge), got, ("colour ignored", light, op, edge))
                if op == M.SPECULAR:  # a valid premultiplied texel: alpha is the largest colour code
                    assert (got[..., 3] == got[..., :3].max(axis=2)).all()
                else:
                    assert (got[..., 3] == 255).all()


def test_a_mirrored_point_light_gives_the_mirrored_bytes(lib):
    for w, h in ((33, 17), (7, 1), (64, 5)):
        pixels = pixels_of(w, h)
        flipped = np.ascontiguousarray(pixels[:, ::-1])
        for px in (10.25, -3.0, w / 2.0):
            for op in M.OPS:
                for edge in M.EDGES:
                    got = library(lib, pixels, Light(M.POINT, position=(px, 4.5, 6.0)), op, 4.0, 1.0, 12.0, (1.0, 0.9, 0.3), edge)
                    mirrored = library(lib, flipped, Light(M.POINT, position=(w - px, 4.5, 6.0)), op, 4.0, 1.0, 12.0, (1.0, 0.9, 0.3), edge)
                    same(mirrored, np.ascontiguousarray(got[:, ::-1]), ("mirror", w, h, px, op, edge))


def test_every_code_is_close_to_the_svg_formula(lib):
    for size in ((7, 1), (33, 17)):
        for pixels in (pixels_of(*size), made_once(("smooth", size), lambda: M.smooth_pixels(*size))):
            for light in lights_of(*size):
                for op, s, k, se, colour in operands():
                    for edge in M.EDGES:
                        got = library(lib, pixels, light, op, s, k, se, colour, edge).astype(np.float64)
                        worst = float(np.abs(got - M.svg(pixels, light, op, s, k, se, colour, edge)).max())
                        assert worst <= 0.5 + 1e-6, (size, light, op, s, edge, worst)


def test_errors_statuses_texts_and_untouched_outputs(lib):
    pixels = pixels_of(3, 2)
    out = np.full((2, 3, 4), 0xAB, dtype=np.uint8)
    image = C.c_void_p(0x1234)
    nan, inf = float("nan"), float("inf")
    distant, point = Light(M.DISTANT, azimuth=30.0, elevation=40.0), Light(M.POINT, position=(1.0, 1.0, 3.0))
    spot = Light(M.SPOT, position=(1.0, 1.0, 3.0), points_at=(2.0, 1.0, 0.0), spot_exponent=2.0, cone_angle=30.0)

    def refused(how, status, text, width=3, height=2):
        if (width, height) == (3, 2):  # (the struct itself is at fault, not the size)
            assert lib.crh_lighting_validate(C.byref(how)) == status, text
            if status == _ffi.ERR_INVALID_ARGUMENT:
                assert lib.crh_last_error().decode() == "crh_lighting_validate: " + text
            assert lib.crh_image_lighting(None, C.byref(how), C.byref(image)) == _ffi.ERR_INVALID_ARGUMENT and image.value == 0x1234
        assert lib.crh_lighting_texels(width, height, pixels.ctypes.data, C.byref(how), out.ctypes.data) == status, text
        if status == _ffi.ERR_INVALID_ARGUMENT:
            assert lib.crh_last_error().decode() == "crh_lighting_validate: " + text
        assert (out == 0xAB).all()

    cases = [(distant, dict(op=2), "op is above CRH_LIGHTING_SPECULAR"), (distant, dict(light=3), "light is above CRH_LIGHT_SPOT"), (distant, dict(edge=4), "edge is above CRH_BLUR_EDGE_REFLECT"),
             (distant, dict(op=0xFFFFFFFF), "op is above CRH_LIGHTING_SPECULAR"),
             (distant, dict(surface_scale=256.5), "surface_scale is outside [-256, 256]"), (point, dict(surface_scale=-257.0), "surface_scale is outside [-256, 256]"),
             (distant, dict(constant=-0.001), "constant is outside [0, 256]"), (spot, dict(constant=256.5), "constant is outside [0, 256]"),
             (distant, dict(op=1, specular_exponent=0.999), "specular_exponent is outside [1, 128]"), (point, dict(op=1, specular_exponent=128.5), "specular_exponent is outside [1, 128]"),
             (distant, dict(color=(1.0, 1.001, 0.0)), "a colour is outside [0, 1]"), (spot, dict(color=(-0.1, 1.0, 0.0)), "a colour is outside [0, 1]"),
             (distant, dict(azimuth=3600.5), "azimuth or elevation is outside [-3600, 3600]"), (distant, dict(elevation=-3601.0), "azimuth or elevation is outside [-3600, 3600]"),
             (point, dict(position=(1.0, 1048577.0, 0.0)), "a position is outside [-2^20, 2^20]"), (spot, dict(position=(-1048577.0, 0.0, 0.0)), "a position is outside [-2^20, 2^20]"),
             (spot, dict(points_at=(0.0, 0.0, 2097152.0)), "a points_at is outside [-2^20, 2^20]"), (spot, dict(points_at=(1.0, 1.0, 3.0)), "points_at is position"),
             (spot, dict(spot_exponent=-0.5), "spot_exponent is outside [0, 128]"), (spot, dict(spot_exponent=129.0), "spot_exponent is outside [0, 128]"),
             (spot, dict(cone_angle=-1.0), "cone_angle is neither 0 nor in (0, 90]"), (spot, dict(cone_angle=90.5), "cone_angle is neither 0 nor in (0, 90]")]
    for light, changes, text in cases:
        refused(how_of(light, **changes), _ffi.ERR_INVALID_ARGUMENT, text)
    for light, changes in ((distant, dict(surface_scale=nan)), (point, dict(constant=inf)), (spot, dict(op=1, specular_exponent=nan)), (distant, dict(color=(0.0, -inf, 0.0))),
                           (distant, dict(azimuth=nan)), (distant, dict(elevation=inf)), (point, dict(position=(0.0, 0.0, nan))), (spot, dict(position=(inf, 0.0, 0.0))),
                           (spot, dict(points_at=(0.0, nan, 0.0))), (spot, dict(spot_exponent=nan)), (spot, dict(cone_angle=inf))):
        refused(how_of(light, **changes), _ffi.ERR_NON_FINITE, "non-finite")
    # the fields that the chosen op and light do not use are not read and not validated
    for how in (how_of(distant, specular_exponent=nan, position=(nan, inf, 4e6), points_at=(nan, nan, nan), spot_exponent=-5.0, cone_angle=nan),
                how_of(point, azimuth=nan, elevation=1e9, points_at=(1.0, 1.0, 3.0), spot_exponent=inf, cone_angle=200.0, specular_exponent=0.0),
                how_of(spot, op=1, specular_exponent=1.0, azimuth=inf, elevation=nan)):
        assert lib.crh_lighting_validate(C.byref(how)) == _ffi.OK, lib.crh_last_error()
    got = np.empty_like(out)
    how = how_of(distant, specular_exponent=nan, position=(nan, inf, 4e6), points_at=(nan, nan, nan), spot_exponent=-5.0, cone_angle=nan)
    assert lib.crh_lighting_texels(3, 2, pixels.ctypes.data, C.byref(how), got.ctypes.data) == _ffi.OK
    same(got, M.lighting(pixels, distant), "unused fields")
    # sizes, null arguments and out == in
    good = how_of(distant)
    for width, height in ((0, 2), (3, 0), (16385, 2), (3, 16385)):
        refused(good, _ffi.ERR_INVALID_ARGUMENT, "width and height lie in [1, 16384]", width, height)
    assert lib.crh_lighting_validate(None) == _ffi.ERR_INVALID_ARGUMENT and lib.crh_last_error().decode() == "crh_lighting_validate: a null argument"
    assert lib.crh_lighting_texels(3, 2, None, C.byref(good), out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode() == "crh_lighting_validate: a null argument"
    assert lib.crh_lighting_texels(3, 2, pixels.ctypes.data, C.byref(good), None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_lighting_texels(3, 2, pixels.ctypes.data, None, out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert (out == 0xAB).all()
    same_buffer = pixels.copy()
    assert lib.crh_lighting_texels(3, 2, same_buffer.ctypes.data, C.byref(good), same_buffer.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT  # out_rgba8 == rgba8
    assert lib.crh_last_error().decode() == "crh_lighting_validate: out_rgba8 is rgba8" and np.array_equal(same_buffer, pixels)
    # the limits themselves
    for how in (how_of(Light(M.DISTANT, azimuth=-3600.0, elevation=3600.0), op=1, surface_scale=-256.0, constant=256.0, specular_exponent=128.0, color=(0.0, 1.0, 0.0), edge=3),
                how_of(Light(M.SPOT, position=(1048576.0, -1048576.0, 0.0), points_at=(1048576.0, -1048576.0, 1e-30), spot_exponent=128.0, cone_angle=90.0), constant=0.0),
                how_of(Light(M.SPOT, position=(0.0, 0.0, 1.0), points_at=(0.0, 0.0, 0.0), spot_exponent=0.0, cone_angle=1e-3), op=1, specular_exponent=1.0)):
        assert lib.crh_lighting_validate(C.byref(how)) == _ffi.OK, lib.crh_last_error()
    # the device entry point validates before it touches a device
    assert lib.crh_image_lighting(None, C.byref(good), C.byref(image)) == _ffi.ERR_INVALID_ARGUMENT and image.value == 0x1234
    assert lib.crh_last_error().decode() == "crh_lighting_validate: a null argument"


def test_unaligned_bytes(lib):
    pixels = pixels_of(33, 17)
    light = lights_of(33, 17)[2]
    expect = M.lighting(pixels, light, M.SPECULAR, 3.0, 1.0, 6.0, (1.0, 1.0, 0.5), M.REFLECT)
    how = how_of(light, M.SPECULAR, 3.0, 1.0, 6.0, (1.0, 1.0, 0.5), M.REFLECT)
    for shift_in, shift_out in ((1, 0), (0, 3), (3, 1)):
        raw_in, raw_out = np.zeros(pixels.size + 8, dtype=np.uint8), np.full(expect.size + 8, 0xCD, dtype=np.uint8)
        raw_in[shift_in:shift_in + pixels.size] = pixels.ravel()
        assert lib.crh_lighting_texels(33, 17, raw_in.ctypes.data + shift_in, C.byref(how), raw_out.ctypes.data + shift_out) == _ffi.OK
        assert np.array_equal(raw_out[shift_out:shift_out + expect.size].reshape(expect.shape), expect)
        assert (raw_out[:shift_out] == 0xCD).all() and (raw_out[shift_out + expect.size:] == 0xCD).all()


def test_the_python_mirror(lib):
    assert [int(v) for v in LightingOp] == [0, 1] and [int(v) for v in R.LightKind] == [0, 1, 2]
    assert callable(R.Image.lighting) and callable(R.Image.diffuse_lighting) and callable(R.Image.specular_lighting)
    pixels = pixels_of(33, 17)
    # the defaults: diffuse, surface_scale 1, constant 1, a white light, BlurEdge.Pad
    same(lighting_texels(pixels, DistantLight(45.0, 30.0)), M.lighting(pixels, Light(M.DISTANT, azimuth=45.0, elevation=30.0)), "defaults")
    same(lighting_texels(pixels, PointLight(3.0, 4.0, 5.0), LightingOp.Specular, specular_exponent=8.0), M.lighting(pixels, Light(M.POINT, position=(3.0, 4.0, 5.0)), M.SPECULAR, specular_exponent=8.0), "point")
    same(lighting_texels(pixels, SpotLight()), M.lighting(pixels, Light(M.SPOT, position=(0.0, 0.0, 1.0), points_at=(0.0, 0.0, 0.0), spot_exponent=1.0)), "spot defaults")
    for bad in (dict(light=DistantLight(), surface_scale=300.0), dict(light=DistantLight(), edge=4), dict(light=DistantLight(), op=2), dict(light=SpotLight((1, 1, 1), (1, 1, 1))),
                dict(light=PointLight(), color=(2.0, 0.0, 0.0)), dict(light="sun")):
        with pytest.raises(ContrastError) as refused:
            lighting_texels(pixels, **bad)
        assert refused.value.status == _ffi.ERR_INVALID_ARGUMENT
    with pytest.raises(ContrastError) as refused:
        lighting_texels(pixels, DistantLight(float("nan"), 0.0))
    assert refused.value.status == _ffi.ERR_NON_FINITE
    with pytest.raises(ContrastError):
        lighting_texels(pixels[..., :3], DistantLight())
    sig = lib._crh_signatures
    assert [len(sig[name][1]) for name in NAMES] == [1, 5, 3]
    fields = [name for name, _ in _ffi.LightingC._fields_]
    assert fields == ["op", "light", "edge", "surface_scale", "constant", "specular_exponent", "color", "azimuth", "elevation", "position", "points_at", "spot_exponent", "cone_angle"]
    assert C.sizeof(_ffi.LightingC) == 4 * 19


def test_the_library_exports_and_the_mirrors_agree_across_header_python_and_ffi_rs(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    exports = open(b.write_export_map()).read()
    for name in NAMES:
        assert f"    {name};\n" in exports
    assert any(os.path.basename(h) == "lighting.hpp" for h in b.header_deps())
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    assert re.search(r"CRH_LIGHTING_DIFFUSE = 0, CRH_LIGHTING_SPECULAR = 1", header) and re.search(r"CRH_LIGHT_DISTANT = 0, CRH_LIGHT_POINT = 1, CRH_LIGHT_SPOT = 2", header)
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    assert committed == fresh
    for text in ("pub fn crh_lighting_validate(how: *const crh_lighting) -> crh_status;",
                 "pub fn crh_lighting_texels(width: u32, height: u32, rgba8: *const c_void, how: *const crh_lighting, out_rgba8: *mut c_void) -> crh_status;",
                 "pub fn crh_image_lighting(src: *const crh_image, how: *const crh_lighting, out: *mut *mut crh_image) -> crh_status;",
                 "pub const CRH_LIGHTING_SPECULAR: u32 = 1;", "pub const CRH_LIGHT_SPOT: u32 = 2;",
                 "pub struct crh_lighting {\n    pub op: u32,\n    pub light: u32,\n    pub edge: u32,\n    pub surface_scale: f32,\n    pub constant: f32,\n    pub specular_exponent: f32,\n"
                 "    pub color: [f32; 3],\n    pub azimuth: f32,\n    pub elevation: f32,\n    pub position: [f32; 3],\n    pub points_at: [f32; 3],\n    pub spot_exponent: f32,\n"
                 "    pub cone_angle: f32,\n}"):
        assert text in committed, text
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub enum LightingOp {", "pub enum Light {", "pub struct Lighting {", "pub fn lighting_validate(light: &Light, lighting: &Lighting) -> Result<(), Error>",
                 "pub fn lighting_texels(width: u32, height: u32, texels: &[u8], light: &Light, lighting: &Lighting) -> Result<Vec<u8>, Error>",
                 "pub fn lighting(&self, light: &Light, lighting: &Lighting) -> Result<Image, Error>",
                 "pub fn diffuse_lighting(&self, light: &Light, surface_scale: f32, constant: f32, color: [f32; 3], edge: BlurEdge) -> Result<Image, Error>",
                 "pub fn specular_lighting(&self, light: &Light, surface_scale: f32, constant: f32, specular_exponent: f32, color: [f32; 3], edge: BlurEdge) -> Result<Image, Error>"):
        assert text in shim, text
    for name in NAMES:
        assert f"ffi::{name}(" in shim, name
    mirror = open(os.path.join(ROOT, "include", "contrast_renderer.hpp")).read()
    for text in ("enum class LightingOp : uint32_t {", "struct DistantLight {", "struct PointLight {", "struct SpotLight {", "struct Lighting {",
                 "Image lighting(const Light& light, const Lighting& lighting = Lighting()) const", "Image diffuse_lighting(const Light& light,", "Image specular_lighting(const Light& light,",
                 "inline std::vector<uint8_t> lighting_texels(uint32_t width, uint32_t height,"):
        assert text in mirror, text
    import contrast_renderer_amd
    for name in ("LightingOp", "DistantLight", "PointLight", "SpotLight", "lighting_texels"):
        assert name in contrast_renderer_amd.__all__ and hasattr(contrast_renderer_amd, name)


def test_the_cpp_mirror_of_lighting_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lighting_harness.cpp"),
               "-o", os.path.join(tmp, "lighting_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """A stand-alone program (its own main, no library, nothing loaded into python) around csrc/lighting.hpp, the rule that crh_lighting_texels
    runs: compiled as host code with the two sanitizers (the flag goes to the host compilation alone) and run once."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        binary = os.path.join(tmp, "lighting_sanitize")
        # -x c++ and -Xarch_host: plain host C++, the sanitizers on the host alone (no device pass; clang links the sanitizers' runtime statically, so the program needs nothing preloaded)
        cmd = [hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
               "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), "-I", os.path.join(ROOT, "contrast_renderer_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "lighting_sanitize.cpp"), "-o", binary]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert re.search(r"\d+ texels, 0 failures$", done.stdout.strip())
