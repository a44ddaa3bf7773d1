"""crh_image_turbulence (include/contrast_hip.h) on the GPU: k_image_turbulence byte for byte against the numpy model of
tests/turbulence_model.py, with no tolerance and no excluded texel — every specialisation (kind x opaque x stitched), octaves 0, 1, 4 and
12, sizes inside one tile, one tile exactly, sizes that cross tile borders, the widest index range — the period and window consequences on
the device, the host function against the device, a chain of image calls step by step, the refused calls and the mipmaps of a result."""
import ctypes as C
import itertools

import numpy as np
import pytest

from contrast_renderer_amd import BlendMode, BlurEdge, CompositeOp, ContrastError, DistantLight, TurbulenceKind, _ffi, batch_from_shapes, turbulence_texels
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image

import blur_model
import composite_model as CM
import lighting_model as LM
import turbulence_model as M
from test_gpu_blending import no_pins, stack  # noqa: F401

pytestmark = pytest.mark.gpu

# k_image_turbulence's tile is 64 x 16 texels (TurbulenceTile in csrc/image_filter.hip, Tile::W x Tile::H of csrc/image_geometry.hpp): a lane per column, four rows per
# lane, four waves. (1, 1), (1, 7), (7, 1) and (33, 15) lie inside one tile; (64, 16) fills one exactly; (65, 16) crosses the first tile
# border in x by one texel and (64, 17) the first in y by one. (129, 33) crosses the second border of both axes by one; (300, 17) crosses
# the fourth in x by 44 and the first in y by one.
SMALL = [(1, 1), (1, 7), (7, 1), (33, 15), (64, 16), (65, 16), (64, 17)]
LARGE = [(129, 33), (300, 17)]
SPECIALISATIONS = list(itertools.product(M.KINDS, (False, True), (False, True)))  # kind, opaque, stitch
# (base_frequency, offset): as in test_turbulence_cpu.py, with a frequency just below the limit
PLACES = (((0.05, 0.08), (10.0, 20.0)), ((4.0, 0.0), (65536.0, -65536.0)), ((2.0, 3.0), (-0.5, 7.25)), ((0.013, 3.9), (-65536.0, 65536.0)), ((0.0, 0.3), (1.5, -3.75)),
          ((3.999, 1.7), (-0.25, 0.75)))


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


def check(image, expect, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == (0, 0), (what, image.width, image.height, image.origin)
    assert image.levels == 1, what
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"
    return got


def run_and_check(renderer, w, h, frequency, octaves, seed, kind, stitch, opaque, offset):
    expect = M.turbulence(w, h, frequency, octaves, seed, kind, stitch, opaque, offset)
    image = Image.turbulence(renderer, w, h, frequency, octaves, seed, TurbulenceKind(kind), stitch, opaque, offset)
    return check(image, expect, (w, h, frequency, octaves, seed, kind, stitch, opaque, offset))


@pytest.mark.parametrize("size", SMALL, ids=[f"{w}x{h}" for w, h in SMALL])
def test_every_specialisation_equals_the_model(size, renderer, no_pins):
    """kind x opaque x stitched, each with 0, 1, 4 and 12 octaves, the places in turn."""
    turn = 0
    for kind, opaque, stitch in SPECIALISATIONS:
        for octaves in (0, 1, 4, 12):
            for _ in range(2):
                frequency, offset = PLACES[turn % len(PLACES)]
                run_and_check(renderer, size[0], size[1], frequency, octaves, 7 + turn, kind, stitch, opaque, offset)
                turn += 1


@pytest.mark.parametrize("size", LARGE, ids=[f"{w}x{h}" for w, h in LARGE])
def test_sizes_that_cross_several_tile_borders(size, renderer, no_pins):
    for turn, (kind, opaque, stitch) in enumerate(SPECIALISATIONS):
        frequency, offset = PLACES[(2 * turn) % len(PLACES)]
        got = run_and_check(renderer, size[0], size[1], frequency, (12, 1, 4)[turn % 3], -turn, kind, stitch, opaque, offset)
        assert (got[..., :3] <= got[..., 3:]).all()
        run_and_check(renderer, size[0], size[1], (0.07, 0.11), 5, turn, kind, stitch, opaque, (-33.5, 12.25))


def test_the_seed_with_a_zero_gradient(renderer, no_pins):
    """Seed 346 has G[1][164] = (0, 0); at more than one cell per texel a 65 x 17 image meets every lattice value many times."""
    assert tuple(M.tables(346)[1][1, 164]) == (0.0, 0.0)
    for kind, opaque, stitch in SPECIALISATIONS:
        run_and_check(renderer, 65, 17, (1.3, 2.6), 3, 346, kind, stitch, opaque, (0.1, -0.2))


@pytest.mark.parametrize("size", [(16384, 2), (2, 16384)], ids=["16384x2", "2x16384"])
def test_the_widest_index_range(size, renderer, no_pins):
    """256 tiles in x, 1024 in y; offsets of +-65536, frequency 4 and 12 octaves give the largest lattice coordinates (every point is then a
    lattice point: a constant image); a frequency just below 4 gives the same coordinates with fractions."""
    w, h = size
    for corner, stitch in itertools.product((1.0, -1.0), (False, True)):
        offset = (65536.0 * corner, 65536.0 * corner)
        got = run_and_check(renderer, w, h, 4.0, 12, 3, M.FRACTAL_NOISE, stitch, False, offset)
        assert (got == np.array([64, 64, 64, 128], dtype=np.uint8)).all()
        got = run_and_check(renderer, w, h, (3.999, 3.7), 12, 3, M.TURBULENCE if stitch else M.FRACTAL_NOISE, stitch, corner > 0, offset)
        assert len(np.unique(got.reshape(-1, 4), axis=0)) > 1000


def test_the_period_and_the_window_on_the_device(renderer, no_pins):
    for kind, opaque in itertools.product(M.KINDS, (False, True)):
        here = Image.turbulence(renderer, 64, 32, (0.05, 0.07), 5, 7, TurbulenceKind(kind), True, opaque, (3, -5)).download_level(0)
        there = Image.turbulence(renderer, 64, 32, (0.05, 0.07), 5, 7, TurbulenceKind(kind), True, opaque, (67, 27)).download_level(0)
        assert np.array_equal(here, there) and np.array_equal(here, M.turbulence(64, 32, (0.05, 0.07), 5, 7, kind, True, opaque, (3, -5)))
        plain = [Image.turbulence(renderer, 64, 32, (0.05, 0.07), 5, 7, TurbulenceKind(kind), False, opaque, o).download_level(0) for o in ((3, -5), (67, 27))]
        assert not np.array_equal(plain[0], plain[1])
        whole = Image.turbulence(renderer, 40, 30, (0.05, 0.07), 6, 11, TurbulenceKind(kind), False, opaque, (-100.5, 64.25)).download_level(0)
        piece = Image.turbulence(renderer, 10, 7, (0.05, 0.07), 6, 11, TurbulenceKind(kind), False, opaque, (-80.5, 75.25)).download_level(0)
        assert np.array_equal(piece, whole[11:18, 20:30])
    # a texture made in pieces: four 100 x 20 images side by side and one 400 x 20 image
    whole = Image.turbulence(renderer, 400, 20, 0.03, 8, 5, TurbulenceKind.FractalNoise, offset=(-7.5, 2.0)).download_level(0)
    pieces = [Image.turbulence(renderer, 100, 20, 0.03, 8, 5, TurbulenceKind.FractalNoise, offset=(-7.5 + 100 * n, 2.0)).download_level(0) for n in range(4)]
    assert np.array_equal(np.concatenate(pieces, axis=1), whole)


def test_the_host_function_equals_the_device(renderer, no_pins):
    for turn, (kind, opaque, stitch) in enumerate(SPECIALISATIONS):
        frequency, offset = PLACES[turn % len(PLACES)]
        args = ((0.2, 0.1) if turn == 1 else frequency, 6, 1000 + turn, TurbulenceKind(kind), stitch, opaque, offset)
        assert np.array_equal(Image.turbulence(renderer, 131, 19, *args).download_level(0), turbulence_texels(131, 19, *args)), args
    assert np.array_equal(Image.turbulence(renderer, 70, 20, 0.1).download_level(0), M.turbulence(70, 20, 0.1))  # the defaults; a scalar frequency


def test_a_chain_on_the_device(no_pins):
    """Image.turbulence -> blur -> diffuse_lighting -> composite(Multiply) onto a drawn layer -> Frame.load_image -> download: every step
    against its model, fed the previous model's bytes."""
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
    noise = Image.turbulence(r, size, size, 0.08, 4, 12, TurbulenceKind.FractalNoise)
    noise_model = M.turbulence(size, size, 0.08, 4, 12, M.FRACTAL_NOISE)
    check(noise, noise_model, "the noise")
    bump = noise.blur(1.5, edge=BlurEdge.Repeat)
    bump_model = blur_model.blur_sigma(noise_model, 1.5, 1.5, blur_model.REPEAT)
    check(bump, bump_model, "the bump map")
    shade = bump.diffuse_lighting(DistantLight(225.0, 40.0), 12.0, 1.1, (1.0, 0.95, 0.9))
    shade_model = LM.lighting(bump_model, LM.Light(LM.DISTANT, azimuth=225.0, elevation=40.0), LM.DIFFUSE, 12.0, 1.1, 1.0, (1.0, 0.95, 0.9), LM.PAD)
    check(shade, shade_model, "the shading")
    assert len(np.unique(shade_model.reshape(-1, 4), axis=0)) > 20
    rough = layer.composite(shade, CompositeOp.SrcOver, BlendMode.Multiply)
    rough_model = CM.composite(drawn, shade_model, CM.SRC_OVER, CM.MULTIPLY, 255, 0, 0)
    check(rough, rough_model, "the rough layer")
    assert not np.array_equal(rough_model, drawn)
    frame.load_image(rough)
    assert np.array_equal(frame.download(), rough_model)
    assert np.array_equal(noise.download_level(0), noise_model) and np.array_equal(bump.download_level(0), bump_model)  # no source was modified


def test_the_refused_calls_leave_out_untouched(renderer, no_pins):
    lib = _ffi.load_library()
    out = C.c_void_p(0x1234)

    def how_of(**changes):
        how = _ffi.TurbulenceC()
        how.kind, how.octaves, how.seed, how.stitch, how.opaque = 1, 2, 5, 0, 0
        how.base_frequency, how.offset = (C.c_float * 2)(0.1, 0.2), (C.c_float * 2)(0.0, 0.0)
        for name, value in changes.items():
            setattr(how, name, (C.c_float * 2)(*value) if isinstance(value, tuple) else value)
        return how

    good = how_of()
    assert lib.crh_image_turbulence(None, 8, 8, C.byref(good), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_turbulence(renderer.handle, 8, 8, None, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_turbulence(renderer.handle, 8, 8, C.byref(good), None) == _ffi.ERR_INVALID_ARGUMENT
    for how, text in ((how_of(kind=2), "kind is above CRH_TURBULENCE_TURBULENCE"), (how_of(stitch=2), "stitch is neither 0 nor 1"), (how_of(opaque=7), "opaque is neither 0 nor 1"),
                      (how_of(octaves=13), "octaves is above CRH_MAX_TURBULENCE_OCTAVES"), (how_of(base_frequency=(4.5, 0.0)), "a base_frequency is outside [0, 4]"),
                      (how_of(base_frequency=(0.1, -1.0)), "a base_frequency is outside [0, 4]"), (how_of(offset=(0.0, 70000.0)), "an offset is outside [-65536, 65536]")):
        assert lib.crh_image_turbulence(renderer.handle, 8, 8, C.byref(how), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234, text
        assert lib.crh_last_error().decode() == "crh_turbulence_validate: " + text
    for w, h in ((0, 8), (8, 0), (16385, 8), (8, 16385)):
        assert lib.crh_image_turbulence(renderer.handle, w, h, C.byref(good), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
        assert lib.crh_last_error().decode() == "crh_turbulence_validate: width and height lie in [1, 16384]"
    assert lib.crh_image_turbulence(renderer.handle, 8, 8, C.byref(how_of(base_frequency=(float("nan"), 0.1))), C.byref(out)) == _ffi.ERR_NON_FINITE and out.value == 0x1234
    assert lib.crh_image_turbulence(renderer.handle, 8, 8, C.byref(how_of(offset=(0.0, float("inf")))), C.byref(out)) == _ffi.ERR_NON_FINITE and out.value == 0x1234
    for bad in (dict(base_frequency=5.0), dict(base_frequency=0.1, octaves=13), dict(base_frequency=0.1, kind=2), dict(base_frequency=0.1, offset=(1e6, 0))):
        with pytest.raises(ContrastError):
            Image.turbulence(renderer, 8, 8, **bad)
    with pytest.raises(ContrastError):
        Image.turbulence(renderer, 0, 8, 0.1)


def test_a_result_takes_mipmaps(renderer, no_pins):
    """The levels below a noise image are those of the same bytes uploaded from the host."""
    image = Image.turbulence(renderer, 37, 21, 0.1, 3, 2, TurbulenceKind.FractalNoise)
    before = image.download_level(0)
    assert np.array_equal(before, M.turbulence(37, 21, 0.1, 3, 2, M.FRACTAL_NOISE))
    image.generate_mipmaps()
    uploaded = Image(renderer, before)
    uploaded.generate_mipmaps()
    assert image.levels == uploaded.levels == 6
    for level in range(6):
        assert np.array_equal(image.download_level(level), uploaded.download_level(level)), level
