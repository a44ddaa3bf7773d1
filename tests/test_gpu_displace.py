"""crh_image_displace (include/contrast_hip.h) on the GPU: k_image_displace byte for byte against the numpy model of
tests/displace_model.py, with no tolerance and no excluded texel — every specialisation (filter x edge) with three channel pairs, sizes
inside one tile, one tile exactly, sizes that cross tile borders with fetches far into other workgroups' tiles and many periods out, the
widest index range, texels that are not premultiplied, the source as its own map — the host function against the device, a chain of image calls step by step, the refused calls, and the mipmaps of a
result and its use as an image paint."""
import ctypes as C
import itertools

import numpy as np
import pytest

from contrast_renderer_amd import BlendMode, BlurEdge, Channel, CompositeOp, ContrastError, TurbulenceKind, _ffi, displace_texels
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Filter, Image

import blur_model
import composite_model as CM
import convolve_model as CVM
import displace_model as M
import turbulence_model as TM
from test_gpu_blending import no_pins  # noqa: F401
from test_gpu_blur import _blit

pytestmark = pytest.mark.gpu

# k_image_displace's tile is 64 x 16 texels (DisplaceTile in csrc/image_filter.hip, Tile::W x Tile::H of csrc/image_geometry.hpp): a lane per column, four rows per
# lane, four waves. (1, 1), (1, 7), (7, 1) and (33, 15) lie inside one tile; (64, 16) fills one exactly; (65, 16) crosses the first tile
# border in x by one texel and (64, 17) the first in y by one: a wave's 64 columns and the rows-per-lane blocking. (129, 33) crosses the
# second border of both axes by one; (300, 17) crosses the fourth in x by 44 and the first in y by one.
SMALL = [(1, 1), (1, 7), (7, 1), (33, 15), (64, 16), (65, 16), (64, 17)]
LARGE = [(129, 33), (300, 17)]
FILTERS = (M.NEAREST, M.LINEAR)
PAIRS = ((M.R, M.G), (M.A, M.A), (M.B, M.R))
SCALES = ((0.0, 0.0), (0.0, 37.5), (-20.0, 20.0), (510.0, 510.0), (1024.0, -1024.0))


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


def images(w, h, seed, partly=False):
    """(source, map), both premultiplied; `partly` makes three texels in ten of the map transparent"""
    rng = np.random.default_rng(seed)
    src, map = (rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(2))
    src[..., :3], map[..., :3] = np.minimum(src[..., :3], src[..., 3:]), np.minimum(map[..., :3], map[..., 3:])
    if partly:
        map[rng.random((h, w)) < 0.3] = 0
    return src, map


def check(image, expect, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == (0, 0), (what, image.width, image.height, image.origin)
    assert image.levels == 1, what
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"
    return got


def run_and_check(source, map_image, src, map, scale, cx, cy, filter, edge):
    expect = M.displace(src, map, scale, cx, cy, filter, edge)
    return check(source.displace(map_image, scale, Channel(cx), Channel(cy), Filter(filter), BlurEdge(edge)), expect, (src.shape, scale, cx, cy, filter, edge))


@pytest.mark.parametrize("size", SMALL, ids=[f"{w}x{h}" for w, h in SMALL])
def test_every_specialisation_equals_the_model(size, renderer, no_pins):
    """filter x edge x channel pair x scale, on a random and on a partly transparent map."""
    for partly in (False, True):
        src, map = images(size[0], size[1], 17 + size[0], partly)
        source, map_image = Image(renderer, src), Image(renderer, map)
        for filter, edge, (cx, cy), scale in itertools.product(FILTERS, M.EDGES, PAIRS, SCALES):
            got = run_and_check(source, map_image, src, map, scale, cx, cy, filter, edge)
            if scale == (0.0, 0.0):
                assert np.array_equal(got, src)
        assert np.array_equal(source.download_level(0), src) and np.array_equal(map_image.download_level(0), map)  # no input was modified


def straight_images(w, h, seed):
    """(source, map) of convolve_model.random_pixels: about one texel in ten has a colour above its alpha"""
    rng = np.random.RandomState(seed)
    src, map = CVM.random_pixels(rng, w, h), CVM.random_pixels(rng, w, h)
    for a in (src, map):
        assert 0.05 < (a[..., :3] > a[..., 3:]).any(axis=2).mean() < 0.5
    return src, map


@pytest.mark.parametrize("size", [(33, 15), (65, 16)], ids=["33x15", "65x16"])
def test_maps_and_sources_that_are_not_premultiplied(size, renderer, no_pins):
    """A map colour above its alpha is loaded as min(c, a), as the colour filter loads it, and so gives the code 255; a source's codes are
    read as they are, with no clamp. Inside one tile, and one texel across the first tile border."""
    src, map = straight_images(size[0], size[1], 31 + size[0])
    clamped = map.copy()
    clamped[..., :3] = np.minimum(map[..., :3], map[..., 3:])
    assert all(np.array_equal(M.codes(map, c), M.codes(clamped, c)) for c in range(4)) and (M.codes(map, M.R)[(map[..., 0] > map[..., 3]) & (map[..., 3] > 0)] == 255).all()
    source, map_image = Image(renderer, src), Image(renderer, map)
    carried = False
    for filter, edge, (cx, cy), scale in itertools.product(FILTERS, M.EDGES, PAIRS, SCALES):
        got = run_and_check(source, map_image, src, map, scale, cx, cy, filter, edge)
        if scale == (0.0, 0.0):
            assert np.array_equal(got, src)  # the copy keeps the colours above their alpha
        carried = carried or bool((got[..., :3] > got[..., 3:]).any())
    assert carried
    assert np.array_equal(source.download_level(0), src) and np.array_equal(map_image.download_level(0), map)  # no input was modified


@pytest.mark.parametrize("filter", FILTERS, ids=["nearest", "linear"])
def test_the_source_as_its_own_map(filter, renderer, no_pins):
    """source.displace(source, ...): one device image behind both of the kernel's pointers, which it only reads. One texel across the first
    tile border, premultiplied texels and texels that are not."""
    for src in (images(65, 16, 12, True)[0], straight_images(65, 16, 13)[0]):
        source = Image(renderer, src)
        for edge, (cx, cy), scale in itertools.product(M.EDGES, PAIRS, SCALES):
            expect = M.displace(src, src, scale, cx, cy, filter, edge)
            check(source.displace(source, scale, Channel(cx), Channel(cy), Filter(filter), BlurEdge(edge)), expect, ("self", scale, cx, cy, filter, edge))
        assert np.array_equal(source.download_level(0), src) and source.levels == 1  # the source is unchanged


@pytest.mark.parametrize("size", LARGE, ids=[f"{w}x{h}" for w, h in LARGE])
def test_fetches_across_tile_borders_and_many_periods_out(size, renderer, no_pins):
    """Scale 1024: offsets of up to 512 texels land in other workgroups' tiles, and beyond the image by more than its size."""
    src, map = images(size[0], size[1], 5, True)
    source, map_image = Image(renderer, src), Image(renderer, map)
    for turn, (filter, edge) in enumerate(itertools.product(FILTERS, M.EDGES)):
        cx, cy = PAIRS[turn % 3]
        got = run_and_check(source, map_image, src, map, (1024.0, 1024.0), cx, cy, filter, edge)
        assert (got[..., :3] <= got[..., 3:]).all()
        run_and_check(source, map_image, src, map, (-1024.0, 333.25), cy, cx, filter, edge)
        run_and_check(source, map_image, src, map, (40.0, 9.5), cx, cy, filter, edge)


@pytest.mark.parametrize("size", [(16384, 2), (2, 16384)], ids=["16384x2", "2x16384"])
def test_the_widest_index_range(size, renderer, no_pins):
    """256 tiles in x, 1024 in y; scales of +-1024 give the largest positions beside the largest indices."""
    src, map = images(size[0], size[1], 9, True)
    source, map_image = Image(renderer, src), Image(renderer, map)
    for turn, (edge, filter, sign) in enumerate(itertools.product((M.REPEAT, M.TRANSPARENT), FILTERS, (1.0, -1.0))):
        cx, cy = PAIRS[turn % 3]
        run_and_check(source, map_image, src, map, (1024.0 * sign, -1024.0 * sign), cx, cy, filter, edge)


def test_the_host_function_equals_the_device(renderer, no_pins):
    src, map = images(131, 19, 3, True)
    source, map_image = Image(renderer, src), Image(renderer, map)
    for filter, edge in itertools.product(FILTERS, M.EDGES):
        args = ((33.3, -12.0), Channel.G, Channel.A, Filter(filter), BlurEdge(edge))
        assert np.array_equal(source.displace(map_image, *args).download_level(0), displace_texels(src, map, *args)), args
    assert np.array_equal(source.displace(map_image, 20.0).download_level(0), M.displace(src, map, 20.0))  # SVG's defaults; a scalar scale


def test_a_chain_on_the_device(renderer, no_pins):
    """Image.turbulence (low frequency, four channels) -> an uploaded layer displaced by it -> blur -> composite onto a backdrop: every step
    against its model, fed the previous model's bytes."""
    w, h = 96, 80
    layer_bytes, _ = images(w, h, 21)
    layer_bytes[::8] = 0  # stripes, so that the displacement shows
    layer = Image(renderer, layer_bytes)
    noise = Image.turbulence(renderer, w, h, 0.02, 2, 4, TurbulenceKind.FractalNoise)
    noise_model = TM.turbulence(w, h, 0.02, 2, 4, TM.FRACTAL_NOISE)
    check(noise, noise_model, "the noise")
    wobbly = layer.displace(noise, 24.0, Channel.R, Channel.G)
    wobbly_model = M.displace(layer_bytes, noise_model, 24.0, M.R, M.G, M.LINEAR, M.TRANSPARENT)
    check(wobbly, wobbly_model, "the displaced layer")
    assert not np.array_equal(wobbly_model, layer_bytes) and len(np.unique(wobbly_model.reshape(-1, 4), axis=0)) > 1000
    soft = wobbly.blur(1.2, edge=BlurEdge.Pad)
    soft_model = blur_model.blur_sigma(wobbly_model, 1.2, 1.2, blur_model.PAD)
    check(soft, soft_model, "the blurred layer")
    backdrop_bytes, _ = images(w, h, 22)
    result = Image(renderer, backdrop_bytes).composite(soft, CompositeOp.SrcOver, BlendMode.Normal, 0.75)
    check(result, CM.composite(backdrop_bytes, soft_model, CM.SRC_OVER, CM.NORMAL, 191, 0, 0), "the composed result")
    assert np.array_equal(noise.download_level(0), noise_model) and np.array_equal(layer.download_level(0), layer_bytes)  # no source was modified


def test_the_refused_calls_leave_out_untouched(renderer, no_pins):
    lib = _ffi.load_library()
    INVALID, PREFIX = _ffi.ERR_INVALID_ARGUMENT, "crh_displace_validate: "
    out = C.c_void_p(0x1234)
    src, map = images(8, 8, 1)
    source, map_image, small = Image(renderer, src), Image(renderer, map), Image(renderer, map[:4])
    other = Image(R.Renderer(R.Configuration(), device=0), map)

    def how_of(**changes):
        how = _ffi.DisplaceC()
        how.scale, how.x_channel, how.y_channel, how.filter, how.edge = (C.c_float * 2)(3.0, 4.0), 0, 1, 1, 0
        for name, value in changes.items():
            setattr(how, name, (C.c_float * 2)(*value) if isinstance(value, tuple) else value)
        return how

    good = how_of()
    for arguments in ((None, map_image.handle, C.byref(good), C.byref(out)), (source.handle, None, C.byref(good), C.byref(out)), (source.handle, map_image.handle, None, C.byref(out)),
                      (source.handle, map_image.handle, C.byref(good), None)):
        assert lib.crh_image_displace(*arguments) == INVALID and out.value == 0x1234 and lib.crh_last_error().decode() == PREFIX + "a null argument"
    for how, text in ((how_of(x_channel=4), "a channel is above CRH_CHANNEL_A"), (how_of(y_channel=7), "a channel is above CRH_CHANNEL_A"),
                      (how_of(filter=0x101), "filter is neither CRH_FILTER_NEAREST nor CRH_FILTER_LINEAR"), (how_of(edge=4), "edge is above CRH_BLUR_EDGE_REFLECT"),
                      (how_of(scale=(1025.0, 0.0)), "a scale is outside [-1024, 1024]")):
        assert lib.crh_image_displace(source.handle, map_image.handle, C.byref(how), C.byref(out)) == INVALID and out.value == 0x1234, text
        assert lib.crh_last_error().decode() == PREFIX + text
    assert lib.crh_image_displace(source.handle, map_image.handle, C.byref(how_of(scale=(float("nan"), 0.0))), C.byref(out)) == _ffi.ERR_NON_FINITE and out.value == 0x1234
    assert lib.crh_image_displace(source.handle, small.handle, C.byref(good), C.byref(out)) == INVALID and out.value == 0x1234
    assert lib.crh_last_error().decode() == PREFIX + "the map is of another size"
    assert lib.crh_image_displace(source.handle, other.handle, C.byref(good), C.byref(out)) == INVALID and out.value == 0x1234
    assert lib.crh_last_error().decode() == PREFIX + "the images belong to different renderers"
    # two faults: a scale out of range is named before the map's size, the map's size before its renderer
    assert lib.crh_image_displace(source.handle, small.handle, C.byref(how_of(scale=(0.0, -2000.0))), C.byref(out)) == INVALID and lib.crh_last_error().decode() == PREFIX + "a scale is outside [-1024, 1024]"
    other_small = Image(other.renderer, map[:4])
    assert lib.crh_image_displace(source.handle, other_small.handle, C.byref(good), C.byref(out)) == INVALID and lib.crh_last_error().decode() == PREFIX + "the map is of another size"
    assert out.value == 0x1234
    for bad in (dict(scale=2000.0), dict(scale=1.0, x_channel=5), dict(scale=1.0, filter=Filter.NearestMipmap), dict(scale=1.0, edge=9)):
        with pytest.raises(ContrastError):
            source.displace(map_image, **bad)
    with pytest.raises(ContrastError):
        source.displace(small, 1.0)
    check(source.displace(map_image, 3.0), M.displace(src, map, 3.0), "a good call after the refused ones")


def test_a_result_takes_mipmaps_and_serves_as_an_image_paint(renderer, no_pins):
    """The levels below a displaced image are those of the same bytes uploaded from the host, and so is what an image paint draws of it."""
    src, map = images(37, 21, 8)
    image = Image(renderer, src).displace(Image(renderer, map), (6.0, -9.0), Channel.R, Channel.B, Filter.Linear, BlurEdge.Reflect)
    before = image.download_level(0)
    assert np.array_equal(before, M.displace(src, map, (6.0, -9.0), M.R, M.B, M.LINEAR, M.REFLECT))
    image.generate_mipmaps()
    uploaded = Image(renderer, before)
    uploaded.generate_mipmaps()
    assert image.levels == uploaded.levels == 6
    for level in range(6):
        assert np.array_equal(image.download_level(level), uploaded.download_level(level)), level
    drawn = []
    for painted in (image, uploaded):
        scene, transforms, colours = _blit(renderer, painted, (1.0, 1.0, 1.0, 1.0), (37, 21))
        frame = R.Frame(renderer, 37, 21)
        frame.clear()
        scene.render(frame, transforms, colours)
        drawn.append(frame.download())
    assert np.array_equal(drawn[0], drawn[1]) and (drawn[0][..., 3] > 0).any()
