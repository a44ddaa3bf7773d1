"""crh_image_transform (include/contrast_hip.h) on the GPU: k_image_transform byte for byte against the numpy model of
tests/transform_model.py, with no tolerance and no excluded texel — every specialisation (filter x edge x affine or projective) under
fourteen matrices, on premultiplied texels and on texels that are not, at result sizes inside one tile, one tile exactly, across tile
borders, and different from the source's; the widest index range; the host function against the device; device against device (crop,
np.rot90); a chain of image calls placed by their origins, step by step; the refused calls; the mipmaps of a result and its use as an
image paint."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from contrast_renderer_amd import BlendMode, BlurEdge, CompositeOp, ContrastError, TransformFilter, _ffi, transform_fit, transform_texels
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image

import blur_model
import composite_model as CM
import regions_model as RM
import transform_model as M
from test_gpu_blending import no_pins  # noqa: F401
from test_gpu_blur import _blit

pytestmark = pytest.mark.gpu

# k_image_transform's tile is 32 x 32 texels (TransformTile in csrc/image_filter.hip: a block tile of 8 x 8 texels per wave instruction,
# four rows of blocks per lane, four waves side by side), so a wave owns 8 columns of the tile and a lane four rows 8 apart. (1, 1),
# (7, 1), (1, 7) and (31, 15) lie inside one tile — (31, 15) over three wave borders in x and into the second block row in y; (32, 32)
# fills one tile exactly; (33, 32) crosses the first tile border in x by one texel and (32, 33) the first in y by one; (33, 15) crosses
# the first in x with rows to spare. (129, 33) crosses the fourth border in x and the first in y by one; (300, 17) crosses the ninth in
# x by 12 inside the first tile row.
SMALL = [(1, 1), (7, 1), (1, 7), (31, 15), (33, 15), (32, 32), (33, 32), (32, 33)]
LARGE = [(129, 33), (300, 17)]
# (source, result): a result smaller than its source and one larger, both across tile borders of the result
OTHER = [((90, 41), (33, 15)), ((33, 15), (90, 41))]


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


def check(image, expect, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == (0, 0), (what, image.width, image.height, image.origin)
    assert image.levels == 1, what
    got = image.download_level(0)
    text = M.first_mismatch(got, expect)
    assert text is None, f"{what}: {text}"
    return got


def run_all(renderer, source_size, result_size, seed):
    """filter x edge x matrix on a premultiplied and on a straight source -> whether visible and invisible texels both occurred"""
    (sw, sh), (w, h) = source_size, result_size
    seen = set()
    for premultiplied in (True, False):
        src = M.source(sw, sh, seed, premultiplied)
        assert premultiplied or sw * sh < 4 or (src[..., :3] > src[..., 3:]).any()
        source = Image(renderer, src)
        for name, matrix in M.matrices(sw, sh, w, h).items():
            if name == "horizon":
                seen |= set(np.unique(M.positions(matrix, w, h)[2]).tolist())
            for filter, edge in itertools.product(M.FILTERS, M.EDGES):
                got = check(source.resample(matrix, w, h, TransformFilter(filter), BlurEdge(edge)), M.transform(src, matrix, w, h, filter, edge), (name, source_size, result_size, filter, edge, premultiplied))
                if name == "identity" and source_size == result_size and (filter != M.CUBIC or premultiplied):
                    assert np.array_equal(got, src)
                if premultiplied:
                    assert (got[..., :3] <= got[..., 3:]).all(), (name, filter, edge)
        assert np.array_equal(source.download_level(0), src) and source.levels == 1  # the input was not modified
    return seen


@pytest.mark.parametrize("size", SMALL + LARGE, ids=[f"{w}x{h}" for w, h in SMALL + LARGE])
def test_every_specialisation_equals_the_model(size, renderer, no_pins):
    seen = run_all(renderer, size, size, 17 + size[0])
    assert seen == ({False} if size == (1, 1) else {True, False})  # the horizon crosses every result of more than one texel


@pytest.mark.parametrize("sizes", OTHER, ids=[f"{s[0]}x{s[1]}-to-{r[0]}x{r[1]}" for s, r in OTHER])
def test_a_result_of_another_size_than_the_source(sizes, renderer, no_pins):
    assert run_all(renderer, sizes[0], sizes[1], 23) == {True, False}


@pytest.mark.parametrize("sizes", [((16384, 2), (2, 16384)), ((2, 16384), (16384, 2))], ids=["16384x2-to-2x16384", "2x16384-to-16384x2"])
def test_the_widest_index_range(sizes, renderer, no_pins):
    """The longest source and result axes: 256 tiles in x or 1024 in y, and source indices up to 16383 on either axis. A quarter turn
    walks the long source axis along the long result axis of the OTHER shape; the identity and `far` read the result's own shape."""
    (sw, sh), (w, h) = sizes
    src = M.source(sw, sh, 9)
    source = Image(renderer, src)
    cases = [("turn_90", M.matrices(sw, sh, w, h)["turn_90"], w, h), ("identity", M.matrices(sw, sh, sw, sh)["identity"], sw, sh),
             ("half", M.matrices(sw, sh, sw, sh)["translate_half"], sw, sh), ("far", M.matrices(sw, sh, w, h)["far"], w, h),
             ("horizon", M.matrices(sw, sh, w, h)["horizon"], w, h)]
    for turn, ((name, matrix, rw, rh), filter) in enumerate(itertools.product(cases, M.FILTERS)):
        edge = M.EDGES[turn % 4]
        check(source.resample(matrix, rw, rh, TransformFilter(filter), BlurEdge(edge)), M.transform(src, matrix, rw, rh, filter, edge), (name, sizes, filter, edge))
    assert np.array_equal(source.resample(cases[0][1], w, h, TransformFilter.Cubic).download_level(0), np.rot90(src, -1))


def test_the_host_function_equals_the_device(renderer, no_pins):
    sw, sh, w, h = 131, 19, 97, 45
    src = M.source(sw, sh, 3)
    source = Image(renderer, src)
    for name in ("rotate_30", "horizon", "scale_0.4"):
        matrix = M.matrices(sw, sh, w, h)[name]
        for filter, edge in itertools.product(TransformFilter, BlurEdge):
            assert np.array_equal(source.resample(matrix, w, h, filter, edge).download_level(0), transform_texels(src, matrix, w, h, filter, edge)), (name, filter, edge)
    assert np.array_equal(source.resample((1, 0, 0.5, 0, 1, 0.25), w, h).download_level(0), M.transform(src, (1, 0, 0.5, 0, 1, 0.25, 0, 0, 1), w, h))  # the defaults; six entries


def test_device_against_device(renderer, no_pins):
    """An integer translation under TRANSPARENT is crop; a quarter turn is the uploaded np.rot90; rotate() by quarter turns fits them."""
    sw, sh = 76, 38  # (both even: a quarter turn about the middle lands on whole texels)
    src = M.source(sw, sh, 6)
    source = Image(renderer, src)
    for filter, (x, y, w, h) in itertools.product(TransformFilter, ((3, -2, 76, 38), (-70, 5, 130, 20), (10, 9, 64, 16))):
        assert np.array_equal(source.resample((1, 0, x, 0, 1, y), w, h, filter).download_level(0), source.crop(x, y, w, h).download_level(0)), (filter, x, y)
    for filter, edge, (name, k, size) in itertools.product(TransformFilter, BlurEdge, (("turn_90", -1, (sh, sw)), ("turn_180", 2, (sw, sh)), ("turn_270", 1, (sh, sw)))):
        turned = source.resample(M.matrices(sw, sh, *size)[name], size[0], size[1], filter, edge)
        assert np.array_equal(turned.download_level(0), Image(renderer, np.ascontiguousarray(np.rot90(src, k))).download_level(0)), (name, filter, edge)
    for degrees, k, (c, s) in ((90, -1, (0.0, 1.0)), (180, 2, (-1.0, 0.0)), (270, 1, (0.0, -1.0)), (-90, 1, (0.0, -1.0)), (0, 0, (1.0, 0.0)), (360, 0, (1.0, 0.0))):
        turned = source.rotate(degrees, filter=TransformFilter.Cubic)
        assert np.array_equal(turned.download_level(0), np.rot90(src, k)), degrees
        # where the image's corner (0, 0) would lie, by the model's fit of the same turn about the middle (38, 19)
        assert turned.origin == M.fit(sw, sh, (c, -s, 38.0 - c * 38.0 + s * 19.0, s, c, 19.0 - s * 38.0 - c * 19.0, 0.0, 0.0, 1.0))[2], degrees


def test_a_chain_placed_by_the_origins(renderer, no_pins):
    """trim -> transform (fit, 30 degrees about the layer's middle) -> blur (TRANSPARENT: it grows) -> composite at the place the origins
    give: every step against its model, fed the previous model's bytes."""
    w, h = 120, 90
    layer_bytes = np.zeros((h, w, 4), dtype=np.uint8)
    layer_bytes[20:55, 30:88] = M.source(58, 35, 21)
    layer_bytes[20:55, 30:88, 3] |= 1  # (nothing inside is empty: the bounds are the rectangle)
    layer_bytes[20:55, 30:88, :3] = np.minimum(layer_bytes[20:55, 30:88, :3], layer_bytes[20:55, 30:88, 3:])
    layer = Image(renderer, layer_bytes)
    trimmed = layer.trim()
    assert RM.statistics(layer_bytes)[1] == (30, 20, 88, 55) and trimmed.origin == (-30, -20)
    trimmed_model = RM.crop(layer_bytes, 30, 20, 58, 35)
    assert np.array_equal(trimmed.download_level(0), trimmed_model)
    turned = trimmed.rotate(30.0, filter=TransformFilter.Cubic)
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    forward = (c, -s, 29.0 - c * 29.0 + s * 17.5, s, c, 17.5 - s * 29.0 - c * 17.5, 0.0, 0.0, 1.0)
    matrix, size, origin = M.fit(58, 35, forward)
    assert (turned.width, turned.height) == size and turned.origin == origin and size[0] > 58 and size[1] > 35
    turned_model = M.transform(trimmed_model, matrix, size[0], size[1], M.CUBIC, M.TRANSPARENT)
    assert np.array_equal(turned.download_level(0), turned_model) and (turned_model[..., 3] > 0).sum() > 58 * 35 * 0.9
    soft = turned.blur(2.0)
    soft_model = blur_model.blur_sigma(turned_model, 2.0, 2.0, blur_model.TRANSPARENT)
    assert np.array_equal(soft.download_level(0), soft_model) and soft.origin == (6, 6)
    # the trimmed layer's texel (0, 0) lay at (30, 20) of the backdrop: target (0, 0) of the turn goes there, the blur's growth comes off
    x, y = 30 - turned.origin[0] - soft.origin[0], 20 - turned.origin[1] - soft.origin[1]
    backdrop_bytes = M.source(w, h, 22)
    result = Image(renderer, backdrop_bytes).composite(soft, CompositeOp.SrcOver, BlendMode.Normal, 1.0, (x, y))
    result_model = CM.composite(backdrop_bytes, soft_model, CM.SRC_OVER, CM.NORMAL, 255, x, y)
    assert np.array_equal(result.download_level(0), result_model)
    assert np.array_equal(layer.download_level(0), layer_bytes) and np.array_equal(trimmed.download_level(0), trimmed_model)  # no source was modified


def test_the_refused_calls_leave_out_untouched(renderer, no_pins):
    lib = _ffi.load_library()
    INVALID, PREFIX = _ffi.ERR_INVALID_ARGUMENT, "crh_transform_validate: "
    out = C.c_void_p(0x1234)
    src = M.source(8, 8, 1)
    source = Image(renderer, src)

    def how_of(matrix=(1, 0, 0, 0, 1, 0, 0, 0, 1), width=8, height=8, filter=1, edge=0):
        return _ffi.TransformC((C.c_double * 9)(*matrix), width, height, filter, edge)

    good = how_of()
    for arguments in ((None, C.byref(good), C.byref(out)), (source.handle, None, C.byref(out)), (source.handle, C.byref(good), None)):
        assert lib.crh_image_transform(*arguments) == INVALID and out.value == 0x1234 and lib.crh_last_error().decode() == PREFIX + "a null argument"
    for how, code, text in ((how_of(filter=3), INVALID, "filter is above CRH_TRANSFORM_CUBIC"), (how_of(edge=4), INVALID, "edge is above CRH_BLUR_EDGE_REFLECT"),
                            (how_of((1, 0, float("nan"), 0, 1, 0, 0, 0, 1)), _ffi.ERR_NON_FINITE, "an entry of the matrix is not finite"),
                            (how_of((1, 0, 0, 0, 1, 0, 0, 0, 1e13)), INVALID, "an entry of the matrix is above 2^40 in magnitude"),
                            (how_of(width=0), INVALID, "width and height lie in [1, 16384]"), (how_of(height=16385), INVALID, "width and height lie in [1, 16384]"),
                            (how_of((1, 0, 0, 0, 1, 0, 0, 0, float("inf")), filter=9), INVALID, "filter is above CRH_TRANSFORM_CUBIC")):
        assert lib.crh_image_transform(source.handle, C.byref(how), C.byref(out)) == code and out.value == 0x1234, text
        assert lib.crh_last_error().decode() == PREFIX + text
    for bad in (dict(matrix=(1, 0, 0, 0, 1, 0), width=0, height=4), dict(matrix=(1, 0, 0, 0, 1, 0), width=4, height=4, filter=5), dict(matrix=(1, 0, 0, 0, 1, 0), width=4, height=4, edge=9),
                dict(matrix=(1e13, 0, 0, 0, 1, 0), width=4, height=4)):
        with pytest.raises(ContrastError):
            source.resample(**bad)
    for forward in ((1, 2, 0, 2, 4, 0), (1, 0, 0, 0, 1, 0, -1, 0, 1), (5000, 0, 0, 0, 1, 0)):  # singular, a corner behind the horizon, too large
        with pytest.raises(ContrastError):
            source.transform(forward)
    check(source.resample((0, 1, 0, -1, 0, 8), 8, 8), np.rot90(src, -1), "a good call after the refused ones")
    assert transform_fit(8, 8, (0, -1, 8, 1, 0, 0))[1:] == ((8, 8), (0, 0))


def test_a_result_takes_mipmaps_and_serves_as_an_image_paint(renderer, no_pins):
    """The levels below a transformed image are those of the same bytes uploaded from the host, and so is what an image paint draws of it."""
    src = M.source(30, 17, 8)
    matrix = M.matrices(30, 17, 37, 21)["rotate_30"]
    image = Image(renderer, src).resample(matrix, 37, 21, TransformFilter.Cubic, BlurEdge.Reflect)
    before = image.download_level(0)
    assert np.array_equal(before, M.transform(src, matrix, 37, 21, M.CUBIC, M.REFLECT))
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
