"""crh_image_color_filter (include/contrast_hip.h) on the GPU: k_image_color_filter byte for byte against the integer model of
tests/color_filter_model.py — every matrix of the CPU list with and without tables, every size at which the kernel changes its access width
or crosses a segment or its grid's cap, texels that are not premultiplied — the result as an image like any other, the refusals, and the way
from a rendered layer through blur, a flood and a composite back into a frame: a coloured drop shadow that never leaves the device."""
import ctypes as C

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, ColorMatrix, CompositeOp, ContrastError, _ffi, blur_taps
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image

import blur_model as BM
import color_filter_model as FM
import composite_model as CM
import mip_model as MM
from test_gpu_blending import no_pins  # noqa: F401
from test_gpu_blur import _blit
from test_gpu_composite import shapes_on

pytestmark = pytest.mark.gpu

# k_image_color_filter has k_image_composite's geometry: a lane owns V = 4, 2 or 1 texels by the width (w % 4 == 0, w % 2 == 0, else), a
# workgroup a row segment of 256 V texels, and the grid is capped at 8192 workgroups: with s segments to a row, min(h, 8192 / s) rows are
# launched and the others strided over. (1, 1) .. (70, 300): V = 1 (1, 5, 67), V = 4 (300) and V = 2 (70), one segment each, ending inside a
# lane group. (257, 2), (514, 3), (1028, 5): one texel group beyond the first segment for V = 1, 2, 4. (1, 8194), (2, 8194), (4, 8194): one
# segment and two rows beyond the cap, for each V. (257, 4100): two segments, so 4096 rows are launched and four are strided over.
SIZES = [(1, 1), (5, 3), (67, 9), (300, 70), (70, 300), (257, 2), (514, 3), (1028, 5), (1, 8194), (2, 8194), (4, 8194), (257, 4100)]
MATRICES = FM.matrices()
FILTERS = {"matrix": (FM.hue_rotate(90), None), "matrix+tables": (FM.saturate(2), FM.random_tables(5))}


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


_pixels = {}


def pixels_of(w, h, salt=0):
    """Random premultiplied texels of a size, made once and never written."""
    key = (w, h, salt)
    if key not in _pixels:
        _pixels[key] = FM.random_image(np.random.RandomState(w + 3 * h + 1000 * salt), w, h)
        _pixels[key].setflags(write=False)
    return _pixels[key]


def check(image, expect, what, origin=(0, 0)):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == origin and image.levels == 1, (what, image.width, image.height, image.origin)
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[bad][0]}, the model {expect[bad][0]}"


@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_sizes_that_cross_a_border_of_the_kernel(size, name, renderer, no_pins):
    matrix, tables = FILTERS[name]
    pixels = pixels_of(*size)
    check(Image(renderer, pixels).color_filter(matrix, tables), FM.texels(pixels, matrix, tables), (size, name))


@pytest.mark.parametrize("width", [67, 68])  # V = 1 and V = 4
@pytest.mark.parametrize("name,matrix", MATRICES, ids=[n for n, _ in MATRICES])
def test_every_matrix_with_and_without_tables(name, matrix, width, renderer, no_pins):
    pixels = pixels_of(width, 9)
    image = Image(renderer, pixels)
    v = FM.apply_matrix(FM.unpremultiply(FM.load(pixels)), FM.coefficients(matrix))
    for tables_name, tables in FM.table_sets():
        check(image.color_filter(matrix, tables), FM.premultiply(FM.apply_tables(v, tables)), (name, tables_name, width))


def test_the_identity_is_a_copy_and_the_staged_expectation_is_the_models(renderer, no_pins):
    pixels = pixels_of(70, 300)
    image = Image(renderer, pixels)
    for matrix, tables in ((None, None), (ColorMatrix.identity(), None), (None, FM.identity_tables()), (ColorMatrix.opacity(1), FM.identity_tables())):
        check(image.color_filter(matrix, tables), pixels, ("identity", matrix is None, tables is None))
    small = pixels_of(67, 9)
    v = FM.apply_matrix(FM.unpremultiply(FM.load(small)), FM.coefficients(FM.saturate(2)))
    assert np.array_equal(FM.premultiply(FM.apply_tables(v, FM.random_tables(5))), FM.texels(small, FM.saturate(2), FM.random_tables(5)))


def test_texels_that_are_not_premultiplied_and_transparent_texels_with_colour_bytes(renderer, no_pins):
    rng = np.random.RandomState(8)
    for width in (67, 68, 70):
        pixels = rng.randint(0, 256, (9, width, 4)).astype(np.uint8)
        pixels[::2, ::3, 3] = 0  # a = 0 with the colour bytes set
        assert (pixels[..., :3] > pixels[..., 3:4]).any() and pixels[pixels[..., 3] == 0][:, :3].any()
        image = Image(renderer, pixels)
        for name, (matrix, tables) in FILTERS.items():
            check(image.color_filter(matrix, tables), FM.texels(pixels, matrix, tables), ("not premultiplied", width, name))
        copy = image.color_filter()
        check(copy, FM.load(pixels).astype(np.uint8), ("the copy is of the loaded texels", width))
        assert not copy.download_level(0)[pixels[..., 3] == 0].any()  # a = 0 goes in as (0, 0, 0, 0)
        # ... and an alpha that comes from the bias alone shows the flood's colour there, not the bytes'
        opaque = image.color_filter(ColorMatrix.flood(1, 0.5, 0, 0)[:19] + [1.0]).download_level(0)
        assert (opaque == np.array([255, 128, 0, 255], dtype=np.uint8)).all()


def test_the_source_is_untouched_and_the_result_is_an_image_like_any_other(renderer, no_pins):
    pixels = pixels_of(70, 300)
    source = Image(renderer, pixels)
    source.generate_mipmaps()
    levels = [source.download_level(l) for l in range(source.levels)]
    matrix, tables = FM.hue_rotate(90), FM.invert_tables()
    got = source.color_filter(matrix, tables)
    expect = FM.texels(pixels, matrix, tables)
    check(got, expect, "hue + invert")
    assert source.levels == len(levels) and all(np.array_equal(source.download_level(l), v) for l, v in enumerate(levels))  # only level 0 is read, nothing written
    source.destroy()
    assert np.array_equal(got.download_level(0), expect)  # the result owns its texels
    # it takes a blur, a composite, another filter and an image paint ...
    qx, _ = blur_taps(1.5)
    blurred = got.blur(1.5, edge=BlurEdge.Reflect)
    assert np.array_equal(blurred.download_level(0), BM.blur(expect, qx, qx, int(BlurEdge.Reflect)))
    other = pixels_of(40, 12, salt=1)
    composed = got.composite(Image(renderer, other), CompositeOp.SrcAtop, offset=(10, 100))
    assert np.array_equal(composed.download_level(0), CM.composite(expect, other, CM.SRC_ATOP, CM.NORMAL, 255, 10, 100))
    check(got.color_filter(ColorMatrix.luminance_to_alpha()), FM.texels(expect, FM.luminance_to_alpha()), "a filter of a filter")
    white, t, colour = _blit(renderer, got, (1.0, 1.0, 1.0, 1.0), (70, 300))
    frame = R.Frame(renderer, 70, 300)
    frame.clear()
    white.render(frame, t, colour)
    assert np.array_equal(frame.download(), expect)
    # ... and mipmaps
    got.generate_mipmaps()
    chain = MM.chain(expect)
    assert got.levels == len(chain) and all(np.array_equal(got.download_level(l), v) for l, v in enumerate(chain))
    # the origin of a grown blur is kept
    grown = Image(renderer, pixels_of(67, 9)).blur(1.0)
    assert grown.origin == (3, 3) and grown.color_filter(ColorMatrix.flood(0, 0, 0, 0.5)).origin == (3, 3)


def test_refusals_on_the_device_path(renderer, no_pins):
    lib = _ffi.load_library()
    pixels = pixels_of(5, 3)
    mine = Image(renderer, pixels)
    out = C.c_void_p(0x1234)
    good = (C.c_float * 20)(*ColorMatrix.identity())
    assert lib.crh_image_color_filter(None, good, None, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_color_filter(mine.handle, good, None, None) == _ffi.ERR_INVALID_ARGUMENT
    above = float(np.nextafter(np.float32(16.0), np.float32(17.0)))
    for at, value, status in ((7, above, _ffi.ERR_INVALID_ARGUMENT), (0, -17.0, _ffi.ERR_INVALID_ARGUMENT), (13, float("nan"), _ffi.ERR_NON_FINITE), (19, float("inf"), _ffi.ERR_NON_FINITE)):
        values = ColorMatrix.identity()
        values[at] = value
        assert lib.crh_image_color_filter(mine.handle, (C.c_float * 20)(*values), None, C.byref(out)) == status and out.value == 0x1234
        with pytest.raises(ContrastError) as refused:
            mine.color_filter(values)
        assert refused.value.status == status
    assert lib.crh_image_color_filter(mine.handle, (C.c_float * 20)(*[17.0] * 20), None, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode() == "crh_color_filter_validate: a coefficient is outside [-CRH_COLOR_MATRIX_MAX, CRH_COLOR_MATRIX_MAX]"
    with pytest.raises(ContrastError):
        mine.color_filter(tables=np.zeros(1000, dtype=np.uint8))
    exact = ColorMatrix.identity()
    exact[7], exact[19] = 16.0, -16.0  # exactly +-16 is accepted
    check(mine.color_filter(exact), FM.texels(pixels, exact), "after the refusals")
    assert np.array_equal(mine.download_level(0), pixels)


def test_a_layer_gets_a_coloured_shadow_and_comes_back_into_a_frame(no_pins):
    """snapshot -> blur (TRANSPARENT) -> color_filter(flood) -> composite under the layer with DST_OVER at the grown origin -> Frame.load_image ->
    download: the chain of the three numpy models, byte for byte."""
    w, h = 96, 64
    r = R.Renderer(R.Configuration(), device=0)
    batch, transforms, colours = shapes_on(w, h, seed=6)
    colours[0, 3] = 1.0  # (one opaque shape: where the layer hides its shadow altogether)
    scene = R.Scene(r, batch)
    first = R.Frame(r, w, h)
    first.clear()
    scene.render(first, transforms, colours)
    drawn = first.download()
    assert (drawn[..., 3] > 0).mean() > 0.1
    flood = ColorMatrix.flood(0.1, 0.2, 0.6, 0.7)
    layer = Image.from_frame(first)
    blurred = layer.blur(2.5)
    shadow = blurred.color_filter(flood)
    assert shadow.origin == blurred.origin == (8, 8) and (shadow.width, shadow.height) == (w + 16, h + 16)
    composed = layer.composite(shadow, CompositeOp.DstOver, offset=(4 - shadow.origin[0], 3 - shadow.origin[1]))  # the shadow 4 right and 3 down
    second = R.Frame(r, w, h)
    second.load_image(composed)
    got = second.download()
    q, radius = blur_taps(2.5)
    assert radius == 8
    blurred_model = BM.blur(drawn, q, q, int(BlurEdge.Transparent))
    shadow_model = FM.texels(blurred_model, FM.flood(0.1, 0.2, 0.6, 0.7))
    assert np.array_equal(shadow.download_level(0), shadow_model)
    composed_model = CM.composite(drawn, shadow_model, CM.DST_OVER, CM.NORMAL, 255, 4 - radius, 3 - radius)
    assert np.array_equal(got, composed_model)
    assert (drawn[..., 3] == 255).any() and np.array_equal(composed_model[drawn[..., 3] == 255], drawn[drawn[..., 3] == 255])  # the layer hides its shadow where it is opaque
    beside = (drawn[..., 3] == 0) & (composed_model[..., 3] > 40)
    assert beside.any()
    tint = composed_model[beside].astype(np.float64)
    # ... and beside it the shadow shows in the flood's colour: straight (0.1, 0.2, 0.6) within the roundings of two 8-bit stages
    assert np.abs(tint[:, :3] / tint[:, 3:4] - np.array([26, 51, 153]) / 255.0).max() <= 1.0 / 40.0
