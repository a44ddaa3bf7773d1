"""crh_image_composite and crh_frame_load_image (include/contrast_hip.h) on the GPU: k_image_composite byte for byte against the integer model of
tests/composite_model.py — every operator and mode, every size at which the kernel changes its access width or crosses a segment or its grid's
cap, every way a source can lie over, across or beside the backdrop — and the way from a rendered frame through blur and two composites back
into a frame."""
import ctypes as C

import numpy as np
import pytest

from contrast_renderer_amd import BlendMode, BlurEdge, CompositeOp, ContrastError, Path, _ffi, batch_from_shapes, blur_taps
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image

import blur_model as BM
import composite_model as CM
import mip_model as MM
from test_gpu_blending import no_pins  # noqa: F401
from test_ground_truth import place

pytestmark = pytest.mark.gpu

OPS, MODES = list(CompositeOp), list(BlendMode)
PAIRS = [(CompositeOp.SrcOver, BlendMode.Normal), (CompositeOp.Xor, BlendMode.HardLight)]
PAIR_IDS = ["Normal-SrcOver", "HardLight-Xor"]
# k_image_composite gives a lane V = 4, 2 or 1 texels by the backdrop's width (w % 4 == 0, w % 2 == 0, else), a workgroup a row segment of
# 256 V texels, and caps the grid at 8192 workgroups: with s segments to a row, min(h, 8192 / s) rows are launched and the others strided over.
# (1, 1) .. (70, 300): the issue's sizes — V = 1 (1, 5, 67), V = 4 (300) and V = 2 (70), one segment each.
# (257, 2), (514, 3), (1028, 5): one texel group beyond the first 256 V-texel segment for V = 1, 2, 4.
# (1, 8194), (2, 8194), (4, 8194): one segment and two rows beyond the cap of 8192, for each V. (257, 4100): two segments, so 4096 rows are
# launched and four are strided over.
SIZES = [(1, 1), (5, 3), (67, 9), (300, 70), (70, 300), (257, 2), (514, 3), (1028, 5), (1, 8194), (2, 8194), (4, 8194), (257, 4100)]
SOURCE = (40, 12)
MIN, MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


_pixels = {}


def pixels_of(w, h, salt=0):
    """Random premultiplied texels of a size, made once and never written."""
    key = (w, h, salt)
    if key not in _pixels:
        _pixels[key] = CM.random_image(np.random.RandomState(w + 3 * h + 1000 * salt), w, h)
        _pixels[key].setflags(write=False)
    return _pixels[key]


def check(image, expect, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == (0, 0) and image.levels == 1, (what, image.width, image.height, image.origin)
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}"


def run(renderer, backdrop, source, op, mode, opacity, offset, what):
    b, s = Image(renderer, backdrop), Image(renderer, source)
    got = b.composite(s, op, mode, opacity, offset)
    check(got, CM.composite(backdrop, source, int(op), int(mode), CM.opacity_code(opacity), offset[0], offset[1]), what)
    return got


@pytest.fixture(scope="module")
def overhang(renderer):
    """The 67 x 9 backdrop and the 40 x 12 source at (-3, -2) of the operator x mode table: the images and their loaded and faded codes, made once"""
    backdrop, source = pixels_of(67, 9), pixels_of(*SOURCE, salt=1)
    o = CM.opacity_code(0.6)
    s, b = CM.fade(CM.load(CM.place(source, 67, 9, -3, -2)), o), CM.load(backdrop)
    return Image(renderer, backdrop), Image(renderer, source), s, b


@pytest.mark.parametrize("mode", MODES, ids=[m.name for m in MODES])
@pytest.mark.parametrize("op", OPS, ids=[o.name for o in OPS])
def test_every_operator_and_mode(op, mode, overhang, no_pins):
    """67 is a multiple of neither 4 nor 64; the source overhangs the top and the left and ends inside the backdrop: both of its bounds are crossed"""
    backdrop, source, s, b = overhang
    got = backdrop.composite(source, op, mode, 0.6, (-3, -2))
    check(got, CM.finish(s, b, CM.blend(s, b, int(mode)), int(op)), (op.name, mode.name))


def test_the_staged_expectation_is_the_models_composite(overhang):
    _, _, s, b = overhang
    expect = CM.composite(pixels_of(67, 9), pixels_of(*SOURCE, salt=1), CM.SRC_ATOP, CM.OVERLAY, 153, -3, -2)
    assert CM.opacity_code(0.6) == 153 and np.array_equal(expect, CM.finish(s, b, CM.blend(s, b, CM.OVERLAY), CM.SRC_ATOP))


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_sizes_that_cross_a_border_of_the_kernel(size, pair, renderer, no_pins):
    backdrop = pixels_of(*size)
    # a source of the backdrop's size at (0, 0): one wide load per texel group where V > 1
    run(renderer, backdrop, pixels_of(*size, salt=2), *pair, 0.6, (0, 0), (size, "same size"))
    # the small source shifted off every alignment, ending inside the backdrop or beyond it
    run(renderer, backdrop, pixels_of(*SOURCE, salt=1), *pair, 1.0, (-3, -2), (size, "overhang"))


OFFSETS = {"origin": (0, 0), "one-right": (1, 0), "one-column-left": (-39, 0), "beside": (None, 0), "above": (0, -SOURCE[1]), "aligned-inside": (8, 3), "aligned-overhang": (-4, 1),
           "far": (MIN, MAX), "far-other-way": (MAX, MIN)}


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("width", [67, 68, 70])  # V = 1, 4, 2; the 40-texel source's rows are a multiple of both
@pytest.mark.parametrize("name", list(OFFSETS))
def test_the_offsets(name, width, pair, renderer, no_pins):
    """(1, 0) shifts the source against any vector alignment; (-39, 0) leaves one source column; (w, 0) and (0, -12) put the source wholly outside;
    (8, 3) and (-4, 1) keep a 16-byte group aligned (one wide load), the second across the source's left end; the far ones wrap in 32 bits."""
    x, y = OFFSETS[name]
    x = width if x is None else x
    got = run(renderer, pixels_of(width, 9), pixels_of(*SOURCE, salt=1), *pair, 0.6, (x, y), (name, width))
    if name in ("beside", "above", "far", "far-other-way"):  # wholly outside: a transparent source leaves the (loaded) backdrop under both operators
        assert np.array_equal(got.download_level(0), pixels_of(width, 9))


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_a_source_larger_than_the_backdrop_on_every_side(pair, renderer, no_pins):
    for width in (67, 68):
        run(renderer, pixels_of(width, 9), pixels_of(80, 20, salt=3), *pair, 0.6, (-5, -4), ("larger", width))
        run(renderer, pixels_of(width, 9), pixels_of(80, 20, salt=3), *pair, 0.6, (-8, -4), ("larger, aligned", width))


def test_texels_that_are_not_premultiplied_are_clamped_on_load(renderer, no_pins):
    rng = np.random.RandomState(8)
    backdrop, source = rng.randint(0, 256, (9, 68, 4)).astype(np.uint8), rng.randint(0, 256, (12, 40, 4)).astype(np.uint8)
    for op, mode in PAIRS + [(CompositeOp.Dst, BlendMode.Normal), (CompositeOp.Copy, BlendMode.Normal)]:
        run(renderer, backdrop, source, op, mode, 0.6, (4, -2), ("not premultiplied", op.name))


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_the_backdrop_as_its_own_source_and_the_ends_of_opacity(pair, renderer, no_pins):
    pixels = pixels_of(67, 9)
    image = Image(renderer, pixels)
    for opacity in (1.0, 0.0):
        for offset in ((0, 0), (2, 1)):
            got = image.composite(image, *pair, opacity, offset)
            check(got, CM.composite(pixels, pixels, int(pair[0]), int(pair[1]), CM.opacity_code(opacity), *offset), ("itself", opacity, offset))
            if opacity == 0.0:
                assert np.array_equal(got.download_level(0), pixels)
    other = pixels_of(*SOURCE, salt=1)
    for opacity in (1.0, 0.0, 1.0 / 255.0, 0.5):
        run(renderer, pixels, other, *pair, opacity, (3, 1), ("opacity", opacity))


def test_the_inputs_are_untouched_and_the_result_is_an_image_like_any_other(renderer, no_pins):
    backdrop_pixels, source_pixels = pixels_of(70, 300), pixels_of(*SOURCE, salt=1)
    backdrop, source = Image(renderer, backdrop_pixels), Image(renderer, source_pixels)
    source.generate_mipmaps()
    levels = [source.download_level(l) for l in range(source.levels)]
    got = backdrop.composite(source, CompositeOp.SrcAtop, BlendMode.Multiply, 0.8, (10, 100))
    check(got, CM.composite(backdrop_pixels, source_pixels, CM.SRC_ATOP, CM.MULTIPLY, CM.opacity_code(0.8), 10, 100), "multiply")
    assert np.array_equal(backdrop.download_level(0), backdrop_pixels) and backdrop.levels == 1
    assert source.levels == len(levels) and all(np.array_equal(source.download_level(l), v) for l, v in enumerate(levels))  # only level 0 is read
    bytes_of = got.download_level(0)
    got.generate_mipmaps()
    chain = MM.chain(bytes_of)
    assert got.levels == len(chain) and all(np.array_equal(got.download_level(l), v) for l, v in enumerate(chain))
    backdrop.destroy(), source.destroy()
    assert np.array_equal(got.download_level(0), bytes_of)  # the result owns its texels


def test_refusals_on_the_device_path(renderer, no_pins):
    lib = _ffi.load_library()
    other = R.Renderer(R.Configuration(), device=0)
    mine, theirs = Image(renderer, pixels_of(5, 3)), Image(other, pixels_of(5, 3))
    how = _ffi.CompositeC(int(CompositeOp.SrcOver), int(BlendMode.Normal), 1.0, 0, 0)
    out = C.c_void_p(0x1234)
    assert lib.crh_image_composite(mine.handle, theirs.handle, C.byref(how), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_last_error().decode() == "crh_image_composite: the images belong to different renderers"
    with pytest.raises(ContrastError) as refused:
        theirs.composite(mine)
    assert refused.value.status == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_image_composite(mine.handle, None, C.byref(how), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_image_composite(None, mine.handle, C.byref(how), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_image_composite(mine.handle, mine.handle, None, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_image_composite(mine.handle, mine.handle, C.byref(how), None) == _ffi.ERR_INVALID_ARGUMENT
    for bad, status in ((_ffi.CompositeC(13, 0, 1.0, 0, 0), _ffi.ERR_INVALID_ARGUMENT), (_ffi.CompositeC(3, 9, 1.0, 0, 0), _ffi.ERR_INVALID_ARGUMENT),
                        (_ffi.CompositeC(3, 0, 1.5, 0, 0), _ffi.ERR_INVALID_ARGUMENT), (_ffi.CompositeC(3, 0, float("nan"), 0, 0), _ffi.ERR_NON_FINITE)):
        assert lib.crh_image_composite(mine.handle, mine.handle, C.byref(bad), C.byref(out)) == status and out.value == 0x1234
    check(mine.composite(mine), CM.composite(pixels_of(5, 3), pixels_of(5, 3), CM.SRC_OVER, CM.NORMAL, 255, 0, 0), "after the refusals")


# ---------------------------------------------------------------- crh_frame_load_image

def shapes_on(w, h, seed, n=5):
    """A few translucent discs and rectangles on a w x h frame: (scene batch, transforms, colours)"""
    rng = np.random.RandomState(seed)
    shapes, ts, colours = [], [], []
    for k in range(n):
        shapes.append(([], [Path.from_rect((0.0, 0.0), (1.0, 0.6))] if k % 2 else [Path.from_circle((0.0, 0.0), 1.0)]))
        ts.append(place(w, h, rng.uniform(10, w - 10), rng.uniform(10, h - 10), rng.uniform(6, 18), rotate=rng.uniform(0, 1)))
        colours.append([rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.3, 0.9)])
    return batch_from_shapes(shapes), np.float32(np.stack(ts)), np.float32(colours)


@pytest.mark.parametrize("msaa", [1, 4])
def test_a_frame_loads_an_image(msaa, no_pins):
    w, h = 64, 48
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa), device=0)
    pixels = pixels_of(w, h)
    image = Image(r, pixels)
    batch, transforms, colours = shapes_on(w, h, seed=2)
    scene = R.Scene(r, batch)
    loaded, uploaded = R.Frame(r, w, h), R.Frame(r, w, h)
    loaded.clear()
    scene.render(loaded, transforms, colours)  # (something to replace, and a pass whose state the load resets)
    loaded.load_image(image)
    image.destroy()  # the copy is done when load_image returns
    assert np.array_equal(loaded.download(), pixels)
    uploaded.upload(pixels)
    scene.render(loaded, transforms, colours)
    scene.render(uploaded, transforms, colours)
    over_loaded, over_uploaded = loaded.download(), uploaded.download()
    assert np.array_equal(over_loaded, over_uploaded)
    assert (over_loaded != pixels).any()  # (the pass drew something)
    # a frame that was cleared shows the image alone, and a second load replaces the first
    again = Image(r, pixels_of(w, h, salt=4))
    loaded.clear()
    loaded.load_image(again)
    assert np.array_equal(loaded.download(), pixels_of(w, h, salt=4))


def test_what_a_frame_refuses_to_load(no_pins):
    lib = _ffi.load_library()
    w, h = 64, 48
    r, other = R.Renderer(R.Configuration(), device=0), R.Renderer(R.Configuration(), device=0)
    image = Image(r, pixels_of(w, h))
    frame = R.Frame(r, w, h)
    frame.upload(pixels_of(w, h, salt=4))
    for bad in (Image(r, pixels_of(w, h - 1)), Image(r, pixels_of(w + 1, h)), Image(r, pixels_of(h, w))):
        with pytest.raises(ContrastError) as refused:
            frame.load_image(bad)
        assert refused.value.status == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode() == "crh_frame_load_image: the image's size is not the frame's"
    with pytest.raises(ContrastError) as refused:
        frame.load_image(Image(other, pixels_of(w, h)))
    assert refused.value.status == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode() == "crh_frame_load_image: the image belongs to another renderer"
    with pytest.raises(ContrastError) as refused:
        R.Frame(r, w, h, format=R.FORMAT_RGBA16F).load_image(image)
    assert refused.value.status == _ffi.ERR_INVALID_ARGUMENT
    slab = R.Frame(r, 160, 160)
    slab.set_tile_rows(0, 64)
    with pytest.raises(ContrastError) as refused:
        slab.load_image(Image(r, pixels_of(160, 160)))
    assert refused.value.status == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_frame_load_image(frame.handle, None) == _ffi.ERR_INVALID_ARGUMENT and lib.crh_frame_load_image(None, image.handle) == _ffi.ERR_INVALID_ARGUMENT
    assert np.array_equal(frame.download(), pixels_of(w, h, salt=4))  # a refused load changes nothing
    frame.load_image(image)
    assert np.array_equal(frame.download(), pixels_of(w, h))


# ---------------------------------------------------------------- the chain: a layer, its shadow, and back into a frame

def test_a_layer_gets_its_shadow_and_comes_back_into_a_frame(no_pins):
    w, h = 96, 64
    r = R.Renderer(R.Configuration(), device=0)
    batch, transforms, colours = shapes_on(w, h, seed=6)
    colours[0, 3] = 1.0  # (one opaque shape: where the layer hides its shadow altogether)
    scene = R.Scene(r, batch)
    over_batch, over_transforms, over_colours = shapes_on(w, h, seed=7, n=3)
    over = R.Scene(r, over_batch)
    first = R.Frame(r, w, h)
    first.clear()
    scene.render(first, transforms, colours)                       # 1. a shape
    drawn = first.download()
    assert (drawn[..., 3] > 0).mean() > 0.1
    layer = Image.from_frame(first)                                # 2.
    blurred = layer.blur(2.5)                                      # 3.
    black = np.zeros((blurred.height, blurred.width, 4), dtype=np.uint8)
    black[..., 3] = 255
    shadow = blurred.composite(Image(r, black), CompositeOp.SrcIn)  # 4. opaque black, in the blurred layer: its alpha alone
    offset = (4 - blurred.origin[0], 3 - blurred.origin[1])
    composed = layer.composite(shadow, CompositeOp.DstOver, offset=offset)  # 5. the shadow under the layer, 4 right and 3 down
    second = R.Frame(r, w, h)
    second.load_image(composed)                                    # 6.
    scene_result = second.download()
    over.render(second, over_transforms, over_colours)
    got = second.download()
    # the same through the host: download, the Python models, upload
    (qx, rx), (qy, ry) = blur_taps(2.5), blur_taps(2.5)
    assert (rx, ry) == (8, 8) == blurred.origin
    blurred_model = BM.blur(drawn, qx, qy, int(BlurEdge.Transparent))
    assert np.array_equal(blurred.download_level(0), blurred_model)
    shadow_model = CM.composite(blurred_model, black, CM.SRC_IN, CM.NORMAL, 255, 0, 0)
    assert not shadow_model[..., :3].any() and np.array_equal(shadow_model[..., 3], blurred_model[..., 3])
    composed_model = CM.composite(drawn, shadow_model, CM.DST_OVER, CM.NORMAL, 255, 4 - rx, 3 - ry)
    assert np.array_equal(scene_result, composed_model)
    assert (drawn[..., 3] == 255).any() and np.array_equal(composed_model[drawn[..., 3] == 255], drawn[drawn[..., 3] == 255])  # the layer hides its shadow where it is opaque
    beside = (drawn[..., 3] == 0) & (composed_model[..., 3] > 0)
    assert beside.any() and not composed_model[beside][:, :3].any()  # ... and the shadow shows, black, beside it
    through_host = R.Frame(r, w, h)
    through_host.upload(composed_model)
    over.render(through_host, over_transforms, over_colours)
    assert np.array_equal(got, through_host.download())
    assert (got != composed_model).any()
