"""crh_image_morphology (include/contrast_hip.h) on the GPU: k_image_morph_h and k_image_morph_v byte for byte against the numpy model of
tests/morphology_model.py — every size that crosses a block border of either kernel, both operators, every edge, radii from 0 to 192 on inputs
that a wide window does not saturate — chains on the device, and the way from a rendered frame to an outlined layer back in a frame."""
import ctypes as C

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, ColorMatrix, CompositeOp, ContrastError, MorphologyOp, _ffi, batch_from_shapes
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image

import blur_model as BM
import color_filter_model as FM
import composite_model as CM
import mip_model
import morphology_model as MM
from test_gpu_blending import no_pins, stack  # noqa: F401

pytestmark = pytest.mark.gpu

SIZE = mip_model.SIZE
# k_image_morph_h's row segment is 256 texels and k_image_morph_v's column block 64, as blur's: (300, 70) crosses the first by 44 texels and
# the second four times, (70, 300) the second once. k_image_morph_v's row block is not blur's 32 rows but the window, 2 radius_y + 1 rows:
# 3, 7 or 11 for the radii below. (1, 7) is the smallest size that crosses it (three blocks of 3 rows, the last with one row), (5, 3) fills
# one block exactly, and (33, 17), (300, 70) and (70, 300) end inside a block for each of the three.
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17), (300, 70), (70, 300)]
RADII = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 5), (7, 3)]
OPS = [MorphologyOp.Erode, MorphologyOp.Dilate]
EDGES = [BlurEdge.Transparent, BlurEdge.Pad, BlurEdge.Repeat, BlurEdge.Reflect]
# (size, radii) of the large-radius tests
LARGE = [((900, 8), (192, 0)), ((900, 8), (192, 3)), ((900, 8), (64, 1)), ((8, 900), (0, 192)), ((8, 900), (3, 192)), ((450, 420), (100, 90))]
# Where the code takes another path. k_image_morph_h runs floor(log2(2 radius_x + 1)) doubling steps: the step count changes between 7 and 8,
# 15 and 16, 31 and 32, 63 and 64, 127 and 128. k_image_morph_v has three instantiations, for windows up to 33, up to 129 and up to 385 rows:
# radius_y 16 | 17 and 64 | 65 lie on either side of the two borders.
PATHS = [(7, 16), (8, 17), (15, 64), (16, 65), (31, 0), (32, 1), (63, 2), (64, 33), (127, 5), (128, 0)]


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


_pixels = {}


def made_once(key, make):
    if key not in _pixels:
        _pixels[key] = make()
        _pixels[key].setflags(write=False)
    return _pixels[key]


def pixels_of(w, h):
    """Random premultiplied texels of a size, made once and never written."""
    return made_once((w, h), lambda: BM.random_premultiplied(np.random.RandomState(w + 3 * h), w, h))


def check(image, expect, origin, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == origin, (what, image.width, image.height, image.origin)
    assert image.levels == 1, what
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"


def origin_of(op, edge, rx, ry):
    return (rx, ry) if MM.grows(int(op), int(edge)) else (0, 0)


def run_and_check(renderer, pixels, op, rx, ry, edge, what):
    source = Image(renderer, pixels)
    expect = MM.morphology(pixels, int(op), rx, ry, int(edge))
    h, w = pixels.shape[:2]
    assert expect.shape[:2] == MM.size(w, h, int(op), rx, ry, int(edge))[::-1]
    check(source.morphology(op, rx, ry, edge), expect, origin_of(op, edge, rx, ry), what)
    assert np.array_equal(source.download_level(0), pixels) and source.levels == 1  # the source is untouched
    return expect


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
@pytest.mark.parametrize("op", OPS, ids=[o.name for o in OPS])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_morphology_equals_the_model(size, op, edge, renderer, no_pins):
    pixels = pixels_of(*size)
    for rx, ry in RADII:
        expect = run_and_check(renderer, pixels, op, rx, ry, edge, (size, op.name, edge.name, rx, ry))
        if (rx, ry) == (0, 0):
            assert np.array_equal(expect, pixels)  # a copy


def straight_of(w, h):
    """Texels whose red lies above their alpha everywhere (alpha below 200), green and blue anywhere: not premultiplied ones."""
    def make():
        rng = np.random.RandomState(5 * w + h)
        t = rng.randint(0, 256, (h, w, 4))
        t[..., 3] = rng.randint(0, 200, (h, w))
        t[..., 0] = np.maximum(t[..., 0], t[..., 3] + 1)
        return t.astype(np.uint8)
    return made_once(("straight", w, h), make)


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
@pytest.mark.parametrize("op", OPS, ids=[o.name for o in OPS])
@pytest.mark.parametrize("size", [(1, 7), (33, 17)], ids=["1x7", "33x17"])
def test_colours_above_their_alpha_go_through_every_route(size, op, edge, renderer, no_pins):
    """The rule is per channel on the codes as they are, with no load clamp (compositing, the colour filter and convolution clamp c to a): the
    copy, the horizontal pass alone, the vertical pass alone and both, on texels whose red exceeds their alpha. Every red of a window
    exceeds its own alpha, so the window's extreme red exceeds its extreme alpha: the result keeps red > alpha everywhere — but for Erode
    under Transparent, where a window that reaches outside the source holds (0, 0, 0, 0) and gives it."""
    pixels = straight_of(*size)
    assert (pixels[..., 0] > pixels[..., 3]).all()
    for rx, ry in ((0, 0), (2, 0), (0, 1), (1, 2)):
        expect = run_and_check(renderer, pixels, op, rx, ry, edge, ("straight", size, op.name, edge.name, rx, ry))
        above = expect[..., 0] > expect[..., 3]
        if (rx, ry) == (0, 0) or not (op == MorphologyOp.Erode and edge == BlurEdge.Transparent):
            assert above.all(), (rx, ry, float(above.mean()))
        else:
            h, w = pixels.shape[:2]
            assert above[ry:h - ry, rx:w - rx].all() and not expect[:ry].any() and not expect[:, :rx].any(), (rx, ry)


def large_input(kind, size, radii):
    w, h = size
    if kind == "ramps":
        return made_once((kind, size), lambda: MM.ramps(w, h))
    make = MM.impulses if kind == "impulses" else MM.holes
    return made_once((kind, size, radii), lambda: make(w, h, radii[0], radii[1], seed=w + 7 * radii[0] + radii[1]))


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
@pytest.mark.parametrize("op", OPS, ids=[o.name for o in OPS])
@pytest.mark.parametrize("case", LARGE, ids=[f"{s[0]}x{s[1]}-{r[0]}-{r[1]}" for s, r in LARGE])
def test_large_radii_on_inputs_that_do_not_saturate(case, op, edge, renderer, no_pins):
    """Random texels saturate under a wide window (the max of 385 random codes is 255 almost everywhere and would hide an error): the ramps
    keep at least 16 distinct codes per colour channel in the result, and the sparse impulses (Dilate) or holes (Erode) give a result that is
    neither the input nor a constant."""
    size, (rx, ry) = case
    ramps = large_input("ramps", size, (rx, ry))
    expect = run_and_check(renderer, ramps, op, rx, ry, edge, ("ramps", size, op.name, edge.name, rx, ry))
    for c in range(3):
        assert len(np.unique(expect[..., c])) >= 16, (c, len(np.unique(expect[..., c])))
    sparse = large_input("impulses" if op == MorphologyOp.Dilate else "holes", size, (rx, ry))
    expect = run_and_check(renderer, sparse, op, rx, ry, edge, ("sparse", size, op.name, edge.name, rx, ry))
    assert expect.shape != sparse.shape or not np.array_equal(expect, sparse)
    assert len(np.unique(expect.reshape(-1, 4), axis=0)) > 1


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
@pytest.mark.parametrize("op", OPS, ids=[o.name for o in OPS])
def test_every_step_count_and_every_instantiation(op, edge, renderer, no_pins):
    ramps = large_input("ramps", (300, 140), None)
    for rx, ry in PATHS:
        run_and_check(renderer, ramps, op, rx, ry, edge, ("paths", op.name, edge.name, rx, ry))


@pytest.mark.parametrize("edge", [BlurEdge.Reflect, BlurEdge.Pad], ids=["Reflect", "Pad"])
@pytest.mark.parametrize("op", OPS, ids=[o.name for o in OPS])
def test_the_widest_index_range(op, edge, renderer, no_pins):
    wide = pixels_of(16384, 1)
    run_and_check(renderer, wide, op, 192, 0, edge, ("16384x1", op.name, edge.name))
    tall = made_once("tall", lambda: np.ascontiguousarray(pixels_of(16384, 1).transpose(1, 0, 2)))
    run_and_check(renderer, tall, op, 0, 192, edge, ("1x16384", op.name, edge.name))


def test_a_grown_side_above_16384_is_unsupported(renderer, no_pins):
    tall = made_once("tall", lambda: np.ascontiguousarray(pixels_of(16384, 1).transpose(1, 0, 2)))
    for pixels, blocked, free in ((pixels_of(16384, 1), (1, 0), (0, 2)), (tall, (0, 1), (2, 0))):
        source = Image(renderer, pixels)
        with pytest.raises(ContrastError) as refused:
            source.dilate(*blocked)
        assert refused.value.status == _ffi.ERR_UNSUPPORTED
        h, w = pixels.shape[:2]
        grown = source.dilate(*free)  # the other axis grows freely
        assert (grown.width, grown.height, grown.origin) == (w + 2 * free[0], h + 2 * free[1], free)
        check(grown, MM.morphology(pixels, MM.DILATE, *free, MM.TRANSPARENT), free, "the free axis")
        check(source.erode(*blocked), MM.morphology(pixels, MM.ERODE, *blocked, MM.TRANSPARENT), (0, 0), "erode keeps the size")


def saturated_pixels(kind, w, h):
    def make():
        j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        on = {"white": np.ones((h, w), dtype=bool), "clear": np.zeros((h, w), dtype=bool), "checker": (i + j) % 2 == 0}[kind]
        return np.repeat(np.where(on, 255, 0).astype(np.uint8)[:, :, None], 4, axis=2)
    return made_once((kind, w, h), make)


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
@pytest.mark.parametrize("kind", ["white", "clear", "checker"])
def test_saturated_inputs_at_the_largest_radius(kind, edge, renderer, no_pins):
    pixels = saturated_pixels(kind, 450, 420)
    for op in OPS:
        expect = run_and_check(renderer, pixels, op, 192, 192, edge, (kind, op.name, edge.name))
        if edge != BlurEdge.Transparent and kind != "checker":
            assert (expect == pixels[0, 0, 0]).all()
        if kind == "checker" and edge != BlurEdge.Transparent:
            assert (expect == (255 if op == MorphologyOp.Dilate else 0)).all()


def test_chains_on_the_device(renderer, no_pins):
    pixels = pixels_of(33, 17)
    source = Image(renderer, pixels)
    first = source.dilate(2, 1)
    second = first.dilate(3, 4)
    assert first.origin == (2, 1) and second.origin == (3, 4)
    once = source.dilate(5, 5)
    assert (first.origin[0] + second.origin[0], first.origin[1] + second.origin[1]) == once.origin == (5, 5)  # the origins add
    expect = MM.morphology(pixels, MM.DILATE, 5, 5, MM.TRANSPARENT)
    check(once, expect, (5, 5), "one dilate")
    assert np.array_equal(second.download_level(0), expect)
    for edge in EDGES:
        opened = source.erode(2, 3, edge).dilate(2, 3, edge)  # an opening
        model = MM.morphology(MM.morphology(pixels, MM.ERODE, 2, 3, int(edge)), MM.DILATE, 2, 3, int(edge))
        check(opened, model, origin_of(MorphologyOp.Dilate, edge, 2, 3), ("opening", edge.name))
    # the result is an image like any other: mipmaps and blur work on it, and only level 0 of a source with mipmaps is read
    chained = Image(renderer, pixels)
    chained.generate_mipmaps()
    assert np.array_equal(chained.dilate(5, 5).download_level(0), expect)
    once.generate_mipmaps()
    chain = mip_model.chain(expect)
    assert once.levels == len(chain) and all(np.array_equal(once.download_level(l), v) for l, v in enumerate(chain))


def test_a_layer_gets_an_outline_and_comes_back_into_a_frame(no_pins):
    """snapshot -> dilate(2) (TRANSPARENT) -> color_filter(flood) -> composite under the layer with DST_OVER at the grown origin ->
    Frame.load_image -> download: the chain of the three numpy models, byte for byte."""
    r = R.Renderer(R.Configuration(), device=0)
    shapes, transforms, colours, _ = stack(seed=7, size=SIZE, n=12, radius=(16, 36))
    scene = R.Scene(r, batch_from_shapes(shapes))
    frame = R.Frame(r, SIZE, SIZE)
    frame.clear()
    scene.render(frame, transforms, colours)
    drawn = frame.download()
    assert (drawn[..., 3] > 0).mean() > 0.3
    snapshot = Image.from_frame(frame)
    grown = snapshot.dilate(2)
    grown_model = MM.morphology(drawn, MM.DILATE, 2, 2, MM.TRANSPARENT)
    check(grown, grown_model, (2, 2), "the dilated snapshot")
    flood = ColorMatrix.flood(0.9, 0.1, 0.2, 1.0)
    outline = grown.color_filter(flood)
    assert outline.origin == (2, 2)
    outline_model = FM.texels(grown_model, FM.flood(0.9, 0.1, 0.2, 1.0))
    assert np.array_equal(outline.download_level(0), outline_model)
    composed = snapshot.composite(outline, CompositeOp.DstOver, offset=(-2, -2))
    second = R.Frame(r, SIZE, SIZE)
    second.load_image(composed)
    got = second.download()
    composed_model = CM.composite(drawn, outline_model, CM.DST_OVER, CM.NORMAL, 255, -2, -2)
    bad = (got != composed_model).any(axis=2)
    assert not bad.any(), f"{int(bad.sum())} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}"
    assert int((got[..., 3] > 0).sum()) > int((drawn[..., 3] > 0).sum())  # the outline adds coverage


def test_the_morphology_refuses_what_it_cannot_do(renderer, no_pins):
    lib = _ffi.load_library()
    source = Image(renderer, pixels_of(5, 3))
    out = C.c_void_p(0x1234)
    assert lib.crh_image_morphology(None, 1, 1, 1, 0, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_morphology(source.handle, 1, 1, 1, 0, None) == _ffi.ERR_INVALID_ARGUMENT
    for op, rx, ry, edge, text in ((2, 1, 1, 0, "op is above CRH_MORPHOLOGY_DILATE"), (1, 1, 1, 4, "edge is above CRH_BLUR_EDGE_REFLECT"),
                                   (1, 193, 1, 1, "a radius exceeds CRH_MAX_MORPHOLOGY_RADIUS"), (0, 1, 193, 0, "a radius exceeds CRH_MAX_MORPHOLOGY_RADIUS")):
        assert lib.crh_image_morphology(source.handle, op, rx, ry, edge, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
        assert lib.crh_last_error().decode() == "crh_morphology_size: " + text
    wide = Image(renderer, pixels_of(16384, 1))
    assert lib.crh_image_morphology(wide.handle, 1, 1, 0, 0, C.byref(out)) == _ffi.ERR_UNSUPPORTED and out.value == 0x1234
    assert lib.crh_last_error().decode() == "crh_morphology_size: a side of the grown result exceeds 16384"
    with pytest.raises(ContrastError):
        source.morphology(MorphologyOp.Dilate, 1, edge=4)
    with pytest.raises(ContrastError):
        source.dilate(193)
    check(source.dilate(192, 192, BlurEdge.Pad), MM.morphology(pixels_of(5, 3), MM.DILATE, 192, 192, MM.PAD), (0, 0), "the limit itself")
