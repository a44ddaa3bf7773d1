"""crh_image_blur (include/contrast_hip.h) on the GPU: k_image_blur_h and k_image_blur_v bit for bit against the integer model of
tests/blur_model.py, with the taps crh_blur_taps hands out — every size that crosses a block border of either kernel, every edge, radii from 0
to 192 — and the way from a rendered frame to a drop shadow drawn as an image paint."""
import ctypes as C

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, ContrastError, Path, _ffi, batch_from_shapes, blur_taps
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Filter, Image, ImagePaint

import blur_model as BM
import mip_model as MM
from test_gpu_blending import no_pins, stack  # noqa: F401
from test_gpu_image_paints import tol_of

pytestmark = pytest.mark.gpu

SIZE = MM.SIZE
# (1, 1) .. (33, 17): one workgroup of either kernel, partly filled. (300, 70): k_image_blur_h's 256-texel row segment with its apron is crossed
# by 44 texels, k_image_blur_v's 64 columns four times and its 32-row block twice, by 6 rows. (70, 300) turns that round: nine row blocks and
# a 32-row LDS chunk that ends inside the source.
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17), (300, 70), (70, 300)]
# (0.01, 0.01): R = 1 with the taps (65536, 0) — the identity with a radius, which the kernels' 16-bit tap words cannot hold and the host routes apart
SIGMAS = [(0.0, 0.0), (0.3, 0.0), (0.0, 2.5), (1.0, 1.0), (2.5, 7.0), (64.0, 64.0), (0.01, 0.01)]
EDGES = [BlurEdge.Transparent, BlurEdge.Pad, BlurEdge.Repeat, BlurEdge.Reflect]


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


_pixels = {}


def pixels_of(w, h):
    """Random premultiplied texels of a size, made once and never written."""
    if (w, h) not in _pixels:
        _pixels[(w, h)] = BM.random_premultiplied(np.random.RandomState(w + 3 * h), w, h)
        _pixels[(w, h)].setflags(write=False)
    return _pixels[(w, h)]


def expect_of(pixels, sigma_x, sigma_y, edge):
    (qx, rx), (qy, ry) = blur_taps(sigma_x), blur_taps(sigma_y)
    return BM.blur(pixels, qx, qy, int(edge)), (rx, ry)


def check(image, expect, origin, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == origin, (what, image.width, image.height, image.origin)
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}"


@pytest.mark.parametrize("sigmas", SIGMAS, ids=[f"{x:g}-{y:g}" for x, y in SIGMAS])
@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_blur_equals_the_integer_model(size, edge, sigmas, renderer, no_pins):
    pixels = pixels_of(*size)
    source = Image(renderer, pixels)
    expect, (rx, ry) = expect_of(pixels, *sigmas, edge)
    grown = edge == BlurEdge.Transparent
    assert expect.shape[:2] == (size[1] + (2 * ry if grown else 0), size[0] + (2 * rx if grown else 0))
    blurred = source.blur(*sigmas, edge)
    check(blurred, expect, (rx, ry) if grown else (0, 0), (size, edge.name, sigmas))
    assert blurred.levels == 1
    if sigmas == (0.0, 0.0):
        assert np.array_equal(expect, pixels)  # a copy
    assert np.array_equal(source.download_level(0), pixels)


def saturated_pixels(kind, w, h):
    """All 255, or a checker of period 1 of (0, 0, 0, 0) and (255, 255, 255, 255): the inputs that take the 32-bit sums of both kernels to their
    bounds (k_image_blur_h: 65536 * 255; k_image_blur_v: 65536 * 65280) and, for the checker, make every lane alternate between 0 and the bound."""
    if (kind, w, h) not in _pixels:
        j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        on = np.ones((h, w), dtype=bool) if kind == "white" else (i + j) % 2 == 0
        _pixels[(kind, w, h)] = np.repeat(np.where(on, 255, 0).astype(np.uint8)[:, :, None], 4, axis=2)
        _pixels[(kind, w, h)].setflags(write=False)
    return _pixels[(kind, w, h)]


@pytest.mark.parametrize("sigmas", [(64.0, 64.0), (64.0, 0.0), (0.0, 64.0)], ids=["64-64", "64-0", "0-64"])
@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
@pytest.mark.parametrize("size", [(70, 300), (300, 70)], ids=["70x300", "300x70"])
@pytest.mark.parametrize("kind", ["white", "checker"])
def test_a_saturated_image_at_the_largest_radius(kind, size, edge, sigmas, renderer, no_pins):
    """The taps of an axis sum to exactly 65536, so an all-255 image stays all 255 under every edge that reads texels of the image only; under
    TRANSPARENT, and for the checker under every edge, the integer model says what the partial sums round to."""
    pixels = saturated_pixels(kind, *size)
    expect, (rx, ry) = expect_of(pixels, *sigmas, edge)
    grown = edge == BlurEdge.Transparent
    assert (rx, ry) == tuple(192 if s else 0 for s in sigmas)
    if kind == "white" and not grown:
        assert (expect == 255).all()
    else:
        assert ((expect > 0) & (expect < 255)).mean() > 0.2  # (partial sums: the rounding decides)
    check(Image(renderer, pixels).blur(*sigmas, edge), expect, (rx, ry) if grown else (0, 0), (kind, size, edge.name, sigmas))


@pytest.mark.parametrize("edge", [BlurEdge.Reflect, BlurEdge.Pad], ids=["Reflect", "Pad"])
def test_the_widest_index_range(edge, renderer, no_pins):
    pixels = pixels_of(16384, 1)
    source = Image(renderer, pixels)
    expect, _ = expect_of(pixels, 64.0, 0.0, edge)
    check(source.blur(64.0, 0.0, edge), expect, (0, 0), ("16384x1", edge.name))


def test_a_grown_side_above_16384_is_unsupported(renderer, no_pins):
    source = Image(renderer, pixels_of(16384, 1))
    with pytest.raises(ContrastError) as refused:
        source.blur(1.0, 0.0, BlurEdge.Transparent)
    assert refused.value.status == _ffi.ERR_UNSUPPORTED
    tall = Image(renderer, np.ascontiguousarray(pixels_of(16384, 1).transpose(1, 0, 2)))
    with pytest.raises(ContrastError) as refused:
        tall.blur(0.0, 0.3, BlurEdge.Transparent)
    assert refused.value.status == _ffi.ERR_UNSUPPORTED
    assert tall.blur(1.0, 0.0, BlurEdge.Transparent).width == 7  # (the other axis grows freely)


def test_an_impulse_is_the_outer_product_of_the_taps(renderer, no_pins):
    white = np.full((1, 1, 4), 255, dtype=np.uint8)
    q, radius = blur_taps(2.0)
    assert radius == 6
    q = [int(v) for v in q]
    blurred = Image(renderer, white).blur(2.0)  # sigma_y = sigma_x, TRANSPARENT
    assert (blurred.width, blurred.height, blurred.origin) == (13, 13, (6, 6))
    got = blurred.download_level(0)
    for j in range(13):
        for i in range(13):
            expect = (q[abs(j - 6)] * ((q[abs(i - 6)] * 255 + 128) >> 8) + (1 << 23)) >> 24
            assert (got[j, i] == expect).all(), (i, j, got[j, i], expect)


def test_the_source_is_untouched_and_the_result_is_an_image_like_any_other(renderer, no_pins):
    pixels = pixels_of(33, 17)
    plain, chained = Image(renderer, pixels), Image(renderer, pixels)
    chained.generate_mipmaps()
    levels = [chained.download_level(l) for l in range(chained.levels)]
    a, b = plain.blur(2.5, 1.0, BlurEdge.Reflect), chained.blur(2.5, 1.0, BlurEdge.Reflect)
    assert np.array_equal(plain.download_level(0), pixels) and plain.levels == 1
    assert chained.levels == len(levels) and all(np.array_equal(chained.download_level(l), v) for l, v in enumerate(levels))
    assert np.array_equal(a.download_level(0), b.download_level(0))  # only level 0 is read
    assert a.levels == b.levels == 1 and a.origin == (0, 0) and plain.origin == (0, 0)
    bytes_of = a.download_level(0)
    a.generate_mipmaps()
    chain = MM.chain(bytes_of)
    assert a.levels == len(chain) and all(np.array_equal(a.download_level(l), v) for l, v in enumerate(chain))


def _blit(r, image, colour, size):
    """test_gpu_image_paints._blit with a tint: one rectangle over the whole frame, path = pixel coordinates, m = the identity, NEAREST."""
    scene = R.Scene(r, batch_from_shapes([([], [Path.from_rect((size[0] / 2.0, size[1] / 2.0), (size[0] / 2.0, size[1] / 2.0))])]))
    t = np.zeros(16, dtype=np.float32)
    t[0], t[5], t[10], t[15], t[12], t[13] = 2.0 / size[0], -2.0 / size[1], 1.0, 1.0, -1.0, 1.0
    scene.set_paints([ImagePaint(image, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), Filter.Nearest)], [0])
    return scene, t.reshape(1, 16), np.float32([colour])


def test_a_frame_becomes_a_shadow(no_pins):
    r = R.Renderer(R.Configuration(), device=0)
    shapes, transforms, colours, _ = stack(seed=7, size=SIZE, n=12, radius=(16, 36))
    scene = R.Scene(r, batch_from_shapes(shapes))
    source = R.Frame(r, SIZE, SIZE)
    source.clear()
    scene.render(source, transforms, colours)
    drawn = source.download()
    assert (drawn[..., 3] > 0).mean() > 0.3
    snapshot = Image.from_frame(source)
    blurred = snapshot.blur(3)
    expect, (rx, ry) = expect_of(drawn, 3.0, 3.0, BlurEdge.Transparent)
    assert (rx, ry) == (9, 9)
    check(blurred, expect, (9, 9), "snapshot")
    size = (blurred.width, blurred.height)
    assert size == (SIZE + 18, SIZE + 18)
    white, t, colour = _blit(r, blurred, (1.0, 1.0, 1.0, 1.0), size)
    shadow, _, tint = _blit(r, blurred, (0.0, 0.0, 0.0, 0.5), size)
    snapshot.destroy()
    blurred.destroy()  # the paint tables keep the blur's output alive
    frame = R.Frame(r, size[0], size[1])
    frame.clear()
    white.render(frame, t, colour)
    assert np.array_equal(frame.download(), expect)
    frame.clear()
    shadow.render(frame, t, tint)
    got = frame.download()
    assert not got[..., :3].any()
    tol = tol_of("over", False, 0.0)
    worst = np.abs(got[..., 3] / 255.0 - 0.5 * expect[..., 3] / 255.0).max()
    assert worst <= tol, (worst * 255, tol * 255)
    assert got[..., 3].max() > 60  # (a shadow, not an empty frame)


def test_the_blur_refuses_what_it_cannot_do(renderer, no_pins):
    lib = _ffi.load_library()
    source = Image(renderer, pixels_of(5, 3))
    out = C.c_void_p(0x1234)
    assert lib.crh_image_blur(None, 1.0, 1.0, 0, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_blur(source.handle, 1.0, 1.0, 0, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_image_blur(source.handle, 1.0, 1.0, 4, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_blur(source.handle, float("nan"), 1.0, 1, C.byref(out)) == _ffi.ERR_NON_FINITE and out.value == 0x1234
    assert lib.crh_image_blur(source.handle, 1.0, 64.5, 1, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_blur(source.handle, 1.0, -0.5, 1, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    with pytest.raises(ContrastError):
        source.blur(1.0, edge=4)
    assert np.array_equal(source.blur(1.0, edge=BlurEdge.Pad).download_level(0), expect_of(pixels_of(5, 3), 1.0, 1.0, BlurEdge.Pad)[0])
