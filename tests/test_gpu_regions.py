"""crh_image_crop, crh_image_create_from_frame_region and crh_image_statistics (include/contrast_hip.h, "Regions and statistics") on the
GPU: k_image_crop byte for byte and k_image_stats / k_image_stats_merge counter for counter against the numpy model of
tests/regions_model.py, at the smallest shapes where the kernels' geometry can go wrong — result widths of each group size V = 4, 2, 1
with aligned and unaligned shifts and source widths (the wide and the narrow source path), a row one group wider than a workgroup's
segment, heights of 1 and one more than the rows a launch gives its workgroups, every class of rectangle, bins above 2^16 and above
2^24 — and the chain the calls are for: a filter of the trimmed layer is the filter of the whole canvas."""
import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, Channel, CompositeOp, ContrastError, Path, _ffi, batch_from_shapes
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image

import regions_model as M
from test_gpu_blending import no_pins  # noqa: F401

pytestmark = pytest.mark.gpu

# Result widths of each group size: V = 4, 2, 1 texels per lane (the most that divides the width). A workgroup's row segment is 256 lanes.
WIDTHS = {4: 8, 2: 6, 1: 5}
# The grids' caps: kStreamBlocks = 8192 (csrc/image_geometry.hpp) workgroups of one row for k_image_crop; kStatsBlocks = 512 (csrc/image_filter.hip)
# workgroups of kStatsRows = 2 rows of lanes for k_image_stats, whose lanes take their rows two at a time. A one-segment image of more rows than a grid
# covers at once — 8192, and 1024 — makes a row loop turn.
CROP_ROWS, STATS_ROWS = 8192, 1024


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


def check(image, expect, origin, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == origin, (what, image.width, image.height, image.origin)
    assert image.levels == 1, what
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"
    return got


def check_crop(image, src, x, y, w, h, what=None):
    return check(image.crop(x, y, w, h), M.crop(src, x, y, w, h), (-x, -y), (what, src.shape, x, y, w, h))


def check_statistics(image, src, channel=M.A, threshold=1, what=None):
    got = image.statistics(Channel(channel), threshold)
    histogram, bounds, count = M.statistics(src, channel, threshold)
    wrong = np.argwhere(got.histogram != histogram)
    assert wrong.size == 0, f"{what} {src.shape}: {len(wrong)} bins differ, first [channel, code] {tuple(wrong[0])}: {got.histogram[tuple(wrong[0])]}, the model {histogram[tuple(wrong[0])]}"
    assert got.bounds == bounds and got.count == count, (what, src.shape, channel, threshold, got.bounds, bounds, got.count, count)
    return got


# ---- crop

@pytest.mark.parametrize("v", (4, 2, 1))
def test_crop_widths_of_each_group_size_through_the_wide_and_the_narrow_source_path(v, renderer, no_pins):
    """x = 0 and v mod V with a source width that V divides (the wide path where V > 1) and one it does not (the narrow path), and x = 1."""
    width = WIDTHS[v]
    for source_w in (12, 13):
        src = M.random_texels(source_w, 9, 100 * v + source_w)
        source = Image(renderer, src)
        for x in (0, v, -v, 1, -1, 2, source_w - 3, -width + 1):
            for y, height in ((0, 9), (-2, 5), (3, 1), (7, 6)):
                check_crop(source, src, x, y, width, height, "paths")


@pytest.mark.parametrize("v", (4, 2, 1))
def test_crop_one_group_wider_than_a_row_segment_and_one_row_beyond_the_grid(v, renderer, no_pins):
    width = 256 * v + v
    src = M.random_texels(width + 5, 4, v)
    source = Image(renderer, src)
    for x in (0, 3, -4):
        check_crop(source, src, x, -1, width, 5, "segment")  # two workgroups along x, the second with one live lane
    tall = M.random_texels(WIDTHS[v] + 1, CROP_ROWS + 1, 7 * v)
    source = Image(renderer, tall)
    for x in (0, 1):
        check_crop(source, tall, x, 0, WIDTHS[v], CROP_ROWS + 1, "rows")  # the last row is a workgroup's second
    check_crop(source, tall, 0, CROP_ROWS, WIDTHS[v], 1, "one row")


def test_crop_rectangles_of_every_class(renderer, no_pins):
    for w, h in ((13, 7), (1, 1), (32, 6)):
        src = M.random_texels(w, h, w + h)
        source = Image(renderer, src)
        for name, x, y, width, height in M.rectangles(w, h):
            check_crop(source, src, x, y, width, height, name)


def test_crop_makes_canvases_and_backdrops_and_composes(renderer, no_pins):
    src = M.random_texels(20, 10, 4, premultiplied=False)  # colours above their alpha: copied as they are
    source = Image(renderer, src)
    canvas = source.crop(-(2 ** 31), 2 ** 31 - 1, 64, 48)
    assert not canvas.download_level(0).any() and canvas.origin == (2 ** 31, -(2 ** 31 - 1))
    backdrop = check_crop(source, src, -7, -5, 40, 30)
    first = source.crop(-7, -5, 40, 30)
    second = first.crop(9, 6, 11, 8)
    check(second, M.crop(src, 2, 1, 11, 8), (-2, -1), "a crop of a crop")
    assert (backdrop[5:15, 7:27] == src).all()
    filtered = first.color_filter()  # a filter that keeps the origin keeps a crop's
    assert filtered.origin == (7, 5)
    with pytest.raises(ContrastError) as refused:
        source.crop(0, 0, 0, 4)
    assert refused.value.status == _ffi.ERR_INVALID_ARGUMENT
    with pytest.raises(ContrastError):
        source.crop(0, 0, 4, 16385)


# ---- frame regions

def scene_frame(r, width=96, height=64, fmt=None):
    """Three rectangles, one of them translucent and one over the frame's edge, in pixel coordinates"""
    shapes = [([], [Path.from_rect((30.0, 20.0), (20.0, 12.0))]), ([], [Path.from_rect((70.0, 40.0), (15.0, 18.0))]), ([], [Path.from_rect((90.0, 8.0), (10.0, 5.0))])]
    t = np.zeros(16, dtype=np.float32)
    t[0], t[5], t[10], t[15], t[12], t[13] = 2.0 / width, -2.0 / height, 1.0, 1.0, -1.0, 1.0
    scene = R.Scene(r, batch_from_shapes(shapes))
    frame = R.Frame(r, width, height) if fmt is None else R.Frame(r, width, height, fmt)
    frame.clear()
    scene.render(frame, np.tile(t.reshape(1, 16), (3, 1)), np.float32([(1.0, 0.2, 0.1, 1.0), (0.1, 0.5, 1.0, 0.6), (0.3, 1.0, 0.3, 1.0)]))
    return frame


REGIONS = ((0, 0, 96, 64), (12, 9, 40, 30), (13, 9, 41, 30), (50, 20, 45, 44), (-5, -7, 20, 20), (60, 30, 60, 60), (-8, -8, 112, 80), (96, 0, 8, 8), (0, -9, 9, 9),
           (-2 ** 31, 3, 4, 4), (2 ** 31 - 1, 2 ** 31 - 1, 5, 5))


def test_a_frame_region_is_the_crop_of_the_snapshot(renderer, no_pins):
    frame = scene_frame(renderer)
    drawn = frame.download()
    assert (drawn[..., 3] > 0).mean() > 0.1 and ((drawn[..., 3] > 0) & (drawn[..., 3] < 255)).any()
    whole = Image.from_frame(frame)
    assert np.array_equal(whole.download_level(0), drawn)
    for x, y, w, h in REGIONS:
        region = Image.from_frame(frame, region=(x, y, w, h))
        expect = whole.crop(x, y, w, h).download_level(0)
        assert np.array_equal(expect, M.crop(drawn, x, y, w, h))
        check(region, expect, (-x, -y), (x, y, w, h))
    # a snapshot: later passes into the frame do not change it
    region = Image.from_frame(frame, region=(12, 9, 40, 30))
    frame.clear()
    check(region, M.crop(drawn, 12, 9, 40, 30), (-12, -9), "after a clear")


def test_a_cleared_frame_gives_zeros_and_refused_frames_are_refused_alike(renderer, no_pins):
    frame = R.Frame(renderer, 96, 64)
    frame.clear()
    for x, y, w, h in ((0, 0, 96, 64), (-3, 5, 17, 9)):
        assert not Image.from_frame(frame, region=(x, y, w, h)).download_level(0).any()
    half = R.Frame(renderer, 16, 16, R.FORMAT_RGBA16F)
    half.clear()
    slab = R.Frame(renderer, 160, 160)
    slab.set_tile_rows(0, 64)
    for refused in (half, slab):
        with pytest.raises(ContrastError) as whole:
            Image.from_frame(refused)
        with pytest.raises(ContrastError) as part:
            Image.from_frame(refused, region=(0, 0, 8, 8))
        assert whole.value.status == part.value.status == _ffi.ERR_UNSUPPORTED
    with pytest.raises(ContrastError) as empty:
        Image.from_frame(frame, region=(0, 0, 0, 8))
    assert empty.value.status == _ffi.ERR_INVALID_ARGUMENT


def test_a_frame_wider_than_an_image_is_snapshotted_in_regions(renderer, no_pins):
    width = 16400
    pixels = M.random_texels(width, 3, 16)
    frame = R.Frame(renderer, width, 3)
    frame.upload(pixels)
    with pytest.raises(ContrastError) as whole:
        Image.from_frame(frame)
    assert whole.value.status == _ffi.ERR_UNSUPPORTED
    for x, w in ((0, 16384), (16384, 16), (16390, 20), (16399, 1)):
        check(Image.from_frame(frame, region=(x, -1, w, 5)), M.crop(pixels, x, -1, w, 5), (-x, 1), ("wide", x, w))


# ---- statistics

@pytest.mark.parametrize("v", (4, 2, 1))
def test_statistics_widths_of_each_group_size_and_heights_round_the_grid(v, renderer, no_pins):
    """Heights 1, one more than the grid's rows (a workgroup's second row of a turn) and one more than twice them (its second turn)."""
    for width, height in ((WIDTHS[v], 1), (WIDTHS[v], 9), (WIDTHS[v], STATS_ROWS + 1), (WIDTHS[v], 2 * STATS_ROWS + 1), (256 * v + v, 5)):
        src = M.random_texels(width, height, 10 * v + height)
        src[(np.arange(height) % 5) == 0] = 0  # whole rows of zeros beside noise
        image = Image(renderer, src)
        for channel, threshold in ((M.A, 1), (M.R, 255), (M.G, 1), (M.B, 128)):
            check_statistics(image, src, channel, threshold, "widths")
    last = np.zeros((2 * STATS_ROWS + 1, WIDTHS[v], 4), dtype=np.uint8)
    last[-1, -1] = (0, 0, 0, 1)  # the only texel inside is in the last turn's row
    assert check_statistics(Image(renderer, last), last).bounds == (WIDTHS[v] - 1, 2 * STATS_ROWS, WIDTHS[v], 2 * STATS_ROWS + 1)


@pytest.mark.parametrize("size", ((257, 3), (1028, 67)))
def test_statistics_of_single_texels_in_the_corners_and_of_none(size, renderer, no_pins):
    w, h = size
    corners = ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))
    for x, y in corners:
        src = np.zeros((h, w, 4), dtype=np.uint8)
        src[y, x] = (3, 2, 1, 255)
        for channel, threshold in ((M.A, 1), (M.A, 255), (M.R, 3), (M.G, 3)):
            got = check_statistics(Image(renderer, src), src, channel, threshold, "corner")
            assert got.bounds == ((x, y, x + 1, y + 1) if channel != M.G else (0, 0, 0, 0))
    src = np.zeros((h, w, 4), dtype=np.uint8)
    src[0, 0] = src[h - 1, w - 1] = (0, 0, 0, 9)
    assert check_statistics(Image(renderer, src), src, M.A, 9).bounds == (0, 0, w, h)
    none = check_statistics(Image(renderer, src), src, M.A, 10)
    assert none.bounds == (0, 0, 0, 0) and none.count == 0


def test_statistics_of_noise_of_rows_and_columns_of_one_value_and_of_a_layer_that_is_mostly_empty(renderer, no_pins):
    w, h = 1028, 67
    rng = np.random.default_rng(5)
    noise = M.random_texels(w, h, 6, premultiplied=False)
    assert all(len(np.unique(noise[..., c])) == 256 for c in range(4))  # the codes span all 256 values
    rows = np.repeat(rng.integers(0, 256, (h, 1, 4), dtype=np.uint8), w, axis=1)     # every row one value: a wave-uniform run that changes with the row
    rows[10:20] = rows[10]                                                           # ... and one that lasts
    columns = np.repeat(rng.integers(0, 256, (1, w, 4), dtype=np.uint8), h, axis=0)  # every column one value: no run
    layer = np.zeros((h, w, 4), dtype=np.uint8)
    layer[30:50, 700:800] = M.random_texels(100, 20, 7)
    halves = np.zeros((h, w, 4), dtype=np.uint8)
    halves[:, 300:] = (9, 8, 7, 200)  # a wave that is partly one value and partly another
    for name, src in (("noise", noise), ("rows", rows), ("columns", columns), ("layer", layer), ("halves", halves)):
        image = Image(renderer, src)
        for channel in range(4):
            for threshold in (1, 255):
                check_statistics(image, src, channel, threshold, name)


def test_statistics_bins_above_16_and_above_24_bits(renderer, no_pins):
    for texel in ((0, 0, 0, 0), (10, 20, 30, 255)):
        src = np.full((512, 512, 4), texel, dtype=np.uint8)
        got = check_statistics(Image(renderer, src), src, M.A, 255, texel)
        assert all(int(got.histogram[c, texel[c]]) == 262144 for c in range(4))
    w, h, texel, other = 4104, 4100, (7, 77, 177, 255), (1, 2, 3, 4)
    src = np.full((h, w, 4), texel, dtype=np.uint8)
    src[h - 1, w - 1] = other  # the last group of the last row is not one value
    got = Image(renderer, src).statistics(Channel.A, 255)  # one upload, one call; the model here is arithmetic
    n = w * h - 1
    assert n > 2 ** 24
    expect = np.zeros((4, 256), dtype=np.uint32)
    for c in range(4):
        expect[c, texel[c]] += n
        expect[c, other[c]] += 1
    assert (got.histogram == expect).all(), np.argwhere(got.histogram != expect)[:4]
    assert got.bounds == (0, 0, w, h) and got.count == n


# ---- end to end: what the calls are for

def test_a_filter_of_the_trimmed_layer_is_the_filter_of_the_canvas(renderer, no_pins):
    """Under BlurEdge.Transparent the texels outside the content add zero to every sum, maximum and distance, so filtering the 300 x 200
    trimmed layer gives, byte for byte, what filtering the 1024 x 1024 canvas gives on that rectangle, and nothing lies outside it."""
    patch = Image.turbulence(renderer, 300, 200, 0.05, octaves=2, seed=3, opaque=True)
    empty = patch.crop(-5000, -5000, 1024, 1024)  # a transparent canvas, made by a crop that misses
    assert empty.statistics().count == 0
    canvas = empty.composite(patch, CompositeOp.SrcOver, offset=(700, 400))
    assert canvas.bounds() == (700, 400, 1000, 600)
    trimmed = canvas.trim()
    assert (trimmed.width, trimmed.height) == (300, 200) and trimmed.origin == (-700, -400)
    assert np.array_equal(trimmed.download_level(0), patch.download_level(0))
    margin = canvas.trim(margin=4)
    assert (margin.width, margin.height) == (308, 208) and margin.origin == (-696, -396)
    nothing = empty.trim()  # nothing inside: the 1 x 1 crop at (0, 0), which keeps the origin of what it was cut from
    assert (nothing.width, nothing.height, nothing.origin) == (1, 1, empty.origin) and empty.origin == (5000, 5000)
    for name, apply in (("blur", lambda image: image.blur(5, edge=BlurEdge.Transparent)), ("dilate", lambda image: image.dilate(3, edge=BlurEdge.Transparent)),
                        ("distance_field", lambda image: image.distance_field(6, edge=BlurEdge.Transparent))):
        small, large = apply(trimmed), apply(canvas)
        # texel (0, 0) of `small` in `large`: trimmed's (0, 0) is the canvas's -trimmed.origin, and each result grew by its own origin
        x = -trimmed.origin[0] - small.origin[0] + large.origin[0]
        y = -trimmed.origin[1] - small.origin[1] + large.origin[1]
        whole = large.download_level(0)
        assert np.array_equal(small.download_level(0), whole[y:y + small.height, x:x + small.width]), name
        x0, y0, x1, y1 = large.bounds()
        assert x <= x0 < x1 <= x + small.width and y <= y0 < y1 <= y + small.height, (name, (x0, y0, x1, y1))
        for channel in (Channel.R, Channel.G, Channel.B):
            assert large.statistics(channel, 1).count == small.statistics(channel, 1).count, name
