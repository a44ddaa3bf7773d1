"""crh_image_distance_field (include/contrast_hip.h) on the GPU: k_image_distance_v and k_image_distance_h byte for byte against the numpy
model of tests/distance_model.py, with no tolerance and no excluded texel, at the smallest shapes where the kernels can go wrong — widths
round a wave and a row segment, heights round the vertical kernel's row blocks on both sides of the launcher's switch between them, aprons
larger than the image and the largest aprons on rows wider than a segment, blocks with nothing in them, colours above their alpha as the
shape's channel, filled shapes and noise with long scans, the grown origin, the last squared distance that counts, the longest axes — and
the result as a source of the other image calls."""
import ctypes as C
import itertools

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, Channel, CompositeOp, ContrastError, DistanceMode, DistantLight, _ffi, distance_texels
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image

import color_filter_model as FM
import composite_model as CM
import distance_model as M
import layers_model
import lighting_model as LM
import mip_model
import turbulence_model as TM
from test_gpu_blending import no_pins  # noqa: F401

pytestmark = pytest.mark.gpu

MODES = (M.OUTSIDE, M.INSIDE)
# k_image_distance_h's row segment is 256 texels, one per lane of four waves; k_image_distance_v's block is 64 columns (one wave) by
# 32 rows for spreads up to 16 and by 128 rows above (kDistanceSegment, kDistanceColumns and launch_image_distance_v in
# csrc/image_filter.hip).
WIDTHS = (1, 63, 64, 65, 255, 256, 257, 513)


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


def mask(w, h, seed, density):
    """A premultiplied image whose alpha is random where a texel in 1 / density is chosen and 0 elsewhere; its colours lie below alpha"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    src[..., :3] = np.minimum(src[..., :3], src[..., 3:])
    src[rng.random((h, w)) >= density] = 0
    return src


def check(image, expect, origin, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == origin, (what, image.width, image.height, image.origin)
    assert image.levels == 1, what
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"
    return got


def run_and_check(source, src, spread, mode, edge, channel=M.A, threshold=128):
    expect = M.distance_field(src, spread, mode, channel, threshold, edge)
    origin = (spread, spread) if M.grows(mode, edge) else (0, 0)
    return check(source.distance_field(spread, DistanceMode(mode), Channel(channel), threshold, BlurEdge(edge)), expect, origin, (src.shape, spread, mode, edge, channel, threshold))


@pytest.mark.parametrize("width", WIDTHS)
def test_widths_round_a_wave_and_a_row_segment(width, renderer, no_pins):
    """Height 3; spread 3 keeps the apron inside a neighbouring segment, spread 40 reaches across one."""
    src = mask(width, 3, width, 0.08)
    source = Image(renderer, src)
    for spread, mode, edge in itertools.product((3, 40), MODES, M.EDGES):
        run_and_check(source, src, spread, mode, edge)
    assert np.array_equal(source.download_level(0), src)


@pytest.mark.parametrize("spread", (1, 3, 255))
def test_heights_round_the_window_and_the_row_blocks(spread, renderer, no_pins):
    """Width 5; heights 1, 2 spread, 2 spread + 1 and 2 spread + 2 (the window), and one row less than, exactly and one row more than the
    kernel's row block of this spread, as source heights and, grown by 2 spread, as result heights."""
    block = 32 if spread <= 16 else 128
    heights = {1, 2 * spread, 2 * spread + 1, 2 * spread + 2, block - 1, block, block + 1, block + 1 - 2 * spread if block + 1 > 2 * spread else 1}
    for height in sorted(heights):
        src = mask(5, height, height, 0.1)
        src[height // 2, 2] = 255  # (never empty)
        source = Image(renderer, src)
        for mode, edge in ((M.OUTSIDE, M.TRANSPARENT), (M.OUTSIDE, M.REFLECT), (M.INSIDE, M.TRANSPARENT), (M.INSIDE, M.REPEAT)):
            run_and_check(source, src, spread, mode, edge, M.A, 1)


@pytest.mark.parametrize("spread", (16, 17))
def test_row_blocks_on_both_sides_of_the_launchers_switch(spread, renderer, no_pins):
    """launch_image_distance_v takes 32-row blocks up to spread 16 and 128-row blocks from 17: both spreads on heights one row less than,
    exactly and one row more than either block, so each kernel runs a last block of one row, a full one and, for the other's heights,
    blocks it would not have been given. Width 65: two column blocks, the second of one lane."""
    for height in (31, 32, 33, 127, 128, 129):
        src = mask(65, height, 1000 * spread + height, 0.1)
        src[height // 2, 64] = 255  # (never empty, and the lone lane's column has a target)
        source = Image(renderer, src)
        for mode, edge in ((M.OUTSIDE, M.TRANSPARENT), (M.OUTSIDE, M.REFLECT), (M.INSIDE, M.TRANSPARENT), (M.INSIDE, M.REPEAT)):
            run_and_check(source, src, spread, mode, edge, M.A, 1)


@pytest.mark.parametrize("size", [(300, 3), (513, 2)], ids=["300x3", "513x2"])
def test_the_largest_aprons_on_rows_wider_than_a_segment(size, renderer, no_pins):
    """Spreads 129 and 255 under the three same-size edges on rows of two and of three segments: a segment of k_image_distance_h stages
    bytes from beyond both its neighbours, the first and the last one through the wrap (at 255 more than a whole 300-texel row of it).
    One inside texel at column 0, one at the last column — each is seen from the other end of the row only through REPEAT — and a
    sparse mask."""
    w, h = size
    first, last = np.zeros((h, w, 4), dtype=np.uint8), np.zeros((h, w, 4), dtype=np.uint8)
    first[0, 0], last[h - 1, w - 1] = 255, 255
    for src in (first, last, mask(w, h, w, 0.01)):
        assert src[..., 3].any()
        source = Image(renderer, src)
        for spread, mode, edge in itertools.product((129, 255), MODES, (M.PAD, M.REPEAT, M.REFLECT)):
            run_and_check(source, src, spread, mode, edge)


def test_a_colour_above_its_alpha_is_the_shape_as_it_is_stored(renderer, no_pins):
    """Straight texels, alpha 0 .. 199 and colours above it: the shape's channel is R, G or B, "the stored code, as it is" — no clamp to
    alpha, and not alpha's inside map, which differs from the channel's in every case here."""
    src = layers_model.random_texels(np.random.RandomState(31), "straight", 70, 37)
    assert not layers_model.premultiplied(src) and src[..., 3].max() <= 199
    source = Image(renderer, src)
    for channel, threshold in itertools.product((M.R, M.G, M.B), (1, 128, 255)):
        assert not np.array_equal(M.inside_map(src, channel, threshold), M.inside_map(src, M.A, threshold)), (channel, threshold)
        assert not np.array_equal(M.inside_map(src, channel, threshold), M.inside_map(np.minimum(src, src[..., 3:]), channel, threshold)), (channel, threshold)
        for mode, edge in itertools.product(MODES, (M.TRANSPARENT, M.REFLECT)):
            expect = M.distance_field(src, 5, mode, channel, threshold, edge)
            assert not np.array_equal(expect, M.distance_field(src, 5, mode, M.A, threshold, edge))  # reading alpha instead cannot pass
            run_and_check(source, src, 5, mode, edge, channel, threshold)


@pytest.mark.parametrize("shape", ("disc", "complement", "noise"))
def test_long_scans_over_filled_shapes_and_noise(shape, renderer, no_pins):
    """130 x 70 with long runs of inside and of outside texels: a filled disc of radius 25, its complement, and fractal noise as the
    device makes it, thresholded on R. Deep inside a run distance_scan goes many steps before dx^2 reaches the best value, at a run's rim
    it stops at once: the lanes of a wave stop far apart, at spreads below and above half a segment."""
    w, h = 130, 70
    j, i = np.mgrid[0:h, 0:w]
    if shape == "noise":
        src = TM.turbulence(w, h, (0.03, 0.05), 2, 7, TM.FRACTAL_NOISE, False, True, (0.0, 0.0))  # opaque: R lies round 128
    else:
        inside = (np.hypot(i - 60, j - 33) < 25) == (shape == "disc")
        src = np.repeat((inside * 255).astype(np.uint8)[:, :, None], 4, axis=2)
    inside = M.inside_map(src, M.R, 128)
    assert 0.1 < inside.mean() < 0.9, inside.mean()
    source = Image(renderer, src)
    for spread, mode, edge in itertools.product((40, 128), MODES, (M.TRANSPARENT, M.REFLECT)):
        run_and_check(source, src, spread, mode, edge, M.R, 128)


@pytest.mark.parametrize("size", [(1, 1), (2, 3), (40, 40)], ids=["1x1", "2x3", "40x40"])
def test_the_largest_spread_on_images_smaller_than_the_apron(size, renderer, no_pins):
    """Spread 255 under all four edges: wraps many periods out in both kernels, a result of 511 x 511 from one texel."""
    src = mask(size[0], size[1], 11, 0.05)
    src[0, 0] = 255
    source = Image(renderer, src)
    for mode, edge in itertools.product(MODES, M.EDGES):
        run_and_check(source, src, 255, mode, edge)
    empty = np.zeros_like(src)
    for mode, edge in itertools.product(MODES, (M.TRANSPARENT, M.REPEAT)):
        run_and_check(Image(renderer, empty), empty, 255, mode, edge)


@pytest.mark.parametrize("density", (0.02, 0.7), ids=["sparse", "dense"])
def test_both_modes_under_every_edge(density, renderer, no_pins):
    """130 x 70: more than one block of columns and of rows; channels and thresholds in turn."""
    src = mask(130, 70, 5, density)
    source = Image(renderer, src)
    for n, (mode, edge, spread) in enumerate(itertools.product(MODES, M.EDGES, (9, 40))):
        channel, threshold = (M.A, M.R, M.G, M.B)[n % 4], (128, 1, 255)[n % 3]
        got = run_and_check(source, src, spread, mode, edge, channel, threshold)
        assert np.array_equal(got, distance_texels(src, spread, DistanceMode(mode), Channel(channel), threshold, BlurEdge(edge)))  # the host function runs the same rule
    assert np.array_equal(source.distance_field(6).download_level(0), M.distance_field(src, 6))  # the defaults


def test_blocks_with_nothing_inside_them(renderer, no_pins):
    """The shape lies in one corner of 600 x 300: whole column blocks, row blocks and row segments hold "none" in both passes, beside
    ones that hold both; and an empty and a full image, where every block does."""
    src = np.zeros((300, 600, 4), dtype=np.uint8)
    src[3:9, 2:30] = mask(28, 6, 1, 0.5)
    source = Image(renderer, src)
    for spread, mode, edge in itertools.product((4, 20), MODES, (M.TRANSPARENT, M.PAD)):
        got = run_and_check(source, src, spread, mode, edge)
        if mode == M.OUTSIDE:
            assert (got[-100:, -300:] == 0).all()
    for value, mode, edge in itertools.product((0, 255), MODES, (M.TRANSPARENT, M.REFLECT)):
        flat = np.full((70, 300, 4), value, dtype=np.uint8)
        run_and_check(Image(renderer, flat), flat, 20, mode, edge)


def test_a_single_texel_at_each_corner_and_the_grown_origin(renderer, no_pins):
    """TRANSPARENT OUTSIDE: the result's texel (i, j) is centred on the source's (i - spread, j - spread)."""
    for (x, y), spread in itertools.product(((0, 0), (8, 0), (0, 5), (8, 5)), (1, 4)):
        src = np.zeros((6, 9, 4), dtype=np.uint8)
        src[y, x] = 255
        got = run_and_check(Image(renderer, src), src, spread, M.OUTSIDE, M.TRANSPARENT)
        assert got[y + spread, x + spread, 0] == 255 and (got[..., 0] == 255).sum() == 1
        assert got[y + spread, x + 2 * spread, 0] == 0 and got[y + spread, x + 2 * spread - 1, 0] == 255 - M.code((spread - 1) ** 2, spread)


@pytest.mark.parametrize("spread,at,before", [(3, (3, 0), (2, 2)), (17, (15, 8), (12, 12))])
def test_the_last_squared_distance_that_counts(spread, at, before, renderer, no_pins):
    """One inside texel: a texel at D2 = spread^2 exactly is 0, and one at spread^2 - 1 (8 = 2^2 + 2^2, 288 = 12^2 + 12^2) holds c(spread^2 - 1):
    240 at spread 3; at spread 17 255 sqrt(288) / 17 = 254.56 rounds to 255 too, which only the integer statement says for sure."""
    assert M.code(8, 3) == 240 and M.code(288, 17) == 255 and M.code(287, 17) == 254
    assert at[0] ** 2 + at[1] ** 2 == spread ** 2 and before[0] ** 2 + before[1] ** 2 == spread ** 2 - 1
    src = np.zeros((41, 41, 4), dtype=np.uint8)
    src[20, 20] = 255
    for edge in (M.TRANSPARENT, M.PAD):
        got = run_and_check(Image(renderer, src), src, spread, M.OUTSIDE, edge)
        o = spread if edge == M.TRANSPARENT else 0
        for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            assert got[20 + o + sy * at[1], 20 + o + sx * at[0], 0] == 0 and got[20 + o + sy * at[0], 20 + o + sx * at[1], 0] == 0
            assert got[20 + o + sy * before[1], 20 + o + sx * before[0], 0] == 255 - M.code(spread ** 2 - 1, spread)
    hole = 255 - src
    got = run_and_check(Image(renderer, hole), hole, spread, M.INSIDE, M.PAD)
    assert got[20 + at[1], 20 + at[0], 0] == 255 and got[20 + before[1], 20 + before[0], 0] == M.code(spread ** 2 - 1, spread)


@pytest.mark.parametrize("size", [(16384, 2), (2, 16384)], ids=["16384x2", "2x16384"])
def test_the_longest_axes(size, renderer, no_pins):
    """64 row segments, 256 column blocks, 512 row blocks: the largest indices of g and of the result. (OUTSIDE under TRANSPARENT would grow
    past 16384: that refusal is below.)"""
    src = mask(size[0], size[1], 9, 0.01)
    source = Image(renderer, src)
    for mode, edge in ((M.OUTSIDE, M.PAD), (M.OUTSIDE, M.REPEAT), (M.INSIDE, M.TRANSPARENT), (M.INSIDE, M.REFLECT)):
        run_and_check(source, src, 2, mode, edge)


def test_the_source_and_its_other_levels_are_untouched(renderer, no_pins):
    src = mask(37, 21, 8, 0.3)
    source = Image(renderer, src)
    source.generate_mipmaps()
    before = [source.download_level(level) for level in range(source.levels)]
    assert source.levels == 6 and np.array_equal(before[0], src)
    for mode, edge in itertools.product(MODES, M.EDGES):
        run_and_check(source, src, 7, mode, edge)  # only level 0 is read
    assert source.levels == 6 and all(np.array_equal(source.download_level(level), before[level]) for level in range(6))
    field = source.distance_field(7)
    field.generate_mipmaps()  # the result is an image like any other
    chain = mip_model.chain(M.distance_field(src, 7))
    assert field.levels == len(chain) and all(np.array_equal(field.download_level(level), expect) for level, expect in enumerate(chain))


def test_the_result_is_a_source_of_the_other_image_calls(renderer, no_pins):
    """A round outline: distance_field -> a table through color_filter -> composite DST_OVER at the grown origin -> Frame.load_image; and
    a chisel: the INSIDE distance lit as a height field. Every step against its model, fed the previous model's bytes."""
    w, h, spread = 96, 64, 8
    layer_bytes = np.zeros((h, w, 4), dtype=np.uint8)
    j, i = np.mgrid[0:h, 0:w]
    layer_bytes[np.hypot(i - 40, j - 30) < 17] = (200, 40, 10, 255)
    layer_bytes[20:50, 60:80] = (0, 90, 120, 180)
    layer = Image(renderer, layer_bytes)
    field = layer.distance_field(spread)
    field_model = M.distance_field(layer_bytes, spread)
    check(field, field_model, (spread, spread), "the field")
    # an outline 5 texels wide: every distance code up to c(25) becomes opaque, everything farther transparent; colours follow alpha
    tables = np.tile(np.where(np.arange(256) >= 255 - M.code(25, spread), 255, 0).astype(np.uint8), 4)
    outline = field.color_filter(None, tables)
    outline_model = FM.texels(field_model, None, tables)
    assert outline.origin == (spread, spread) and np.array_equal(outline.download_level(0), outline_model)
    assert set(np.unique(outline_model[..., 3]).tolist()) == {0, 255}
    composed = layer.composite(outline, CompositeOp.DstOver, offset=(-spread, -spread))
    composed_model = CM.composite(layer_bytes, outline_model, CM.DST_OVER, CM.NORMAL, 255, -spread, -spread)
    check(composed, composed_model, (0, 0), "the outlined layer")
    assert int((composed_model[..., 3] > 0).sum()) > int((layer_bytes[..., 3] > 0).sum())  # the outline adds coverage
    frame = R.Frame(renderer, w, h)
    frame.load_image(composed)
    assert np.array_equal(frame.download(), composed_model)
    chisel = layer.distance_field(6, DistanceMode.Inside, edge=BlurEdge.Pad)
    chisel_model = M.distance_field(layer_bytes, 6, M.INSIDE, M.A, 128, M.PAD)
    check(chisel, chisel_model, (0, 0), "the inside distance")
    lit = chisel.diffuse_lighting(DistantLight(225.0, 35.0), 4.0)
    check(lit, LM.lighting(chisel_model, LM.Light(LM.DISTANT, azimuth=225.0, elevation=35.0), LM.DIFFUSE, 4.0), (0, 0), "the chisel")
    assert np.array_equal(layer.download_level(0), layer_bytes)


def test_a_result_that_cannot_grow_is_refused_and_out_is_untouched(renderer, no_pins):
    lib = _ffi.load_library()
    out = C.c_void_p(0x1234)
    src = np.zeros((1, 16384, 4), dtype=np.uint8)
    source = Image(renderer, src)
    how = _ffi.DistanceC(0, 3, 128, 1, 0)
    assert lib.crh_image_distance_field(source.handle, C.byref(how), C.byref(out)) == _ffi.ERR_UNSUPPORTED and out.value == 0x1234
    assert lib.crh_last_error().decode() == "crh_distance_validate: a side of the grown result exceeds 16384"
    with pytest.raises(ContrastError):
        source.distance_field(1)
    with pytest.raises(ContrastError):
        source.distance_field(256, DistanceMode.Inside)
    check(source.distance_field(1, DistanceMode.Inside), M.distance_field(src, 1, M.INSIDE), (0, 0), "a good call after the refused ones")
