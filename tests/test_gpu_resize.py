"""crh_image_resize (include/contrast_hip.h) on the GPU: k_image_resize_h and k_image_resize_v byte for byte against the numpy model of
tests/resize_model.py, with no tolerance and no excluded texel, at the smallest shapes where the kernels can go wrong — widths round a
wave, the horizontal kernel's group of output columns and its chunk of staged source columns, heights round its 64-row tile and the
vertical kernel's row block, one texel on either side of the call, odd and even windows at both image ends, prime ratios in both
directions at once, the longest windows, the input that binds every clamp, colours above their alpha, where min(v, alpha) binds on most
texels — and the result as a source of the other image calls."""
import ctypes as C
import itertools

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, CompositeOp, ContrastError, ResizeFilter, _ffi, resize_texels
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image

import blur_model as BM
import composite_model as CM
import layers_model
import mip_model
import resize_model as M
from test_gpu_blending import no_pins  # noqa: F401

pytestmark = pytest.mark.gpu

# k_image_resize_h: a workgroup owns 32 output columns (8 per wave) of 64 rows and stages 64 source columns at a time; k_image_resize_v: 64
# columns by 32 output rows (kResizeGroup, kResizeRows, kResizeChunk, kResizeColumns and kResizeBlockRows in csrc/image_filter.hip).
GROUP, TILE_ROWS, CHUNK, COLUMNS, BLOCK_ROWS = 32, 64, 64, 64, 32


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


def check(image, expect, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == (0, 0) and image.levels == 1, (what, image.width, image.height, image.origin)
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"
    return got


def run_and_check(source, src, width, height, filter, counters=None):
    return check(source.resize(width, height, ResizeFilter(filter)), M.resize(src, width, height, filter, counters), (src.shape, width, height, M.NAMES[filter]))


@pytest.mark.parametrize("src_w", (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1))
def test_widths_round_a_wave_a_group_and_a_chunk(src_w, renderer, no_pins):
    """Height 3. Result widths round the group of 32 output columns and a wave of 64, source widths round one and two chunks of 64 staged
    columns: up and down, spans of one, two and three chunks."""
    src = M.premultiplied(np.random.default_rng(src_w), 3, src_w)
    source = Image(renderer, src)
    for width, filter in itertools.product((GROUP - 1, GROUP, GROUP + 1, COLUMNS - 1, COLUMNS, COLUMNS + 1), M.FILTERS):
        run_and_check(source, src, width, 2, filter)
    assert np.array_equal(source.download_level(0), src)


@pytest.mark.parametrize("src_h", (TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1))
def test_heights_round_the_row_tile_and_the_row_block(src_h, renderer, no_pins):
    """Width 5. Source heights round the horizontal kernel's tile of 64 rows, result heights the vertical kernel's block of 32 rows and
    its four waves."""
    src = M.premultiplied(np.random.default_rng(100 + src_h), src_h, 5)
    source = Image(renderer, src)
    for height, filter in itertools.product((3, 4, 5, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 2 * TILE_ROWS + 1), M.FILTERS):
        run_and_check(source, src, 4, height, filter)


@pytest.mark.parametrize("filter", M.FILTERS, ids=list(M.NAMES.values()))
def test_one_texel_on_either_side(filter, renderer, no_pins):
    """1 x 1 to 1 x 1, 1 x 1 to 300 x 200 and 300 x 200 to 1 x 1: a window of one texel for every output, and one window that is the whole
    source on both axes (300 and 200 taps: clipped by the source, so inside the cap under every filter)."""
    one = np.array([[[10, 20, 30, 200]]], dtype=np.uint8)
    source = Image(renderer, one)
    assert np.array_equal(run_and_check(source, one, 1, 1, filter), one)
    got = run_and_check(source, one, 300, 200, filter)
    assert (got == one[0, 0]).all()
    src = M.premultiplied(np.random.default_rng(7), 200, 300)
    run_and_check(Image(renderer, src), src, 1, 1, filter)


@pytest.mark.parametrize("filter", M.FILTERS, ids=list(M.NAMES.values()))
def test_odd_and_even_windows_at_both_ends(filter, renderer, no_pins):
    """Every pair of small sizes, both axes: windows of odd and even counts that start on odd and even indices (the zero tap that pads a
    pair, in front and behind), clipped at index 0 and at the last index of an odd and of an even axis."""
    rng = np.random.default_rng(11)
    sizes = (1, 2, 3, 4, 5, 7, 8)
    for n, m in itertools.product(sizes, sizes):
        src = M.premultiplied(rng, m, n)  # n x m texels
        run_and_check(Image(renderer, src), src, m, n, filter)  # -> m x n: the two axes take the pair in both directions


@pytest.mark.parametrize("filter", M.FILTERS, ids=list(M.NAMES.values()))
def test_prime_ratios_up_on_one_axis_and_down_on_the_other(filter, renderer, no_pins):
    """211 x 97 to 97 x 211 and back (ratios 211 / 97 and 97 / 211 at once), and 300 x 200 to 111 x 74: several groups, tiles and blocks."""
    src = M.premultiplied(np.random.default_rng(13), 97, 211)
    source = Image(renderer, src)
    got = run_and_check(source, src, 97, 211, filter)
    assert np.array_equal(got, resize_texels(src, 97, 211, ResizeFilter(filter)))  # the host function runs the same rule
    tall = np.ascontiguousarray(src.transpose(1, 0, 2))
    run_and_check(Image(renderer, tall), tall, 211, 97, filter)
    big = M.saturated(np.random.default_rng(14), 200, 300)
    run_and_check(Image(renderer, big), big, 111, 74, filter)


@pytest.mark.parametrize("transpose", (False, True), ids=["16384x2", "2x16384"])
def test_the_longest_windows(transpose, renderer, no_pins):
    """16384 x 2 to 33 x 2 under BOX (498 taps, the fewest outputs 16384 texels can go to) and to 193 x 2 under LANCZOS3 (511 taps, of both
    signs), and the transposes: the horizontal kernel's accumulators live across nine chunks, the vertical kernel's loop runs 256 pairs."""
    assert M.max_count(16384, 33, M.BOX) == 498 and M.max_count(16384, 193, M.LANCZOS3) == 511
    src = M.premultiplied(np.random.default_rng(15), 2, 16384)
    if transpose:
        src = np.ascontiguousarray(src.transpose(1, 0, 2))
    source = Image(renderer, src)
    for m, filter in ((33, M.BOX), (193, M.LANCZOS3)):
        run_and_check(source, src, *((2, m) if transpose else (m, 2)), filter)
    with pytest.raises(ContrastError) as refused:
        source.resize(*((2, 32) if transpose else (32, 2)), ResizeFilter.Box)  # 513 taps
    assert refused.value.status == _ffi.ERR_UNSUPPORTED


def test_the_checker_binds_every_clamp(renderer, no_pins):
    """8 x 5 to 21 x 13: under the three filters with negative lobes both clamps of both passes bind (the model counts them), under BOX and
    TRIANGLE none does."""
    src = M.checker(5, 8)
    source = Image(renderer, src)
    for filter in M.FILTERS:
        counters = {}
        run_and_check(source, src, 21, 13, filter, counters)
        clamps = [counters[k] for k in ("h_low", "h_high", "v_low", "v_high")]
        assert all(clamps) if filter in (M.CATMULL_ROM, M.MITCHELL, M.LANCZOS3) else not any(clamps), (M.NAMES[filter], counters)
    src = M.premultiplied(np.random.default_rng(2), 6, 11)
    for filter in (M.CATMULL_ROM, M.LANCZOS3):
        counters = {}
        run_and_check(Image(renderer, src), src, 5, 4, filter, counters)
        assert counters["min_alpha"] > 0, (M.NAMES[filter], counters)  # min(v, alpha) lowers a colour


def test_straight_sources_where_min_alpha_binds_on_most_texels(renderer, no_pins):
    """Colours above their alpha (alpha 0 .. 199, R above it everywhere): resize_texel's min(v, alpha) lowers a colour on most texels, not
    only where a filter overshoots; to the source's own size, up on one axis and down on the other both ways, under every filter. The
    result is premultiplied whatever the source was."""
    src = layers_model.random_texels(np.random.RandomState(23), "straight", 70, 37)
    assert not layers_model.premultiplied(src)
    source = Image(renderer, src)
    for filter, (width, height) in itertools.product(M.FILTERS, ((70, 37), (13, 90), (150, 5))):
        counters = {}
        got = run_and_check(source, src, width, height, filter, counters)
        assert counters["min_alpha"] > 0, (M.NAMES[filter], width, height, counters)
        assert layers_model.premultiplied(got), (M.NAMES[filter], width, height)
    assert np.array_equal(source.download_level(0), src)


def test_constants_and_copies(renderer, no_pins):
    flat = np.full((37, 70, 4), (7, 99, 180, 201), dtype=np.uint8)
    src = M.premultiplied(np.random.default_rng(17), 37, 70)
    for filter in M.FILTERS:
        for width, height in ((70, 37), (13, 90), (150, 5)):
            assert (run_and_check(Image(renderer, flat), flat, width, height, filter) == flat[0, 0]).all()
        got = run_and_check(Image(renderer, src), src, 70, 37, filter)
        assert np.array_equal(got, src) == (filter != M.MITCHELL)


def test_the_source_is_untouched_and_the_result_feeds_the_other_image_calls(renderer, no_pins):
    """Only level 0 is read; the result takes generate_mipmaps, blur and composite, each against its sibling's model on the model's bytes."""
    src = M.premultiplied(np.random.default_rng(19), 45, 83)
    source = Image(renderer, src)
    source.generate_mipmaps()
    before = [source.download_level(level) for level in range(source.levels)]
    small = source.resize(31, 17, ResizeFilter.Lanczos3)
    small_model = M.resize(src, 31, 17, M.LANCZOS3)
    check(small, small_model, "the thumbnail")
    assert all(np.array_equal(source.download_level(level), before[level]) for level in range(source.levels))
    small.generate_mipmaps()
    chain = mip_model.chain(small_model)
    assert small.levels == len(chain) and all(np.array_equal(small.download_level(level), expect) for level, expect in enumerate(chain))
    soft = small.blur(1.5, edge=BlurEdge.Pad)
    soft_model = BM.blur_sigma(small_model, 1.5, 1.5, BM.PAD)
    assert np.array_equal(soft.download_level(0), soft_model)
    back = soft.resize(83, 45, ResizeFilter.Triangle)  # the half-resolution blur: down, blur, up
    back_model = M.resize(soft_model, 83, 45, M.TRIANGLE)
    check(back, back_model, "the blur brought back up")
    composed = source.composite(back, CompositeOp.SrcOver, opacity=0.5)
    assert np.array_equal(composed.download_level(0), CM.composite(src, back_model, CM.SRC_OVER, CM.NORMAL, 128, 0, 0))


def test_refusals_on_a_live_renderer_leave_nothing_behind(renderer, no_pins):
    lib = _ffi.load_library()
    out = C.c_void_p(0x1234)
    src = M.premultiplied(np.random.default_rng(21), 2, 2000)
    source = Image(renderer, src)
    for width, height, filter, status, text in ((0, 1, 4, _ffi.ERR_INVALID_ARGUMENT, "width and height lie in [1, 16384]"),
                                                (1, 16385, 4, _ffi.ERR_INVALID_ARGUMENT, "width and height lie in [1, 16384]"),
                                                (5, 5, 5, _ffi.ERR_INVALID_ARGUMENT, "filter is above CRH_RESIZE_LANCZOS3"),
                                                (5, 2, 4, _ffi.ERR_UNSUPPORTED, "an output's window exceeds CRH_MAX_RESIZE_TAPS texels: chain two calls")):
        assert lib.crh_image_resize(source.handle, width, height, filter, C.byref(out)) == status and out.value == 0x1234, (width, height, filter)
        assert lib.crh_last_error().decode() == "crh_resize_taps: " + text
    assert lib.crh_image_resize(None, 5, 5, 0, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_resize(source.handle, 5, 5, 0, None) == _ffi.ERR_INVALID_ARGUMENT
    with pytest.raises(ContrastError):
        source.resize(5, 2)
    run_and_check(source, src, 24, 2, M.LANCZOS3)  # a good call after the refused ones (2000 / 24: 501 taps)
