"""crh_image_distance_field without a GPU (include/contrast_hip.h states the rule): the numpy model of tests/distance_model.py against a
plain scalar restatement and against hand-derived answers; crh_distance_texels, crh_distance_code, crh_distance_size and the Python mirror
byte for byte against the model; every stated consequence and refusal; the mirrors; and the rule as a stand-alone program under the address
and undefined-behaviour sanitizers. Every comparison is of every byte of every texel."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, Channel, ContrastError, DistanceMode, MorphologyOp, _ffi, distance_code, distance_size, distance_texels, morphology_texels

import distance_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_distance_validate", "crh_distance_code", "crh_distance_size", "crh_distance_texels", "crh_image_distance_field")
MODES = (M.OUTSIDE, M.INSIDE)
CHANNELS = (M.R, M.A)
THRESHOLDS = (1, 128, 255)
SPREADS = (1, 2, 4, 17, 255)
SIZES = [(1, 1), (1, 40), (40, 1), (7, 5), (64, 9), (67, 33)]
KINDS = ("empty", "full", "corner", "checkerboard", "sparse")
PREFIX = "crh_distance_validate: "
INVALID, UNSUPPORTED = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def how_of(spread=4, mode=0, channel=3, threshold=128, edge=0):
    return _ffi.DistanceC(mode, channel, threshold, spread, edge)


def image_of(w, h, kind, seed=0):
    """A premultiplied (h, w, 4) uint8 image: nothing, everything, one opaque texel in a corner, a checkerboard of opaque texels, or one
    texel in seven with random codes (so that the three thresholds and the two channels make different shapes of it)"""
    rng = np.random.default_rng(seed * 1000 + w * 37 + h)
    src = np.zeros((h, w, 4), dtype=np.uint8)
    if kind == "full":
        src[:] = 255
    elif kind == "corner":
        src[(0, -1)[seed & 1], (0, -1)[(seed >> 1) & 1]] = 255
    elif kind == "checkerboard":
        j, i = np.mgrid[0:h, 0:w]
        src[(i + j) % 2 == 0] = 255
    elif kind == "sparse":
        texels = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        texels[..., :3] = np.minimum(texels[..., :3], texels[..., 3:])
        chosen = rng.random((h, w)) < 1.0 / 7.0
        src[chosen] = texels[chosen]
    return src


_models = {}


def model(src, spread, mode, channel, threshold, edge):
    """M.distance_field, once per inside map: the rule reads nothing else of the source"""
    inside = M.inside_map(src, channel, threshold)
    key = (inside.shape, inside.tobytes(), spread, mode, edge)
    if key not in _models:
        _models[key] = M.of_inside(inside, spread, mode, edge)
    return _models[key]


def library(lib, src, spread, mode, channel, threshold, edge):
    w, h = M.size(src.shape[1], src.shape[0], spread, mode, edge)
    out = np.full((h, w, 4), 0xA5, dtype=np.uint8)
    how = how_of(spread, mode, channel, threshold, edge)
    assert lib.crh_distance_texels(src.shape[1], src.shape[0], src.ctypes.data, C.byref(how), out.ctypes.data) == 0
    return out


def same(got, expect, what):
    assert got.shape == expect.shape, (what, got.shape, expect.shape)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"


# ---- a plain scalar restatement of the header's rule: a double loop over all q within the spread (Python integers)
def scalar(src, spread, mode, channel, threshold, edge):
    h, w = src.shape[:2]

    def wrap(v, n):
        if edge == M.PAD:
            return min(max(v, 0), n - 1)
        if edge == M.REPEAT:
            return v % n
        v %= 2 * n
        return v if v < n else 2 * n - 1 - v

    def inside(x, y):
        if edge == M.TRANSPARENT:
            return 0 <= x < w and 0 <= y < h and int(src[y, x, channel]) >= threshold
        return int(src[wrap(y, h), wrap(x, w), channel]) >= threshold

    o = spread if mode == M.OUTSIDE and edge == M.TRANSPARENT else 0
    out = np.zeros((h + 2 * o, w + 2 * o, 4), dtype=np.uint8)
    for j, i in itertools.product(range(h + 2 * o), range(w + 2 * o)):
        x, y = i - o, j - o
        wanted = mode == M.OUTSIDE  # the q looked for: inside ones for OUTSIDE, the others for INSIDE
        d2 = None
        if inside(x, y) == wanted:
            d2 = 0
        else:
            for dy, dx in itertools.product(range(-spread, spread + 1), repeat=2):
                if inside(x + dx, y + dy) == wanted and (d2 is None or dx * dx + dy * dy < d2):
                    d2 = dx * dx + dy * dy
        c = 255
        if d2 is not None:
            c = 0 if d2 == 0 else max(k for k in range(256) if (2 * k - 1) ** 2 * spread ** 2 <= 260100 * d2)
        out[j, i] = c if mode == M.INSIDE else 255 - c
    return out


def test_the_model_is_the_definition():
    """The scalar restatement on every texel of images of at most 7 x 5, and the answers derived by hand in the header: spread 4, OUTSIDE,
    one inside texel; D2 = 1, 2, 4, 5, 9, 16 give c = 64, 90, 128, 143, 191, 255 — 255 sqrt(D2) / 4 = 63.75, 90.16, 127.5 (a tie: it
    rounds up), 142.55, 191.25, 255 — and the bytes 191, 165, 127, 112, 64, 0."""
    assert [M.code(d2, 4) for d2 in (0, 1, 2, 4, 5, 9, 16, 17)] == [0, 64, 90, 128, 143, 191, 255, 255]
    assert (2 * 128 - 1) ** 2 * 16 <= 260100 * 4 < (2 * 129 - 1) ** 2 * 16 and 255 * 4 == 510 * 2  # the tie of D2 = 4
    src = np.zeros((9, 9, 4), dtype=np.uint8)
    src[4, 4] = (9, 9, 9, 200)
    for edge in M.EDGES:
        out = M.distance_field(src, 4, M.OUTSIDE, M.A, 128, edge)
        o = 4 if edge == M.TRANSPARENT else 0
        assert out.shape == (9 + 2 * o, 9 + 2 * o, 4)
        assert [int(out[4 + o + dy, 4 + o + dx, 2]) for dx, dy in ((0, 0), (1, 0), (1, 1), (0, -2), (-2, 1), (3, 0), (0, 4), (3, 3))] == [255, 191, 165, 127, 112, 64, 0, 0]
        assert (out[..., :1] == out).all()
    assert (M.distance_field(src, 4, M.OUTSIDE, M.R, 128, M.PAD) == 0).all()  # the stored code of R is 9: nothing is inside
    assert (M.distance_field(src, 4, M.OUTSIDE, M.R, 9, M.PAD) == M.distance_field(src, 4, M.OUTSIDE, M.A, 128, M.PAD)).all()
    # INSIDE of a 5 x 5 block under TRANSPARENT: the middle texel is 3 texels from the nearest position off the shape (off the image)
    block = np.full((5, 5, 4), 255, dtype=np.uint8)
    inner = M.distance_field(block, 4, M.INSIDE, M.A, 128, M.TRANSPARENT)
    assert inner.shape == (5, 5, 4) and inner[2, :, 0].tolist() == [64, 128, 191, 128, 64] and inner[0, 0, 0] == 64
    assert (M.distance_field(block, 4, M.INSIDE, M.A, 128, M.PAD) == 255).all()  # padded, the shape has no outside: "none"
    for n, (mode, edge) in enumerate(itertools.product(MODES, M.EDGES)):
        for (w, h), spread in (((7, 5), (1, 3, 9)[n % 3]), ((1, 1), 2), ((3, 2), 7), ((5, 1), 4)):
            for kind in ("sparse", "checkerboard", "corner"):
                src = image_of(w, h, kind, n)
                channel, threshold = CHANNELS[n % 2], THRESHOLDS[n % 3]
                assert np.array_equal(M.distance_field(src, spread, mode, channel, threshold, edge), scalar(src, spread, mode, channel, threshold, edge)), (mode, edge, w, h, spread, kind)


def test_the_codes_equal_the_integer_statement_for_every_spread(lib):
    """crh_distance_code for every D2 in [0, spread^2 + 2] and every spread: the count of the c in 1..255 whose (2 c - 1)^2 spread^2, a
    Python integer, is at most 260100 D2 (both below 2^63, compared exactly), and beside it the floating-point reading where it is no tie."""
    code = C.c_uint32(77)
    for spread in range(1, 256):
        bounds = np.array([(2 * c - 1) ** 2 * spread * spread for c in range(1, 256)], dtype=np.int64)
        d2 = np.arange(spread * spread + 3, dtype=np.int64)
        expect = np.searchsorted(bounds, 260100 * d2, side="right")
        assert expect[0] == 0 and expect[1] == M.code(1, spread) and expect[-3:].tolist() == [255, 255, 255]
        outside, inside = how_of(spread, M.OUTSIDE), how_of(spread, M.INSIDE)
        for value, c in zip(d2.tolist(), expect.tolist()):
            assert lib.crh_distance_code(C.byref(inside), value, C.byref(code)) == 0 and code.value == c, (spread, value)
        for value in (0, 1, spread * spread - 1, spread * spread):
            assert lib.crh_distance_code(C.byref(outside), value, C.byref(code)) == 0 and code.value == 255 - int(expect[value]), (spread, value)
    for spread, value in ((4, 5), (17, 288), (255, 65024), (255, 1 << 40), (1, (1 << 64) - 1)):
        assert distance_code(spread, value) == M.byte(value, spread, M.OUTSIDE) and distance_code(spread, value, DistanceMode.Inside) == M.byte(value, spread, M.INSIDE)


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("spread", SPREADS)
def test_the_library_equals_the_model(lib, spread, size):
    """Both modes, four edges, channels R and A, thresholds 1, 128 and 255, five images: every byte, and the size."""
    w, h = size
    got_w, got_h = C.c_uint32(), C.c_uint32()
    for n, (kind, mode, edge, channel, threshold) in enumerate(itertools.product(KINDS, MODES, M.EDGES, CHANNELS, THRESHOLDS)):
        src = image_of(w, h, kind, n % 4)
        expect = model(src, spread, mode, channel, threshold, edge)
        what = (size, spread, kind, mode, edge, channel, threshold)
        assert lib.crh_distance_size(w, h, C.byref(how_of(spread, mode, channel, threshold, edge)), C.byref(got_w), C.byref(got_h)) == 0
        assert (got_h.value, got_w.value) == expect.shape[:2] == M.size(w, h, spread, mode, edge)[::-1], what
        same(library(lib, src, spread, mode, channel, threshold, edge), expect, what)
        inside = M.inside_map(src, channel, threshold)
        if mode == M.OUTSIDE:  # an inside texel is 255, and the grown result holds the source at (spread, spread)
            o = spread if edge == M.TRANSPARENT else 0
            assert (expect[o:o + h, o:o + w, 0][inside] == 255).all(), what
        else:  # an inside texel is at least c(1), everything else 0
            assert (expect[..., 0][inside] >= M.code(1, spread)).all() and (expect[..., 0][~inside] == 0).all(), what


def test_the_python_mirror(lib):
    src = image_of(12, 7, "sparse", 3)
    assert np.array_equal(distance_texels(src, 5), M.distance_field(src, 5))  # the defaults: OUTSIDE of alpha >= 128, transparent outside, grown
    assert distance_texels(src, 5).shape == (17, 22, 4) and distance_size(12, 7, 5) == (22, 17) and distance_size(12, 7, 5, DistanceMode.Inside) == (12, 7)
    assert distance_size(12, 7, 5, edge=BlurEdge.Reflect) == (12, 7)
    got = distance_texels(src, 9, DistanceMode.Inside, Channel.R, 1, BlurEdge.Repeat)
    assert np.array_equal(got, M.distance_field(src, 9, M.INSIDE, M.R, 1, M.REPEAT))
    assert np.array_equal(distance_texels(src[:, ::2], 3), M.distance_field(np.ascontiguousarray(src[:, ::2]), 3))  # a strided view
    for bad in (dict(spread=0), dict(spread=256), dict(spread=2, mode=2), dict(spread=2, channel=4), dict(spread=2, threshold=0), dict(spread=2, threshold=256), dict(spread=2, edge=4)):
        with pytest.raises(ContrastError):
            distance_texels(src, **bad)
        with pytest.raises(ContrastError):
            distance_size(12, 7, **bad)
    with pytest.raises(ContrastError):
        distance_texels(src.astype(np.float32), 2)
    with pytest.raises(ContrastError):
        distance_size(16384, 2, 1)
    with pytest.raises(ContrastError):
        distance_code(0, 1)
    assert [m.value for m in DistanceMode] == [0, 1]


def test_inside_is_the_complement_of_outside_under_the_same_size_edges(lib):
    """INSIDE of an image = 255 - OUTSIDE of its complement (code -> 255 - code, threshold t -> 256 - t: code >= t iff not 255 - code >= 256 - t)."""
    for (w, h), spread, edge, threshold, channel in itertools.product(((7, 5), (64, 9), (1, 40)), (1, 4, 17, 255), (M.PAD, M.REPEAT, M.REFLECT), THRESHOLDS, CHANNELS):
        src = image_of(w, h, "sparse", spread)
        inside = library(lib, src, spread, M.INSIDE, channel, threshold, edge)
        outside = library(lib, 255 - src, spread, M.OUTSIDE, channel, 256 - threshold, edge)
        assert np.array_equal(inside, 255 - outside), (w, h, spread, edge, threshold, channel)


def test_the_transpose_of_the_result_is_the_result_of_the_transpose(lib):
    for (w, h), spread, mode, edge in itertools.product(((7, 5), (64, 9), (1, 40), (67, 33)), (2, 17, 255), MODES, M.EDGES):
        src = image_of(w, h, "sparse", 2)
        turned = np.ascontiguousarray(src.transpose(1, 0, 2))
        assert np.array_equal(library(lib, src, spread, mode, M.A, 128, edge).transpose(1, 0, 2), library(lib, turned, spread, mode, M.A, 128, edge)), (w, h, spread, mode, edge)


def test_under_repeat_a_roll_of_the_source_rolls_the_result(lib):
    for (w, h), spread, mode, (dx, dy) in itertools.product(((7, 5), (64, 9), (40, 1)), (1, 4, 255), MODES, ((1, 0), (-3, 2), (100, -77))):
        src = image_of(w, h, "sparse", 5)
        rolled = np.ascontiguousarray(np.roll(src, (dy, dx), axis=(0, 1)))
        assert np.array_equal(library(lib, rolled, spread, mode, M.A, 1, M.REPEAT), np.roll(library(lib, src, spread, mode, M.A, 1, M.REPEAT), (dy, dx), axis=(0, 1))), (w, h, spread, mode, dx, dy)


def test_neighbouring_bytes_differ_by_at_most_the_code_of_one_texel_and_one(lib):
    """|d(p) - d(p')| <= 1 for neighbours, and c rounds 255 d / spread once: |c - c'| <= c(1) + 1."""
    for (w, h), spread, mode, edge, kind in itertools.product(((7, 5), (64, 9), (67, 33)), SPREADS, MODES, M.EDGES, ("sparse", "checkerboard", "corner")):
        out = library(lib, image_of(w, h, kind, 1), spread, mode, M.A, 128, edge)[..., 0].astype(int)
        bound = M.code(1, spread) + 1
        assert np.abs(np.diff(out, axis=0)).max(initial=0) <= bound and np.abs(np.diff(out, axis=1)).max(initial=0) <= bound, (w, h, spread, mode, edge, kind)


def test_the_level_sets_lie_between_morphology_s_squares_and_are_its_line_on_one_row(lib):
    """On a binarised image under PAD, {v >= 255 - c(r^2)} lies within dilate(r, r), contains dilate(k, k) for 2 k^2 <= r^2, and on a
    one-row image (whose padded rows are all the same, so D2 = dx^2) equals dilate(r, 0)."""
    for (w, h), spread, r in itertools.product(((67, 33), (64, 9), (40, 1), (1, 40)), (17, 255), (1, 2, 5, 10, 16)):
        src = image_of(w, h, "sparse", 4)
        src[...] = np.where(src[..., 3:] >= 128, 255, 0)
        field = library(lib, src, spread, M.OUTSIDE, M.A, 128, M.PAD)[..., 0]
        level = field >= 255 - M.code(r * r, spread)

        def dilated(rx, ry):
            return morphology_texels(src, MorphologyOp.Dilate, rx, ry, BlurEdge.Pad)[..., 3] == 255

        assert not (level & ~dilated(r, r)).any(), (w, h, spread, r)
        k = max(k for k in range(r + 1) if 2 * k * k <= r * r)
        assert not (dilated(k, k) & ~level).any(), (w, h, spread, r, k)
        if h == 1:
            assert np.array_equal(level, dilated(r, 0)), (w, spread, r)


class ImageHead(C.Structure):
    """What a crh_image starts with: its renderer and its size. Enough for the calls below, which refuse before they look at the texels or
    at the renderer behind the pointer (0x10 is never followed)."""
    _fields_ = [("renderer", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("pixels", C.c_void_p * 2)]


def test_refusals_statuses_texts_and_untouched_outputs(lib):
    mode, channel, threshold = "mode is above CRH_DISTANCE_INSIDE", "channel is above CRH_CHANNEL_A", "threshold is outside [1, 255]"
    spread, edge, a_size = "spread is outside [1, CRH_MAX_DISTANCE_SPREAD]", "edge is above CRH_BLUR_EDGE_REFLECT", "width and height lie in [1, 16384]"
    grown, null = "a side of the grown result exceeds 16384", PREFIX + "a null argument"
    cases = ((how_of(mode=2), mode), (how_of(channel=4), channel), (how_of(threshold=0), threshold), (how_of(threshold=256), threshold), (how_of(spread=0), spread),
             (how_of(spread=256), spread), (how_of(edge=4), edge),
             # the order: the mode before the channel before the threshold before the spread before the edge
             (how_of(mode=9, channel=9, threshold=0, spread=0, edge=9), mode), (how_of(channel=9, threshold=0, spread=0, edge=9), channel),
             (how_of(threshold=999, spread=0, edge=9), threshold), (how_of(spread=999, edge=9), spread))
    src = image_of(5, 3, "sparse")
    out = np.full((3 + 8, 5 + 8, 4), 0xA5, dtype=np.uint8)
    code, w, h, handle = C.c_uint32(77), C.c_uint32(7), C.c_uint32(9), C.c_void_p(0x1234)
    heads = [ImageHead(0x10, 5, 3), ImageHead(0x10, 16384, 1), ImageHead(0x10, 1, 16384 - 2 * 4 + 1), ImageHead(None, 5, 3), ImageHead(0x10, 0, 3)]
    fake, wide, tall, unowned, flat = (C.addressof(head) for head in heads)

    def untouched():
        return (out == 0xA5).all() and (code.value, w.value, h.value, handle.value) == (77, 7, 9, 0x1234)

    for how, text in cases:
        for call in (lambda: lib.crh_distance_validate(C.byref(how)), lambda: lib.crh_distance_code(C.byref(how), 5, C.byref(code)),
                     lambda: lib.crh_distance_size(5, 3, C.byref(how), C.byref(w), C.byref(h)), lambda: lib.crh_distance_texels(5, 3, src.ctypes.data, C.byref(how), out.ctypes.data),
                     # a size outside the range, an output that is the input and an image too large to grow beside it: the field is named
                     lambda: lib.crh_distance_texels(0, 3, src.ctypes.data, C.byref(how), src.ctypes.data), lambda: lib.crh_distance_size(16385, 0, C.byref(how), C.byref(w), C.byref(h)),
                     # (a refused crh_image_distance_field does not touch the device: the image is not looked at before the fields)
                     lambda: lib.crh_image_distance_field(fake, C.byref(how), C.byref(handle)), lambda: lib.crh_image_distance_field(wide, C.byref(how), C.byref(handle))):
            assert lib.crh_blur_taps(-1.0, None, 0, None) == INVALID  # some other text first
            assert call() == INVALID and lib.crh_last_error().decode() == PREFIX + text and untouched(), text
    good = how_of()
    assert lib.crh_distance_validate(C.byref(good)) == 0
    for call in (lambda: lib.crh_distance_validate(None), lambda: lib.crh_distance_code(None, 5, C.byref(code)), lambda: lib.crh_distance_code(C.byref(good), 5, None),
                 lambda: lib.crh_distance_size(5, 3, None, C.byref(w), C.byref(h)), lambda: lib.crh_distance_size(5, 3, C.byref(good), None, C.byref(h)),
                 lambda: lib.crh_distance_size(5, 3, C.byref(good), C.byref(w), None), lambda: lib.crh_distance_texels(5, 3, None, C.byref(good), out.ctypes.data),
                 lambda: lib.crh_distance_texels(5, 3, src.ctypes.data, None, out.ctypes.data), lambda: lib.crh_distance_texels(5, 3, src.ctypes.data, C.byref(good), None),
                 # a null beside a bad field, and beside a bad size: the null is named
                 lambda: lib.crh_distance_texels(0, 3, None, C.byref(how_of(edge=9)), out.ctypes.data), lambda: lib.crh_distance_size(0, 3, C.byref(how_of(mode=9)), None, None),
                 # crh_image_distance_field with a null source, a null `how`, a null `out`, and a source without a renderer
                 lambda: lib.crh_image_distance_field(None, C.byref(good), C.byref(handle)), lambda: lib.crh_image_distance_field(fake, None, C.byref(handle)),
                 lambda: lib.crh_image_distance_field(fake, C.byref(good), None), lambda: lib.crh_image_distance_field(unowned, C.byref(good), C.byref(handle)),
                 lambda: lib.crh_image_distance_field(None, C.byref(how_of(spread=0)), None)):
        assert lib.crh_blur_taps(-1.0, None, 0, None) == INVALID
        assert call() == INVALID and lib.crh_last_error().decode() == null and untouched()
    # a bad field beside a source without a renderer: the field is named
    assert lib.crh_image_distance_field(unowned, C.byref(how_of(threshold=0)), C.byref(handle)) == INVALID and lib.crh_last_error().decode() == PREFIX + threshold
    for width, height in ((0, 3), (5, 0), (16385, 1), (1, 16385)):
        assert lib.crh_distance_texels(width, height, src.ctypes.data, C.byref(good), out.ctypes.data) == INVALID and lib.crh_last_error().decode() == PREFIX + a_size and untouched()
        assert lib.crh_distance_size(width, height, C.byref(good), C.byref(w), C.byref(h)) == INVALID and lib.crh_last_error().decode() == PREFIX + a_size and untouched()
        # a size outside the range and an output that is the input: the size is named
        assert lib.crh_distance_texels(width, height, src.ctypes.data, C.byref(good), src.ctypes.data) == INVALID and lib.crh_last_error().decode() == PREFIX + a_size
    assert lib.crh_image_distance_field(flat, C.byref(good), C.byref(handle)) == INVALID and lib.crh_last_error().decode() == PREFIX + a_size and untouched()
    before = src.copy()
    assert lib.crh_distance_texels(5, 3, src.ctypes.data, C.byref(good), src.ctypes.data) == INVALID and lib.crh_last_error().decode() == PREFIX + "out_rgba8 is rgba8"
    assert np.array_equal(src, before)
    # the growing size above 16384: OUTSIDE under TRANSPARENT alone, CRH_ERR_UNSUPPORTED, from 16384 - 2 spread + 1 on
    for how, (width, height), refused in ((good, (16384, 1), True), (good, (1, 16377), True), (good, (16376, 16376), False), (how_of(255), (15875, 1), True), (how_of(255), (15874, 15874), False),
                                          (how_of(mode=1), (16384, 16384), False), (how_of(edge=1), (16384, 16384), False), (how_of(255, edge=3), (16384, 1), False)):
        status = lib.crh_distance_size(width, height, C.byref(how), C.byref(w), C.byref(h))
        if refused:
            assert status == UNSUPPORTED and lib.crh_last_error().decode() == PREFIX + grown and untouched(), (width, height)
            assert lib.crh_distance_texels(width, height, src.ctypes.data, C.byref(how), out.ctypes.data) == UNSUPPORTED and lib.crh_last_error().decode() == PREFIX + grown and untouched()
            # the output that is the input is named before the size that cannot grow
            assert lib.crh_distance_texels(width, height, src.ctypes.data, C.byref(how), src.ctypes.data) == INVALID and lib.crh_last_error().decode() == PREFIX + "out_rgba8 is rgba8"
        else:
            grow = 2 * how.spread if how.mode == 0 and how.edge == 0 else 0
            assert status == 0 and (w.value, h.value) == (width + grow, height + grow), (width, height)
            w.value, h.value = 7, 9
    for image in (wide, tall):
        assert lib.crh_image_distance_field(image, C.byref(good), C.byref(handle)) == UNSUPPORTED and lib.crh_last_error().decode() == PREFIX + grown and untouched()
    # the limits themselves are served
    small = np.full((3 + 510, 5 + 510, 4), 0xA5, dtype=np.uint8)
    for how in (how_of(255, 1, 3, 255, 3), how_of(1, 0, 0, 1, 0), how_of(255, 0, 0, 1, 0)):
        assert lib.crh_distance_validate(C.byref(how)) == 0 and lib.crh_distance_texels(5, 3, src.ctypes.data, C.byref(how), small.ctypes.data) == 0


def test_unaligned_bytes(lib):
    src = image_of(7, 3, "sparse", 6)
    raw_in = np.full(7 * 3 * 4 + 3, 0xA5, dtype=np.uint8)
    raw_in[1:-2] = src.reshape(-1)
    for mode, edge in itertools.product(MODES, M.EDGES):
        expect = M.distance_field(src, 2, mode, M.A, 1, edge)
        raw_out = np.full(expect.size + 3, 0xA5, dtype=np.uint8)
        assert lib.crh_distance_texels(7, 3, raw_in.ctypes.data + 1, C.byref(how_of(2, mode, 3, 1, edge)), raw_out.ctypes.data + 2) == 0
        assert np.array_equal(raw_out[2:-1].reshape(expect.shape), expect) and (raw_out[:2] == 0xA5).all() and raw_out[-1] == 0xA5


def test_the_library_exports_and_the_mirrors_agree_across_header_python_and_ffi_rs(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    exports = open(b.write_export_map()).read()
    for name in NAMES:
        assert f"    {name};\n" in exports
    assert any(os.path.basename(h) == "distance.hpp" for h in b.header_deps())
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    assert "CRH_DISTANCE_OUTSIDE = 0, CRH_DISTANCE_INSIDE = 1" in header and "#define CRH_MAX_DISTANCE_SPREAD 255u" in header
    assert "crh_image_distance_field under a table of crh_image_color_filter" in header  # morphology's "no disc" points here
    assert C.sizeof(_ffi.DistanceC) == 5 * 4 and [name for name, _ in _ffi.DistanceC._fields_] == ["mode", "channel", "threshold", "spread", "edge"]
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    assert committed == fresh
    for text in ("pub fn crh_distance_validate(how: *const crh_distance) -> crh_status;",
                 "pub fn crh_distance_code(how: *const crh_distance, squared_distance: u64, code: *mut u32) -> crh_status;",
                 "pub fn crh_distance_size(width: u32, height: u32, how: *const crh_distance, out_width: *mut u32, out_height: *mut u32) -> crh_status;",
                 "pub fn crh_distance_texels(width: u32, height: u32, rgba8: *const c_void, how: *const crh_distance, out_rgba8: *mut c_void) -> crh_status;",
                 "pub fn crh_image_distance_field(src: *const crh_image, how: *const crh_distance, out: *mut *mut crh_image) -> crh_status;",
                 "pub const CRH_DISTANCE_INSIDE: u32 = 1;", "pub const CRH_MAX_DISTANCE_SPREAD: usize = 255;",
                 "pub struct crh_distance {\n    pub mode: u32,\n    pub channel: u32,\n    pub threshold: u32,\n    pub spread: u32,\n    pub edge: u32,\n}"):
        assert text in committed, text
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub enum DistanceMode {", "pub struct Distance {", "pub fn distance_validate(distance: &Distance) -> Result<(), Error>",
                 "pub fn distance_code(distance: &Distance, squared_distance: u64) -> Result<u32, Error>",
                 "pub fn distance_size(width: u32, height: u32, distance: &Distance) -> Result<(u32, u32), Error>",
                 "pub fn distance_texels(width: u32, height: u32, texels: &[u8], distance: &Distance) -> Result<(u32, u32, Vec<u8>), Error>",
                 "pub fn distance_field(&self, distance: &Distance) -> Result<Image, Error>"):
        assert text in shim, text
    for name in NAMES:
        assert f"ffi::{name}(" in shim, name
    mirror = open(os.path.join(ROOT, "include", "contrast_renderer.hpp")).read()
    for text in ("enum class DistanceMode : uint32_t {", "struct Distance {", "Image distance_field(const Distance& distance) const",
                 "inline std::vector<uint8_t> distance_texels(uint32_t width, uint32_t height,", "inline std::array<uint32_t, 2> distance_size(uint32_t width, uint32_t height, const Distance& distance)",
                 "inline uint32_t distance_code(const Distance& distance, uint64_t squared_distance)"):
        assert text in mirror, text
    import contrast_renderer_amd
    for name in ("DistanceMode", "distance_texels", "distance_size", "distance_code"):
        assert name in contrast_renderer_amd.__all__ and hasattr(contrast_renderer_amd, name)
    assert hasattr(contrast_renderer_amd.Image, "distance_field")


def test_the_cpp_mirror_of_the_distance_field_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "distance_harness.cpp"),
               "-o", os.path.join(tmp, "distance_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """A stand-alone program (its own main, no library, nothing loaded into python) around csrc/distance.hpp, the rule that
    crh_distance_texels runs: compiled as host code with the two sanitizers (the flag goes to the host compilation alone) and run once. It
    sweeps spread 255 on 1 x 1 and 3 x 2 images under every edge, wraps many periods out, in heap buffers sized exactly."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        binary = os.path.join(tmp, "distance_sanitize")
        # -x c++ and -Xarch_host: plain host C++, the sanitizers on the host alone (no device pass; clang links the sanitizers' runtime statically, so the program needs nothing preloaded)
        cmd = [hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
               "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), "-I", os.path.join(ROOT, "contrast_renderer_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "distance_sanitize.cpp"), "-o", binary]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert re.search(r"\d+ texels, 0 failures$", done.stdout.strip())
