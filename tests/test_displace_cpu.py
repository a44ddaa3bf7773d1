"""crh_image_displace without a GPU (include/contrast_hip.h states the rule): the numpy model of tests/displace_model.py against a plain
scalar restatement and against known answers; crh_displace_offset, crh_displace_texels and the Python mirror byte for byte against the
model; every stated consequence and refusal; the mirrors; and the rule as a stand-alone program under the address and undefined-behaviour
sanitizers. Every comparison is of every byte of every texel."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, Channel, CompositeOp, ContrastError, Filter, _ffi, composite_texels, displace_offset, displace_texels

import displace_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_displace_validate", "crh_displace_offset", "crh_displace_texels", "crh_image_displace")
SIZES = [(1, 1), (1, 7), (7, 1), (33, 15), (64, 17)]
FILTERS = (M.NEAREST, M.LINEAR)
PAIRS = ((M.R, M.G), (M.A, M.A), (M.B, M.R), (M.G, M.A))
SCALES = ((0.0, 0.0), (0.0, 37.5), (-20.0, 20.0), (7.77, -0.3), (510.0, 510.0), (1024.0, -1024.0))
PREFIX = "crh_displace_validate: "


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def how_of(scale=(3.0, -4.5), x_channel=0, y_channel=1, filter=1, edge=0):
    how = _ffi.DisplaceC()
    how.scale = (C.c_float * 2)(*scale)
    how.x_channel, how.y_channel, how.filter, how.edge = x_channel, y_channel, filter, edge
    return how


def images(w, h, seed, kind="random"):
    """(source, map): a premultiplied source; a map that is random and premultiplied, transparent (a = 0, colours kept, so the load clamp
    gives u = 0), or not premultiplied (colours above alpha: the load clamp acts)"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    src[..., :3] = np.minimum(src[..., :3], src[..., 3:])
    map = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if kind == "random":
        map[..., :3] = np.minimum(map[..., :3], map[..., 3:])
    elif kind == "transparent":
        map[..., 3] = 0
    elif kind == "partly":
        map[..., :3] = np.minimum(map[..., :3], map[..., 3:])
        map[rng.random((h, w)) < 0.3] = 0
    return src, map


def library(lib, src, map, scale, x_channel, y_channel, filter, edge):
    out = np.full(src.shape, 0xA5, dtype=np.uint8)
    how = how_of(scale, x_channel, y_channel, filter, edge)
    assert lib.crh_displace_texels(src.shape[1], src.shape[0], src.ctypes.data, map.ctypes.data, C.byref(how), out.ctypes.data) == 0
    return out


def same(got, expect, what):
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"


# ---- a plain scalar restatement of the header's rule (Python integers; // is the true floor, >> the arithmetic shift)
def scalar_texel(src, map, i, j, scale, x_channel, y_channel, filter, edge):
    h, w = src.shape[:2]

    def code(channel):
        r, g, b, a = (int(v) for v in map[j, i])
        if channel == 3:
            return a
        c = min((r, g, b)[channel], a)
        return 0 if a == 0 else (255 * c + a // 2) // a

    def q(s, u):
        k = int(np.floor(np.float64(np.float32(s)) * 256 + 0.5))
        return (k * (2 * u - 255) + 255) // 510

    def wrap(v, n):
        if edge == M.PAD:
            return min(max(v, 0), n - 1)
        if edge == M.REPEAT:
            return v % n
        v %= 2 * n
        return v if v < n else 2 * n - 1 - v

    def S(x, y):
        if edge == M.TRANSPARENT:
            return [0, 0, 0, 0] if not (0 <= x < w and 0 <= y < h) else [int(v) for v in src[y, x]]
        return [int(v) for v in src[wrap(y, h), wrap(x, w)]]

    X, Y = 256 * i + 128 + q(scale[0], code(x_channel)), 256 * j + 128 + q(scale[1], code(y_channel))
    if filter == M.NEAREST:
        return S(X >> 8, Y >> 8)
    ax, ay = X - 128, Y - 128
    i0, j0, fx, fy = ax >> 8, ay >> 8, ax & 255, ay & 255
    out = []
    for c in range(4):
        top = S(i0, j0)[c] * (256 - fx) + S(i0 + 1, j0)[c] * fx
        bottom = S(i0, j0 + 1)[c] * (256 - fx) + S(i0 + 1, j0 + 1)[c] * fx
        out.append((top * (256 - fy) + bottom * fy + 32768) >> 16)
    return out


def test_the_model_is_the_definition():
    """The scalar restatement on every texel of a few calls of every kind, and known answers worked out by hand.

    One LINEAR texel by hand: a 2 x 1 source with texels (10, 20, 30, 40) and (50, 60, 70, 80), scale (1, 0), both channels A, the map's
    alpha 255 at texel 0. K = 256, n = 256 * 255 = 65280, q = floor(65535 / 510) = 128: half a texel to the right. X = 128 + 128 = 256,
    ax = 128, i0 = 0, fx = 128; Y = 128, ay = 0, j0 = 0, fy = 0. top = s0 * 128 + s1 * 128, so per channel 128 * (10 + 50) = 7680,
    128 * 80 = 10240, 12800, 15360; the value is (top * 256 + 32768) >> 16 = (top + 128) >> 8 = 30, 40, 50, 60: the mean of the two.
    Under TRANSPARENT texel 1 (alpha 0 in the map, u = 0, q = floor((-65280 + 255) / 510) = floor(-127.5) = -128) reads X = 256 + 128 - 128
    = 256 too and gives the same mean."""
    src = np.array([[[10, 20, 30, 40], [50, 60, 70, 80]]], dtype=np.uint8)
    map = np.array([[[0, 0, 0, 255], [0, 0, 0, 0]]], dtype=np.uint8)
    assert M.offsets(256, 255) == 128 and M.offsets(256, 0) == -128
    assert M.displace(src, map, (1.0, 0.0), M.A, M.A, M.LINEAR, M.TRANSPARENT).tolist() == [[[30, 40, 50, 60], [30, 40, 50, 60]]]
    # NEAREST takes the texel that holds X = 256: texel 1
    assert M.displace(src, map, (1.0, 0.0), M.A, M.A, M.NEAREST, M.TRANSPARENT).tolist() == [[[50, 60, 70, 80], [50, 60, 70, 80]]]
    # scale 0: q = floor(255 / 510) = 0 for every code
    assert (M.offsets(0, np.arange(256)) == 0).all()
    # scale 510: K = 130560, q = floor((130560 (2 u - 255) + 255) / 510) = 256 (2 u - 255) exactly: whole texels
    assert M.scale_k(510.0) == 130560 and (M.offsets(130560, np.arange(256)) == 256 * (2 * np.arange(256) - 255)).all()
    # a 5 x 1 ramp moved by whole texels under REPEAT: the map's alpha 128 reads 1 texel to the right, 127 one to the left
    ramp = np.array([[[n, n, n, 255] for n in (1, 2, 3, 4, 5)]], dtype=np.uint8)
    right = np.zeros((1, 5, 4), dtype=np.uint8)
    right[..., 3] = 128
    for filter in FILTERS:
        assert M.displace(ramp, right, (510.0, 0.0), M.A, M.A, filter, M.REPEAT)[0, :, 0].tolist() == [2, 3, 4, 5, 1]
        right[..., 3] = 127
        assert M.displace(ramp, right, (510.0, 0.0), M.A, M.A, filter, M.REPEAT)[0, :, 0].tolist() == [5, 1, 2, 3, 4]
        assert M.displace(ramp, right, (510.0, 0.0), M.A, M.A, filter, M.TRANSPARENT)[0, :, 0].tolist() == [0, 1, 2, 3, 4]
        right[..., 3] = 128
    for n, (filter, edge) in enumerate(itertools.product(FILTERS, M.EDGES)):
        (w, h), scale, (cx, cy) = ((7, 5), (3, 4), (1, 6))[n % 3], SCALES[1 + n % 5], PAIRS[n % 4]
        src, map = images(w, h, 100 + n, ("random", "clamped", "partly")[n % 3])
        image = M.displace(src, map, scale, cx, cy, filter, edge)
        for j, i in itertools.product(range(h), range(w)):
            assert image[j, i].tolist() == scalar_texel(src, map, i, j, scale, cx, cy, filter, edge), (filter, edge, scale, i, j)


def test_the_offsets_equal_the_model_and_keep_the_error_bound(lib):
    """crh_displace_offset for all 256 codes at the scales of the rule's corners; q is within 3/4 of a 1/256 texel of the real
    scale (u / 255 - 1/2) * 256, in exact rationals (the scale is the float the library was given)."""
    q = (C.c_int32 * 2)()
    worst = Fraction(0)
    for scale in (0.0, 1.0, -1.0, 0.3, 7.77, 255.0, 510.0, 1024.0, -1024.0):
        held = Fraction(float(np.float32(scale)))
        how = how_of((scale, -scale))
        for u in range(256):
            assert lib.crh_displace_offset(C.byref(how), u, 255 - u, q) == 0
            expect = (int(M.offsets(M.scale_k(scale), u)), int(M.offsets(M.scale_k(-scale), 255 - u)))
            assert (q[0], q[1]) == expect, (scale, u)
            assert displace_offset((scale, -scale), u, 255 - u) == expect
            for got, s, code in ((q[0], held, u), (q[1], -held, 255 - u)):
                error = abs(got - s * (Fraction(code, 255) - Fraction(1, 2)) * 256)
                worst = max(worst, error)
                assert error <= Fraction(3, 4), (scale, code, got)
        if scale == 510.0:
            assert all(int(M.offsets(M.scale_k(scale), u)) == 256 * (2 * u - 255) for u in range(256))
        if scale == 255.0:
            assert all(int(M.offsets(M.scale_k(scale), u)) == 128 * (2 * u - 255) for u in range(256))
    assert worst > Fraction(1, 2)  # (the bound is not idle: K's quarter is used)
    # no neutral code: 127 and 128 give -+ scale / 510
    assert displace_offset(510.0, 127, 128) == (-256, 256) and displace_offset(510.0, 0, 255) == (-255 * 256, 255 * 256)


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("filter", FILTERS, ids=["nearest", "linear"])
def test_the_library_and_the_python_mirror_equal_the_model(lib, filter, size):
    w, h = size
    for n, (edge, (cx, cy), kind) in enumerate(itertools.product(M.EDGES, PAIRS, ("random", "transparent", "clamped", "partly"))):
        src, map = images(w, h, 7 + n, kind)
        for scale in (SCALES[n % len(SCALES)], SCALES[(n + 3) % len(SCALES)]):
            expect = M.displace(src, map, scale, cx, cy, filter, edge)
            what = (size, filter, edge, cx, cy, kind, scale)
            same(library(lib, src, map, scale, cx, cy, filter, edge), expect, what)
            same(displace_texels(src, map, scale, Channel(cx), Channel(cy), Filter(filter), BlurEdge(edge)), expect, what)
            assert (expect[..., :3] <= expect[..., 3:]).all()  # rgb <= a survives (the source is premultiplied)


def test_zero_scales_copy_and_leave_an_axis_unmoved(lib):
    for (w, h), filter, edge in itertools.product(SIZES, FILTERS, M.EDGES):
        src, map = images(w, h, w * 31 + h, "clamped")
        for cx, cy in PAIRS:
            assert np.array_equal(library(lib, src, map, (0.0, 0.0), cx, cy, filter, edge), src), (w, h, filter, edge)
        # x unmoved: every texel comes from its own column (a source whose rows are all equal comes back)
        columns = np.broadcast_to(src[:1], src.shape).copy()
        assert np.array_equal(library(lib, columns, map, (0.0, 37.5), M.R, M.G, filter, M.PAD if edge == M.TRANSPARENT else edge), columns), (w, h, filter, edge)
        rows = np.broadcast_to(src[:, :1], src.shape).copy()
        assert np.array_equal(library(lib, rows, map, (-20.0, 0.0), M.R, M.G, filter, M.PAD if edge == M.TRANSPARENT else edge), rows), (w, h, filter, edge)


def test_equal_texels_come_back_exactly(lib):
    texel = np.array([17, 99, 200, 231], dtype=np.uint8)
    for (w, h), filter, edge in itertools.product(SIZES, FILTERS, (M.PAD, M.REPEAT, M.REFLECT)):
        src, map = images(w, h, 5)
        src[:] = texel
        for scale in SCALES:
            assert (library(lib, src, map, scale, M.G, M.B, filter, edge) == texel).all(), (w, h, filter, edge, scale)


def test_scale_510_moves_by_whole_texels_and_the_filters_agree(lib):
    for (w, h), edge, (cx, cy) in itertools.product(SIZES, M.EDGES, PAIRS[:3]):
        src, map = images(w, h, w + h, "partly")
        j, i = np.mgrid[0:h, 0:w]
        expect = M.fetch(src, i + 2 * M.codes(map, cx) - 255, j + 2 * M.codes(map, cy) - 255, edge).astype(np.uint8)
        for filter in FILTERS:
            same(library(lib, src, map, (510.0, 510.0), cx, cy, filter, edge), expect, (w, h, edge, cx, cy, filter))


def test_a_constant_map_is_a_translation_and_composite_copy_under_transparent(lib):
    """A constant map whose q is a multiple of 256 translates; under TRANSPARENT that is crh_image_composite's COPY of the source onto a
    transparent backdrop of the same size at (-qx / 256, -qy / 256) — through crh_composite_texels on the shifted copy the device call
    would read."""
    for (w, h), (ux, uy) in itertools.product(SIZES, ((128, 127), (130, 120), (255, 0), (100, 140))):
        src, map = images(w, h, ux)
        map[:] = (0, 0, 0, 255)
        map[..., 0], map[..., 1] = ux, uy
        qx, qy = displace_offset(510.0, ux, uy)
        assert qx % 256 == 0 and qy % 256 == 0
        dx, dy = -qx // 256, -qy // 256  # where the source's texel (0, 0) lands
        shifted = np.zeros_like(src)  # the source at offset (dx, dy) over the backdrop's extent
        xs, ys = slice(max(dx, 0), max(min(w + dx, w), 0)), slice(max(dy, 0), max(min(h + dy, h), 0))
        part = src[max(-dy, 0):max(-dy, 0) + max(ys.stop - ys.start, 0), max(-dx, 0):max(-dx, 0) + max(xs.stop - xs.start, 0)]
        if part.size:
            shifted[ys, xs] = part
        copy = composite_texels(shifted.reshape(-1, 4), np.zeros_like(src).reshape(-1, 4), op=CompositeOp.Copy).reshape(src.shape)
        for filter in FILTERS:
            same(library(lib, src, map, (510.0, 510.0), M.R, M.G, filter, M.TRANSPARENT), copy, (w, h, ux, uy, filter))
            j, i = np.mgrid[0:h, 0:w]
            for edge in (M.PAD, M.REPEAT, M.REFLECT):
                same(library(lib, src, map, (510.0, 510.0), M.R, M.G, filter, edge), M.fetch(src, i - dx, j - dy, edge).astype(np.uint8), (w, h, ux, uy, filter, edge))


def test_no_code_is_neutral_and_a_transparent_map_moves_by_half_the_scale(lib):
    src, map = images(9, 5, 3)
    map[:] = 0  # u = 0 on every channel: -scale / 2 = 2 texels to the left and 1 up at scale (4, 2)
    j, i = np.mgrid[0:5, 0:9]
    for filter, (cx, cy) in itertools.product(FILTERS, PAIRS):
        assert np.array_equal(library(lib, src, map, (4.0, 2.0), cx, cy, filter, M.REPEAT), M.fetch(src, i - 2, j - 1, M.REPEAT).astype(np.uint8))
    for u in (127, 128):
        map[:] = (0, 0, 0, u)
        assert not np.array_equal(library(lib, src, map, (510.0, 510.0), M.A, M.A, M.NEAREST, M.REPEAT), src)
    assert displace_offset(1024.0, 127, 128) == (-514, 514)  # floor((-262144 + 255) / 510) and floor((262144 + 255) / 510)


def test_many_periods_out_on_short_axes(lib):
    """Scale 1024 on a 1-texel and a 3-texel axis: an index up to 513 texels out, 513 or 171 periods, under each wrapping edge."""
    for (w, h), edge, filter in itertools.product(((1, 1), (3, 1), (1, 3), (3, 3), (1, 64), (64, 1)), (M.PAD, M.REPEAT, M.REFLECT), FILTERS):
        src, map = images(w, h, 11 * w + h)
        map[0, 0], map[-1, -1] = (0, 0, 0, 0), (255, 255, 255, 255)  # both ends of the range are there
        for scale, (cx, cy) in itertools.product(((1024.0, 1024.0), (-1024.0, 1024.0)), PAIRS[:3]):
            same(library(lib, src, map, scale, cx, cy, filter, edge), M.displace(src, map, scale, cx, cy, filter, edge), (w, h, edge, filter, scale, cx, cy))


def test_refusals_statuses_texts_and_untouched_outputs(lib):
    INVALID, NON_FINITE = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_NON_FINITE
    nan, inf = float("nan"), float("inf")
    channel, filter_text, edge_text = "a channel is above CRH_CHANNEL_A", "filter is neither CRH_FILTER_NEAREST nor CRH_FILTER_LINEAR", "edge is above CRH_BLUR_EDGE_REFLECT"
    finite, large = "a scale is not finite", "a scale is outside [-1024, 1024]"
    cases = ((how_of(x_channel=4), INVALID, channel), (how_of(y_channel=4), INVALID, channel), (how_of(filter=2), INVALID, filter_text), (how_of(filter=0x101), INVALID, filter_text),
             (how_of(filter=0x100), INVALID, filter_text), (how_of(edge=4), INVALID, edge_text), (how_of(scale=(nan, 1.0)), NON_FINITE, finite), (how_of(scale=(1.0, -inf)), NON_FINITE, finite),
             (how_of(scale=(1024.5, 1.0)), INVALID, large), (how_of(scale=(1.0, -1025.0)), INVALID, large),
             # the order: an enumerator before a non-finite scale, a non-finite scale before a range, the channels before the filter before the edge
             (how_of(scale=(nan, 1.0), edge=7), INVALID, edge_text), (how_of(scale=(2000.0, inf)), NON_FINITE, finite), (how_of(x_channel=9, filter=9, edge=9), INVALID, channel),
             (how_of(filter=9, edge=9), INVALID, filter_text))
    src, map = images(5, 3, 1)
    out = np.full((3, 5, 4), 0xA5, dtype=np.uint8)
    q = (C.c_int32 * 2)(77, 77)
    handle = C.c_void_p(0x1234)
    for how, status, text in cases:
        assert lib.crh_displace_validate(C.byref(how)) == status, text
        assert lib.crh_last_error().decode() == PREFIX + text
        assert lib.crh_displace_texels(5, 3, src.ctypes.data, map.ctypes.data, C.byref(how), out.ctypes.data) == status and (out == 0xA5).all(), text
        assert lib.crh_last_error().decode() == PREFIX + text
        assert lib.crh_displace_offset(C.byref(how), 1, 2, q) == status and (q[0], q[1]) == (77, 77), text
        # (a refused crh_image_displace does not touch the device: the images are not looked at before the fields)
        assert lib.crh_image_displace(C.c_void_p(0x10), C.c_void_p(0x10), C.byref(how), C.byref(handle)) == status and handle.value == 0x1234, text
        assert lib.crh_last_error().decode() == PREFIX + text
        # a size outside the range beside it: the field is named
        assert lib.crh_displace_texels(0, 3, src.ctypes.data, map.ctypes.data, C.byref(how), out.ctypes.data) == status and lib.crh_last_error().decode() == PREFIX + text
    good = how_of()
    null = PREFIX + "a null argument"
    assert lib.crh_displace_validate(C.byref(good)) == 0
    assert lib.crh_displace_validate(None) == INVALID and lib.crh_last_error().decode() == null
    for arguments in ((None, map.ctypes.data, C.byref(good), out.ctypes.data), (src.ctypes.data, None, C.byref(good), out.ctypes.data), (src.ctypes.data, map.ctypes.data, None, out.ctypes.data),
                      (src.ctypes.data, map.ctypes.data, C.byref(good), None)):
        assert lib.crh_displace_texels(5, 3, *arguments) == INVALID and lib.crh_last_error().decode() == null and (out == 0xA5).all()
    # a null beside a bad field: the null is named
    assert lib.crh_displace_texels(5, 3, None, map.ctypes.data, C.byref(how_of(edge=9)), out.ctypes.data) == INVALID and lib.crh_last_error().decode() == null
    for arguments in ((None, C.c_void_p(0x10), C.byref(good), C.byref(handle)), (C.c_void_p(0x10), None, C.byref(good), C.byref(handle)), (C.c_void_p(0x10), C.c_void_p(0x10), None, C.byref(handle)),
                      (C.c_void_p(0x10), C.c_void_p(0x10), C.byref(good), None)):
        assert lib.crh_image_displace(*arguments) == INVALID and lib.crh_last_error().decode() == null and handle.value == 0x1234
    assert lib.crh_displace_offset(None, 1, 2, q) == INVALID and lib.crh_last_error().decode() == null
    assert lib.crh_displace_offset(C.byref(good), 1, 2, None) == INVALID and lib.crh_last_error().decode() == null
    for codes in ((256, 0), (0, 256), (0xFFFFFFFF, 3)):
        assert lib.crh_displace_offset(C.byref(good), codes[0], codes[1], q) == INVALID and lib.crh_last_error().decode() == PREFIX + "a code is above 255" and (q[0], q[1]) == (77, 77)
    for w, h in ((0, 3), (5, 0), (16385, 1), (1, 16385)):
        assert lib.crh_displace_texels(w, h, src.ctypes.data, map.ctypes.data, C.byref(good), out.ctypes.data) == INVALID and (out == 0xA5).all()
        assert lib.crh_last_error().decode() == PREFIX + "width and height lie in [1, 16384]"
        # a size outside the range and an output that is an input: the size is named
        assert lib.crh_displace_texels(w, h, src.ctypes.data, map.ctypes.data, C.byref(good), src.ctypes.data) == INVALID
        assert lib.crh_last_error().decode() == PREFIX + "width and height lie in [1, 16384]"
    before = (src.copy(), map.copy())
    for target in (src, map):
        assert lib.crh_displace_texels(5, 3, src.ctypes.data, map.ctypes.data, C.byref(good), target.ctypes.data) == INVALID
        assert lib.crh_last_error().decode() == PREFIX + "out_rgba8 is rgba8 or map_rgba8"
    assert np.array_equal(src, before[0]) and np.array_equal(map, before[1])
    # the limits themselves are served
    for how in (how_of(scale=(1024.0, -1024.0), x_channel=3, y_channel=3, filter=0, edge=3), how_of(scale=(-0.0, 0.0))):
        assert lib.crh_displace_validate(C.byref(how)) == 0 and lib.crh_displace_texels(5, 3, src.ctypes.data, map.ctypes.data, C.byref(how), out.ctypes.data) == 0


def test_unaligned_bytes(lib):
    src, map = images(7, 3, 2, "partly")
    raw_in, raw_map, raw_out = (np.full(7 * 3 * 4 + 3, 0xA5, dtype=np.uint8) for _ in range(3))
    raw_in[1:-2], raw_map[3:] = src.reshape(-1), map.reshape(-1)
    for filter, edge in itertools.product(FILTERS, M.EDGES):
        how = how_of((2.5, -3.25), M.B, M.A, filter, edge)
        assert lib.crh_displace_texels(7, 3, raw_in.ctypes.data + 1, raw_map.ctypes.data + 3, C.byref(how), raw_out.ctypes.data + 2) == 0
        assert np.array_equal(raw_out[2:-1].reshape(3, 7, 4), M.displace(src, map, (2.5, -3.25), M.B, M.A, filter, edge)) and (raw_out[:2] == 0xA5).all() and raw_out[-1] == 0xA5


def test_the_python_mirror(lib):
    src, map = images(12, 5, 4)
    assert np.array_equal(displace_texels(src, map, 6.5), M.displace(src, map, 6.5, M.A, M.A, M.LINEAR, M.TRANSPARENT))  # SVG's defaults; a scalar scale serves both axes
    assert np.array_equal(displace_texels(src, map, (6.5, -2), Channel.R, Channel.B, Filter.Nearest, BlurEdge.Reflect), M.displace(src, map, (6.5, -2), M.R, M.B, M.NEAREST, M.REFLECT))
    assert np.array_equal(displace_texels(src[:, ::2], map[:, ::2], 3.0), M.displace(np.ascontiguousarray(src[:, ::2]), np.ascontiguousarray(map[:, ::2]), 3.0))  # strided views
    for bad in (dict(scale=1025.0), dict(scale=float("nan")), dict(scale=1.0, x_channel=4), dict(scale=1.0, filter=Filter.LinearMipmap), dict(scale=1.0, edge=4)):
        with pytest.raises(ContrastError):
            displace_texels(src, map, **bad)
    with pytest.raises(ContrastError):
        displace_texels(src, map[:, :5], 1.0)
    with pytest.raises(ContrastError):
        displace_texels(src.astype(np.float32), map, 1.0)
    with pytest.raises(ContrastError):
        displace_offset(1.0, 256, 0)


def test_the_library_exports_and_the_mirrors_agree_across_header_python_and_ffi_rs(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    exports = open(b.write_export_map()).read()
    for name in NAMES:
        assert f"    {name};\n" in exports
    assert any(os.path.basename(h) == "displace.hpp" for h in b.header_deps())
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    assert "CRH_CHANNEL_R = 0, CRH_CHANNEL_G = 1, CRH_CHANNEL_B = 2, CRH_CHANNEL_A = 3" in header and "#define CRH_MAX_DISPLACE_SCALE 1024.0f" in header
    assert C.sizeof(_ffi.DisplaceC) == 6 * 4
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    assert committed == fresh
    for text in ("pub fn crh_displace_validate(how: *const crh_displace) -> crh_status;",
                 "pub fn crh_displace_offset(how: *const crh_displace, code_x: u32, code_y: u32, q: *mut i32) -> crh_status;",
                 "pub fn crh_displace_texels(width: u32, height: u32, rgba8: *const c_void, map_rgba8: *const c_void, how: *const crh_displace, out_rgba8: *mut c_void) -> crh_status;",
                 "pub fn crh_image_displace(src: *const crh_image, map: *const crh_image, how: *const crh_displace, out: *mut *mut crh_image) -> crh_status;",
                 "pub const CRH_CHANNEL_A: u32 = 3;", "pub const CRH_MAX_DISPLACE_SCALE: usize = 1024;",
                 "pub struct crh_displace {\n    pub scale: [f32; 2],\n    pub x_channel: u32,\n    pub y_channel: u32,\n    pub filter: u32,\n    pub edge: u32,\n}"):
        assert text in committed, text
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub enum Channel {", "pub struct Displace {", "pub fn displace_validate(displace: &Displace) -> Result<(), Error>",
                 "pub fn displace_offset(displace: &Displace, code_x: u32, code_y: u32) -> Result<[i32; 2], Error>",
                 "pub fn displace_texels(width: u32, height: u32, texels: &[u8], map: &[u8], displace: &Displace) -> Result<Vec<u8>, Error>",
                 "pub fn displace(&self, map: &Image, displace: &Displace) -> Result<Image, Error>"):
        assert text in shim, text
    for name in NAMES:
        assert f"ffi::{name}(" in shim, name
    mirror = open(os.path.join(ROOT, "include", "contrast_renderer.hpp")).read()
    for text in ("enum class Channel : uint32_t {", "struct Displace {", "Image displace(const Image& map, const Displace& displace) const",
                 "inline std::vector<uint8_t> displace_texels(uint32_t width, uint32_t height,", "inline std::array<int32_t, 2> displace_offset(const Displace& displace, uint32_t code_x, uint32_t code_y)"):
        assert text in mirror, text
    import contrast_renderer_amd
    for name in ("Channel", "displace_texels", "displace_offset"):
        assert name in contrast_renderer_amd.__all__ and hasattr(contrast_renderer_amd, name)
    assert hasattr(contrast_renderer_amd.Image, "displace")
    assert [c.value for c in Channel] == [0, 1, 2, 3]


def test_the_cpp_mirror_of_displace_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "displace_harness.cpp"),
               "-o", os.path.join(tmp, "displace_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """A stand-alone program (its own main, no library, nothing loaded into python) around csrc/displace.hpp, the rule that crh_displace_texels
    runs: compiled as host code with the two sanitizers (the flag goes to the host compilation alone) and run once. It sweeps the
    many-periods and the 16384-axis cases in heap buffers sized exactly."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        binary = os.path.join(tmp, "displace_sanitize")
        # -x c++ and -Xarch_host: plain host C++, the sanitizers on the host alone (no device pass; clang links the sanitizers' runtime statically, so the program needs nothing preloaded)
        cmd = [hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
               "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), "-I", os.path.join(ROOT, "contrast_renderer_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "displace_sanitize.cpp"), "-o", binary]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert re.search(r"\d+ texels, 0 failures$", done.stdout.strip())
