"""crh_image_convolve without a GPU: crh_convolve_texels (host only, the rule of csrc/convolve.hpp that the kernel runs) and
crh_convolve_coefficients byte for byte against the numpy model of tests/convolve_model.py; every consequence the header states; the errors with
their statuses and texts; the Python / C++ / Rust mirrors; and one run of the rule as a stand-alone program under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, ContrastError, ConvolveKernel, _ffi, convolve_coefficients, convolve_texels
from contrast_renderer_amd import renderer as R

import composite_model as CM
import convolve_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_convolve_validate", "crh_convolve_coefficients", "crh_convolve_texels", "crh_image_convolve")
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17)]
ORDERS = [(1, 1), (3, 3), (2, 4), (5, 5), (15, 1), (1, 15), (15, 15)]
SAME_SIZE = (M.PAD, M.REPEAT, M.REFLECT)
MODES = (False, True)


def targets_of(order):
    return [(order[0] // 2, order[1] // 2), (0, 0), (order[0] - 1, order[1] - 1)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


_made = {}


def made_once(key, make):
    if key not in _made:
        _made[key] = make()
        if isinstance(_made[key], np.ndarray):
            _made[key].setflags(write=False)
    return _made[key]


def pixels_of(w, h):
    """Random texels of a size (some colours above their alpha), made once and never written."""
    return made_once((w, h), lambda: M.random_pixels(np.random.RandomState(5 * w + h), w, h))


def kernel_of(order):
    """A random signed kernel of an order and its divisor, made once."""
    return made_once(("kernel", order), lambda: M.random_kernel(np.random.RandomState(31 * order[0] + order[1]), *order))


def how_of(kernel, divisor=1.0, bias=0.0, target=None, edge=M.PAD, preserve_alpha=0, order=None):
    """-> (ConvolveC, the float array it points to)"""
    k = np.ascontiguousarray(kernel, dtype=np.float32)
    oy, ox = k.shape if order is None else order[::-1]
    tx, ty = (ox // 2, oy // 2) if target is None else target
    values = (C.c_float * k.size)(*[float(v) for v in k.ravel()])
    return _ffi.ConvolveC(ox, oy, tx, ty, C.cast(values, C.POINTER(C.c_float)), divisor, bias, edge, preserve_alpha), values


def library(lib, pixels, kernel, divisor=1.0, bias=0.0, target=None, edge=M.PAD, preserve_alpha=False):
    h, w = pixels.shape[:2]
    how, keep = how_of(kernel, divisor, bias, target, edge, int(preserve_alpha))
    out = np.full((h, w, 4), 0xAB, dtype=np.uint8)
    assert lib.crh_convolve_texels(w, h, pixels.ctypes.data, C.byref(how), out.ctypes.data) == _ffi.OK, lib.crh_last_error()
    return out


def same(got, expect, what):
    assert got.shape == expect.shape, (what, got.shape, expect.shape)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"


def test_the_model_is_the_definition():
    """The numpy model against the definition taken one texel and one tap at a time, on sizes small enough for it."""
    for w, h in ((1, 1), (1, 7), (5, 3), (7, 4)):
        for order in ((1, 1), (3, 3), (2, 4), (5, 1), (1, 15)):
            kernel, divisor = kernel_of(order)
            for target in targets_of(order):
                for edge in M.EDGES:
                    for mode in MODES:
                        same(M.convolve(pixels_of(w, h), kernel, divisor, -0.2, target, edge, mode), M.brute(pixels_of(w, h), kernel, divisor, -0.2, target, edge, mode),
                             (w, h, order, target, edge, mode))


@pytest.mark.parametrize("edge", M.EDGES, ids=[BlurEdge(e).name for e in M.EDGES])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_library_and_the_python_mirror_equal_the_model(lib, size, edge):
    pixels = pixels_of(*size)
    for order in ORDERS:
        kernel, divisor = kernel_of(order)
        for target in targets_of(order):
            for mode in MODES:
                expect = M.convolve(pixels, kernel, divisor, 0.1, target, edge, mode)
                same(library(lib, pixels, kernel, divisor, 0.1, target, edge, mode), expect, (size, order, target, edge, mode))
                same(convolve_texels(pixels, kernel, divisor, 0.1, target, BlurEdge(edge), mode), expect, ("mirror", size, order, target, edge, mode))


def test_the_coefficients_equal_the_model(lib):
    for order in ORDERS:
        kernel, divisor = kernel_of(order)
        for bias in (0.0, 0.1, -1.0, 1.0, 0.49999):
            expect_k, expect_bias = M.quantize(kernel, divisor, bias)
            how, keep = how_of(kernel, divisor, bias)
            k = np.full(order[0] * order[1] + 1, 0x5A5A5A5A, dtype=np.int32)
            bias_k = C.c_int32(7)
            assert lib.crh_convolve_coefficients(C.byref(how), k.ctypes.data_as(C.POINTER(C.c_int32)), order[0] * order[1], C.byref(bias_k)) == _ffi.OK
            assert np.array_equal(k[:-1].reshape(order[::-1]), expect_k) and k[-1] == 0x5A5A5A5A and bias_k.value == expect_bias
            got_k, got_bias = convolve_coefficients(kernel, divisor, bias)
            assert np.array_equal(got_k, expect_k) and got_bias == expect_bias and got_k.dtype == np.int32
            assert lib.crh_convolve_coefficients(C.byref(how), None, 0, C.byref(bias_k)) == _ffi.OK  # k == NULL: validate, and the bias alone
            assert lib.crh_convolve_coefficients(C.byref(how), None, 0, None) == _ffi.OK
    # the rounding: floor(x + 1/2), halves upwards for both signs
    k, bias_k = convolve_coefficients([[0.5, -0.5, 1.5, -1.5]], 65536.0, 0.5 / 65536.0)
    assert k.tolist() == [[1, 0, 2, -1]] and bias_k == 1
    assert convolve_coefficients(ConvolveKernel.box(3))[0].tolist() == [[7282] * 3] * 3  # divisor=None: the sum of the entries
    assert convolve_coefficients(ConvolveKernel.laplacian())[0].tolist() == [[0, 65536, 0], [65536, -262144, 65536], [0, 65536, 0]]  # a sum of 0: divisor 1


EXTREMES = [(+1, [[1.0] * 8] * 8), (-1, [[-1.0] * 8] * 8), (+1, [[64.0]]), (-1, [[-64.0]]), (+1, [[64.0 / 225] * 15] * 15)]


def test_both_ends_of_the_accumulator(lib):
    """All-positive and all-negative kernels with sum |k| = 2^22 exactly and bias +-1 on an all-255 image: the largest magnitudes the header states."""
    white = made_once("white", lambda: np.full((5, 9, 4), 255, dtype=np.uint8))
    for sign, kernel in EXTREMES[:4]:
        k, _ = M.quantize(kernel, 1.0, float(sign))
        assert int(np.abs(k).sum()) == 1 << 22
        for edge in M.EDGES:
            for mode in MODES:
                n, _ = M.sums(white, kernel, 1.0, float(sign), None, edge, mode)
                if edge != M.TRANSPARENT:
                    assert int(n[..., :3].max() if sign > 0 else n[..., :3].min()) == (1086291968 if sign > 0 else -1086226432)  # +-(2^22 + 2^16) * 255 + 32768
                expect = M.convolve(white, kernel, 1.0, float(sign), None, edge, mode)
                same(library(lib, white, kernel, 1.0, float(sign), None, edge, mode), expect, (sign, edge, mode))
                if edge != M.TRANSPARENT:
                    assert (expect[..., :3] == (255 if sign > 0 else 0)).all()
    # the limit itself and one step above it
    how, keep = how_of(EXTREMES[4][1])
    assert lib.crh_convolve_validate(C.byref(how)) == _ffi.OK
    how, keep = how_of([[32.0, 32.0001]])
    assert lib.crh_convolve_validate(C.byref(how)) == _ffi.ERR_INVALID_ARGUMENT


def all_pairs():
    """Every pair c <= a as a 257 x 128 image: (c, a - c, c, a)"""
    def make():
        pairs = np.array([(c, a) for a in range(256) for c in range(a + 1)], dtype=np.uint8)
        assert len(pairs) == 32896 == 257 * 128
        c, a = pairs[:, 0], pairs[:, 1]
        return np.ascontiguousarray(np.stack([c, a - c, c, a], axis=1).reshape(128, 257, 4))
    return made_once("pairs", make)


def test_the_identity_kernel_returns_every_loaded_texel(lib):
    pairs = all_pairs()
    for edge in M.EDGES:
        for mode in MODES:
            same(library(lib, pairs, [[1.0]], 1.0, 0.0, None, edge, mode), pairs, ("identity", edge, mode))
    loose = pixels_of(33, 17)  # colours above their alpha come back clamped: the loaded texel
    assert (loose[..., :3] > loose[..., 3:]).any()
    for mode in MODES:
        same(library(lib, loose, ConvolveKernel.identity(), 1.0, 0.0, None, M.PAD, mode), M.load(loose).astype(np.uint8), ("loaded", mode))


def test_a_single_tap_is_a_translation(lib):
    """Every cell of a 3 x 2 kernel: under TRANSPARENT the result is the source composited COPY onto a transparent backdrop at the stated offset."""
    pixels = pixels_of(33, 17)
    backdrop = np.zeros_like(pixels)
    order_x, order_y = 3, 2
    for target in ((1, 1), (0, 0), (2, 1)):
        for r in range(order_y):
            for c in range(order_x):
                kernel = np.zeros((order_y, order_x), dtype=np.float32)
                kernel[r, c] = 1.0
                dx, dy = c + target[0] - (order_x - 1), r + target[1] - (order_y - 1)
                expect = CM.composite(backdrop, pixels, CM.COPY, CM.NORMAL, 255, dx, dy)
                same(library(lib, pixels, kernel, 1.0, 0.0, target, M.TRANSPARENT, False), expect, ("translation", target, r, c))
                moved = library(lib, pixels, kernel, 1.0, 0.0, target, M.REPEAT, False)  # under REPEAT: a roll of the loaded texels
                same(moved, np.roll(M.load(pixels).astype(np.uint8), (dy, dx), axis=(0, 1)), ("roll", target, r, c))


def test_a_kernel_that_sums_to_one_keeps_a_constant_image(lib):
    rng = np.random.RandomState(9)
    kernels = [ConvolveKernel.box(3), ConvolveKernel.box(5), ConvolveKernel.box(15), ConvolveKernel.sharpen(0.7), rng.uniform(0.0, 1.0, (15, 15)), rng.uniform(0.0, 1.0, (4, 7)),
               rng.uniform(-0.3, 1.0, (5, 5))]
    for kernel in kernels:
        k, _ = convolve_coefficients(kernel)  # divisor=None: the sum of the entries
        e = int(k.sum()) - 65536
        assert abs(e) <= 112, e
        for texel in ((255, 255, 255, 255), (0, 0, 0, 0), (1, 0, 1, 1), (200, 13, 77, 201), (0, 128, 64, 128), (3, 2, 1, 254)):
            constant = np.ascontiguousarray(np.broadcast_to(np.array(texel, dtype=np.uint8), (6, 19, 4)))
            for edge in SAME_SIZE:
                for mode in MODES:
                    same(convolve_texels(constant, kernel, edge=BlurEdge(edge), preserve_alpha=mode), constant, (np.asarray(kernel).shape, texel, edge, mode, e))


def test_colours_stay_below_alpha_and_the_result_is_within_the_stated_bound(lib):
    for size in ((5, 3), (33, 17)):
        pixels = pixels_of(*size)
        loaded = M.load(pixels).astype(np.float64)
        for order in ORDERS:
            kernel, divisor = kernel_of(order)
            real_k = kernel.astype(np.float64) / float(np.float32(divisor))
            for edge in M.EDGES:
                for bias in (0.0, 0.3):
                    for mode in MODES:
                        got = library(lib, pixels, kernel, divisor, bias, None, edge, mode)
                        assert (got[..., :3] <= got[..., 3:]).all(), (size, order, edge, bias, mode)  # c' <= a'
                    # the real-valued formula on the loaded codes, in float64
                    h, w = pixels.shape[:2]
                    oy, ox = kernel.shape
                    real = np.full((h, w, 4), 255.0 * float(np.float32(bias)))
                    for r in range(oy):
                        for c in range(ox):
                            y = np.arange(h) - oy // 2 + (oy - 1 - r)
                            x = np.arange(w) - ox // 2 + (ox - 1 - c)
                            if edge == M.TRANSPARENT:
                                inside = ((y >= 0) & (y < h))[:, None] & ((x >= 0) & (x < w))[None, :]
                                real += real_k[r, c] * loaded[np.clip(y, 0, h - 1)][:, np.clip(x, 0, w - 1)] * inside[:, :, None]
                            else:
                                real += real_k[r, c] * loaded[M.wrap(y, h, edge)][:, M.wrap(x, w, edge)]
                    real = np.clip(real, 0.0, 255.0)
                    real[..., :3] = np.minimum(real[..., :3], real[..., 3:])
                    bound = 0.5 + 255.0 * (ox * oy + 1) / 2.0 ** 17
                    got = library(lib, pixels, kernel, divisor, bias, None, edge, False).astype(np.float64)
                    worst = float(np.abs(got - real).max())
                    assert worst <= bound + 1e-9, (size, order, edge, bias, worst, bound)


def test_errors_statuses_texts_and_untouched_outputs(lib):
    pixels = pixels_of(5, 3)
    out = np.full((3, 5, 4), 0xAB, dtype=np.uint8)
    k = np.full(225, 0x5A5A5A5A, dtype=np.int32)
    bias_k = C.c_int32(7)
    image = C.c_void_p(0x1234)
    nan, inf = float("nan"), float("inf")
    unit = [[0.0, 1.0, 0.0]]

    def refused(how, status, text, width=5, height=3):
        if (width, height) == (5, 3):  # (the struct itself is at fault, not the size)
            assert lib.crh_convolve_validate(C.byref(how)) == status, text
            if status == _ffi.ERR_INVALID_ARGUMENT:
                assert lib.crh_last_error().decode() == "crh_convolve_validate: " + text
        assert lib.crh_convolve_texels(width, height, pixels.ctypes.data, C.byref(how), out.ctypes.data) == status, text
        if status == _ffi.ERR_INVALID_ARGUMENT:
            assert lib.crh_last_error().decode() == "crh_convolve_validate: " + text
        assert (out == 0xAB).all()
        if (width, height) == (5, 3):
            assert lib.crh_convolve_coefficients(C.byref(how), k.ctypes.data_as(C.POINTER(C.c_int32)), 225, C.byref(bias_k)) == status, text
            assert (k == 0x5A5A5A5A).all() and bias_k.value == 7

    cases = [(dict(order=(0, 1)), "an order is outside [1, CRH_MAX_CONVOLVE_ORDER]"), (dict(order=(3, 0)), "an order is outside [1, CRH_MAX_CONVOLVE_ORDER]"),
             (dict(order=(16, 1)), "an order is outside [1, CRH_MAX_CONVOLVE_ORDER]"), (dict(order=(1, 16)), "an order is outside [1, CRH_MAX_CONVOLVE_ORDER]"),
             (dict(order=(0xFFFFFFFF, 1)), "an order is outside [1, CRH_MAX_CONVOLVE_ORDER]"),
             (dict(target=(3, 0)), "a target is not below its order"), (dict(target=(0, 1)), "a target is not below its order"), (dict(target=(0xFFFFFFFF, 0)), "a target is not below its order"),
             (dict(divisor=0.0), "divisor is 0"), (dict(divisor=-0.0), "divisor is 0"), (dict(bias=1.0001), "bias is outside [-1, 1]"), (dict(bias=-1.5), "bias is outside [-1, 1]"),
             (dict(edge=4), "edge is above CRH_BLUR_EDGE_REFLECT"), (dict(preserve_alpha=2), "preserve_alpha is above 1"),
             (dict(divisor=1.0 / 65.0), "the kernel over the divisor exceeds CRH_CONVOLVE_MAX_GAIN: sum |k| is above 64 * 65536"),
             (dict(divisor=1e-30), "the kernel over the divisor exceeds CRH_CONVOLVE_MAX_GAIN: sum |k| is above 64 * 65536")]
    for changes, text in cases:
        how, keep = how_of(np.zeros((16, 16)) if "order" in changes else unit, **changes)
        refused(how, _ffi.ERR_INVALID_ARGUMENT, text)
    how, keep = how_of([[22.0, -21.5, 21.0]])  # every entry inside the limit, their magnitudes' sum above it
    refused(how, _ffi.ERR_INVALID_ARGUMENT, "the kernel over the divisor exceeds CRH_CONVOLVE_MAX_GAIN: sum |k| is above 64 * 65536")
    for changes in (dict(divisor=nan), dict(divisor=inf), dict(bias=nan), dict(bias=-inf)):
        how, keep = how_of(unit, **changes)
        refused(how, _ffi.ERR_NON_FINITE, "non-finite")
    for bad in ([[0.0, nan, 0.0]], [[inf, 1.0, 0.0]], [[0.0, 1.0, -inf]]):
        how, keep = how_of(bad)
        refused(how, _ffi.ERR_NON_FINITE, "non-finite")
    how, keep = how_of(unit)
    for width, height in ((0, 3), (5, 0), (16385, 3), (5, 16385)):
        refused(how, _ffi.ERR_INVALID_ARGUMENT, "width and height lie in [1, 16384]", width, height)
    # null arguments and a null kernel
    null_kernel = _ffi.ConvolveC(1, 1, 0, 0, None, 1.0, 0.0, 1, 0)
    refused(null_kernel, _ffi.ERR_INVALID_ARGUMENT, "a null argument")
    assert lib.crh_convolve_validate(None) == _ffi.ERR_INVALID_ARGUMENT and lib.crh_last_error().decode() == "crh_convolve_validate: a null argument"
    assert lib.crh_convolve_coefficients(None, k.ctypes.data_as(C.POINTER(C.c_int32)), 225, C.byref(bias_k)) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_convolve_texels(5, 3, None, C.byref(how), out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode() == "crh_convolve_validate: a null argument"
    assert lib.crh_convolve_texels(5, 3, pixels.ctypes.data, C.byref(how), None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_convolve_texels(5, 3, pixels.ctypes.data, None, out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert (out == 0xAB).all() and (k == 0x5A5A5A5A).all() and bias_k.value == 7
    same_buffer = pixels.copy()
    assert lib.crh_convolve_texels(5, 3, same_buffer.ctypes.data, C.byref(how), same_buffer.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT  # out_rgba8 == rgba8
    assert lib.crh_last_error().decode() == "crh_convolve_validate: out_rgba8 is rgba8" and np.array_equal(same_buffer, pixels)
    # a capacity below order_x * order_y given together with k
    assert lib.crh_convolve_coefficients(C.byref(how), k.ctypes.data_as(C.POINTER(C.c_int32)), 2, C.byref(bias_k)) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode() == "crh_convolve_validate: capacity is below order_x * order_y" and (k == 0x5A5A5A5A).all() and bias_k.value == 7
    assert lib.crh_convolve_coefficients(C.byref(how), k.ctypes.data_as(C.POINTER(C.c_int32)), 3, C.byref(bias_k)) == _ffi.OK and k[:4].tolist() == [0, 65536, 0, 0x5A5A5A5A]
    # the limits themselves
    how, keep = how_of(np.full((15, 15), 64.0 / 225.0), 1.0, -1.0, (14, 14), 3, 1)
    assert lib.crh_convolve_validate(C.byref(how)) == _ffi.OK
    # the device entry point validates before it touches a device
    assert lib.crh_image_convolve(None, C.byref(how), C.byref(image)) == _ffi.ERR_INVALID_ARGUMENT and image.value == 0x1234
    assert lib.crh_last_error().decode() == "crh_convolve_validate: a null argument"


def test_unaligned_bytes(lib):
    pixels = pixels_of(33, 17)
    kernel, divisor = kernel_of((5, 5))
    expect = M.convolve(pixels, kernel, divisor, 0.0, None, M.REFLECT, True)
    how, keep = how_of(kernel, divisor, 0.0, None, M.REFLECT, 1)
    for shift_in, shift_out in ((1, 0), (0, 3), (3, 1)):
        raw_in, raw_out = np.zeros(pixels.size + 8, dtype=np.uint8), np.full(expect.size + 8, 0xCD, dtype=np.uint8)
        raw_in[shift_in:shift_in + pixels.size] = pixels.ravel()
        assert lib.crh_convolve_texels(33, 17, raw_in.ctypes.data + shift_in, C.byref(how), raw_out.ctypes.data + shift_out) == _ffi.OK
        assert np.array_equal(raw_out[shift_out:shift_out + expect.size].reshape(expect.shape), expect)
        assert (raw_out[:shift_out] == 0xCD).all() and (raw_out[shift_out + expect.size:] == 0xCD).all()


def test_the_python_mirror(lib):
    assert R.MAX_CONVOLVE_ORDER == 15 == M.MAX_ORDER and R.CONVOLVE_MAX_GAIN == 64.0
    assert callable(R.Image.convolve)
    pixels = pixels_of(33, 17)
    # the presets against what they are: the defaults divide by the sum (or 1) and aim at the centre
    for kernel, divisor in ((ConvolveKernel.identity(), 1.0), (ConvolveKernel.sharpen(0.5), 1.0), (ConvolveKernel.box(5), 25.0), (ConvolveKernel.emboss(), 1.0),
                            (ConvolveKernel.laplacian(), 1.0), (ConvolveKernel.sobel_x(), 1.0), (ConvolveKernel.sobel_y(), 1.0)):
        for mode in MODES:
            same(convolve_texels(pixels, kernel, bias=0.25, preserve_alpha=mode), M.convolve(pixels, kernel, divisor, 0.25, None, M.PAD, mode), (kernel, mode))
    assert np.asarray(ConvolveKernel.sharpen(2.0)).sum() == 1.0 and np.asarray(ConvolveKernel.sobel_x()).T.tolist() == ConvolveKernel.sobel_y()
    assert np.count_nonzero(ConvolveKernel.sobel_x()) == 6 and np.count_nonzero(ConvolveKernel.laplacian()) == 5
    same(convolve_texels(pixels, [[1.0, 2.0, 3.0]], target=(2, 0), edge=BlurEdge.Repeat), M.convolve(pixels, [[1.0, 2.0, 3.0]], 6.0, 0.0, (2, 0), M.REPEAT, False), "target")
    for bad in (dict(kernel=np.zeros((16, 1)) + 1), dict(kernel=[[1.0]], divisor=0.0), dict(kernel=[[1.0]], bias=2.0), dict(kernel=[[1.0]], edge=4), dict(kernel=[[65.0]], divisor=1.0),
                dict(kernel=[[1.0, 1.0]], target=(2, 0)), dict(kernel=[1.0, 2.0]), dict(kernel=np.zeros((0, 3)))):
        with pytest.raises(ContrastError) as refused:
            convolve_texels(pixels, **bad)
        assert refused.value.status == _ffi.ERR_INVALID_ARGUMENT
    with pytest.raises(ContrastError) as refused:
        convolve_texels(pixels, [[float("nan")]], divisor=1.0)
    assert refused.value.status == _ffi.ERR_NON_FINITE
    with pytest.raises(ContrastError):
        convolve_texels(pixels[..., :3], [[1.0]])
    with pytest.raises(ContrastError):
        convolve_coefficients([[65.0]], 1.0)
    sig = lib._crh_signatures
    assert [len(sig[name][1]) for name in NAMES] == [1, 4, 5, 3]
    fields = [name for name, _ in _ffi.ConvolveC._fields_]
    assert fields == ["order_x", "order_y", "target_x", "target_y", "kernel", "divisor", "bias", "edge", "preserve_alpha"]


def test_the_library_exports_and_the_mirrors_agree_across_header_python_and_ffi_rs(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    exports = open(b.write_export_map()).read()
    for name in NAMES:
        assert f"    {name};\n" in exports
    assert any(os.path.basename(h) == "convolve.hpp" for h in b.header_deps())
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    assert re.search(r"#define CRH_MAX_CONVOLVE_ORDER 15u\b", header) and re.search(r"#define CRH_CONVOLVE_MAX_GAIN 64\.0f\b", header)
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    assert committed == fresh
    for text in ("pub fn crh_convolve_validate(how: *const crh_convolve) -> crh_status;",
                 "pub fn crh_convolve_coefficients(how: *const crh_convolve, k: *mut i32, capacity: u32, bias_k: *mut i32) -> crh_status;",
                 "pub fn crh_convolve_texels(width: u32, height: u32, rgba8: *const c_void, how: *const crh_convolve, out_rgba8: *mut c_void) -> crh_status;",
                 "pub fn crh_image_convolve(src: *const crh_image, how: *const crh_convolve, out: *mut *mut crh_image) -> crh_status;",
                 "pub const CRH_MAX_CONVOLVE_ORDER: usize = 15;", "pub const CRH_CONVOLVE_MAX_GAIN: usize = 64;",
                 "pub struct crh_convolve {\n    pub order_x: u32,\n    pub order_y: u32,\n    pub target_x: u32,\n    pub target_y: u32,\n    pub kernel: *const f32,\n    pub divisor: f32,\n"
                 "    pub bias: f32,\n    pub edge: u32,\n    pub preserve_alpha: u32,\n}"):
        assert text in committed, text
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub struct ConvolveKernel {", "pub fn convolve_validate(kernel: &ConvolveKernel, edge: BlurEdge, preserve_alpha: bool) -> Result<(), Error>",
                 "pub fn convolve_coefficients(kernel: &ConvolveKernel) -> Result<(Vec<i32>, i32), Error>",
                 "pub fn convolve_texels(width: u32, height: u32, texels: &[u8], kernel: &ConvolveKernel, edge: BlurEdge, preserve_alpha: bool) -> Result<Vec<u8>, Error>",
                 "pub fn convolve(&self, kernel: &ConvolveKernel, edge: BlurEdge, preserve_alpha: bool) -> Result<Image, Error>",
                 "pub fn identity() -> ConvolveKernel", "pub fn sharpen(amount: f32) -> ConvolveKernel", "pub fn box_filter(n: u32) -> ConvolveKernel", "pub fn emboss() -> ConvolveKernel",
                 "pub fn laplacian() -> ConvolveKernel", "pub fn sobel_x() -> ConvolveKernel", "pub fn sobel_y() -> ConvolveKernel"):
        assert text in shim, text
    for name in NAMES:
        assert f"ffi::{name}(" in shim, name
    mirror = open(os.path.join(ROOT, "include", "contrast_renderer.hpp")).read()
    for text in ("struct ConvolveKernel {", "Image convolve(const ConvolveKernel& kernel, BlurEdge edge = BlurEdge::Pad, bool preserve_alpha = false) const",
                 "inline std::vector<int32_t> convolve_coefficients(const ConvolveKernel& kernel)", "inline std::vector<uint8_t> convolve_texels(uint32_t width, uint32_t height,"):
        assert text in mirror, text


def test_the_cpp_mirror_of_convolve_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "convolve_harness.cpp"),
               "-o", os.path.join(tmp, "convolve_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """A stand-alone program (its own main, no library, nothing loaded into python) around csrc/convolve.hpp, the rule that crh_convolve_texels
    runs: compiled as host code with the two sanitizers (the flag goes to the host compilation alone) and run once."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        binary = os.path.join(tmp, "convolve_sanitize")
        # -x c++ and -Xarch_host: plain host C++, the sanitizers on the host alone (no device pass; clang links the sanitizers' runtime statically, so the program needs nothing preloaded)
        cmd = [hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
               "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), "-I", os.path.join(ROOT, "contrast_renderer_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "convolve_sanitize.cpp"), "-o", binary]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert done.stdout.strip().endswith("100008 texels, 0 failures")
