"""crh_image_turbulence without a GPU (include/contrast_hip.h states the rule): the numpy model of tests/turbulence_model.py against a plain
scalar transcription and against known answers; crh_turbulence_tables, crh_turbulence_texels and the Python mirror byte for byte against the
model; every stated consequence and error; the mirrors; and the rule as a stand-alone program under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, TurbulenceKind, _ffi, turbulence_tables, turbulence_texels

import turbulence_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_turbulence_validate", "crh_turbulence_tables", "crh_turbulence_texels", "crh_image_turbulence")
SEEDS = (1, 0, -1, 2, 346, 2147483647, -2147483648)
SIZES = [(1, 1), (1, 7), (7, 1), (33, 17), (64, 32)]
OCTAVES = (0, 1, 4, 12)
# (base_frequency, offset): a plain pair, the largest frequency beside 0 at the largest offsets, integers with a fractional and a negative offset,
# a small and a large fractional frequency at the other corner of the offsets, and a zero frequency on x
PLACES = (((0.05, 0.08), (10.0, 20.0)), ((4.0, 0.0), (65536.0, -65536.0)), ((2.0, 3.0), (-0.5, 7.25)), ((0.013, 3.9), (-65536.0, 65536.0)), ((0.0, 0.3), (1.5, -3.75)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def how_of(kind=1, octaves=2, seed=5, stitch=0, opaque=0, base_frequency=(0.1, 0.2), offset=(0.0, 0.0)):
    how = _ffi.TurbulenceC()
    how.kind, how.octaves, how.seed, how.stitch, how.opaque = kind, octaves, seed, stitch, opaque
    how.base_frequency, how.offset = (C.c_float * 2)(*base_frequency), (C.c_float * 2)(*offset)
    return how


def library(lib, w, h, base_frequency, octaves, seed, kind, stitch, opaque, offset):
    fx, fy = (base_frequency, base_frequency) if np.isscalar(base_frequency) else base_frequency
    out = np.full((h, w, 4), 0xA5, dtype=np.uint8)
    how = how_of(int(kind), octaves, seed, int(stitch), int(opaque), (fx, fy), offset)
    assert lib.crh_turbulence_texels(w, h, C.byref(how), out.ctypes.data) == 0
    return out


def same(got, expect, what):
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"


# ---- a plain scalar transcription of the header's rule (Python floats are binary64 and nothing is contracted)
def scalar_texel(width, height, i, j, base_frequency, octaves, seed, kind, stitch, opaque, offset):
    s = seed
    if s <= 0:
        s = (abs(s) % 2147483646) + 1
    if s > 2147483646:
        s = 2147483646

    def draw():
        nonlocal s
        s = 16807 * (s % 127773) - 2836 * (s // 127773)
        if s <= 0:
            s += 2147483647
        return s

    G = [[None] * 256 for _ in range(4)]
    for k in range(4):
        for n in range(256):
            gx = float((draw() % 512) - 256) / 256.0
            gy = float((draw() % 512) - 256) / 256.0
            length = math.sqrt(gx * gx + gy * gy)
            G[k][n] = (0.0, 0.0) if length == 0.0 else (gx / length, gy / length)
    lat = list(range(256))
    for n in range(255, 0, -1):
        m = draw() % 256
        lat[n], lat[m] = lat[m], lat[n]

    def axis(f, n):
        f = float(np.float32(f))
        if not stitch or f == 0.0:
            return f, 0
        lo, hi = math.floor(n * f) / n, -math.floor(-(n * f)) / n
        chosen = hi if lo == 0.0 else (lo if f / lo < hi / f else hi)
        return chosen, int(math.floor(n * chosen + 0.5))

    (fx, px), (fy, py) = axis(base_frequency[0], width), axis(base_frequency[1], height)

    def wrap(v, period):
        return (v if period == 0 else v % period) & 255  # (Python's % is the non-negative one)

    def noise(k, vx, vy, period_x, period_y):
        flx, fly = math.floor(vx), math.floor(vy)
        rx0, ry0 = vx - flx, vy - fly
        rx1, ry1 = rx0 - 1.0, ry0 - 1.0
        bx0, bx1, by0, by1 = wrap(flx, period_x), wrap(flx + 1, period_x), wrap(fly, period_y), wrap(fly + 1, period_y)
        a0, a1 = lat[bx0], lat[bx1]
        q00, q10, q01, q11 = G[k][lat[(a0 + by0) & 255]], G[k][lat[(a1 + by0) & 255]], G[k][lat[(a0 + by1) & 255]], G[k][lat[(a1 + by1) & 255]]
        sx = (rx0 * rx0) * (3.0 - (2.0 * rx0))
        sy = (ry0 * ry0) * (3.0 - (2.0 * ry0))
        u = (rx0 * q00[0]) + (ry0 * q00[1])
        v = (rx1 * q10[0]) + (ry0 * q10[1])
        a = u + (sx * (v - u))
        u = (rx0 * q01[0]) + (ry1 * q01[1])
        v = (rx1 * q11[0]) + (ry1 * q11[1])
        b = u + (sx * (v - u))
        return a + (sy * (b - a))

    codes = []
    for k in range(3 if opaque else 4):
        vx, vy = (float(np.float32(offset[0])) + float(i)) * fx, (float(np.float32(offset[1])) + float(j)) * fy
        total, ratio = 0.0, 1.0
        for o in range(octaves):
            n = noise(k, vx, vy, px << o, py << o)
            total = total + ((n if kind == M.FRACTAL_NOISE else abs(n)) / ratio)
            ratio = ratio * 2.0
            vx, vy = vx * 2.0, vy * 2.0
        t = (total + 1.0) * 0.5 if kind == M.FRACTAL_NOISE else total
        codes.append(255 if t >= 1 else int(math.floor(t * 255.0 + 0.5)) if t > 0 else 0)
    alpha = 255 if opaque else codes[3]
    return [(c * alpha + 127) // 255 for c in codes[:3]] + [alpha]


def test_the_model_is_the_definition():
    """The known answers of a transcription made apart from this code, and the scalar transcription above on a few texels of every kind of call."""
    lattice, gradient = M.tables(1)
    assert list(lattice[:8]) == [190, 142, 200, 122, 63, 159, 188, 173] and list(lattice[252:]) == [52, 82, 88, 240]
    assert tuple(gradient[0, 0]) == (0.9959903964832638, -0.08946021525298777) and tuple(gradient[3, 255]) == (0.18226100971715328, -0.9832501840004322)
    assert list(M.tables(2147483646)[0][:4]) == [0, 104, 88, 4]
    assert tuple(M.tables(346)[1][1, 164]) == (0.0, 0.0)
    assert M.turbulence(4, 2, (0.05, 0.08), 4, 1, M.FRACTAL_NOISE, False, False, (10, 20)).tolist() == [
        [[79, 34, 32, 113], [84, 36, 32, 118], [84, 39, 32, 117], [78, 41, 31, 115]], [[95, 36, 40, 130], [100, 36, 44, 137], [103, 37, 44, 138], [97, 41, 41, 135]]]
    assert M.turbulence(4, 1, (0.3, 0.02), 3, 1, M.TURBULENCE, False, True, (-7.5, 2.25)).tolist() == [[[87, 54, 84, 255], [31, 30, 51, 255], [92, 38, 106, 255], [92, 59, 112, 255]]]
    assert M.turbulence(4, 1, (0.05, 0.07), 5, 7, M.FRACTAL_NOISE, True, False, (3, -5)).tolist() == [[[39, 43, 32, 93], [64, 64, 64, 128], [93, 86, 105, 162], [64, 64, 64, 128]]]
    for n, (kind, stitch, opaque) in enumerate(itertools.product(M.KINDS, (False, True), (False, True))):
        frequency, offset = PLACES[n % len(PLACES)]
        octaves, seed, (w, h) = (1, 4, 12)[n % 3], (346, 7, -3)[n % 3], ((33, 17), (64, 32))[n % 2]
        image = M.turbulence(w, h, frequency, octaves, seed, kind, stitch, opaque, offset)
        for i, j in ((0, 0), (w - 1, h - 1), (w // 2, 3), (5, h // 2)):
            assert image[j, i].tolist() == scalar_texel(w, h, i, j, frequency, octaves, seed, kind, stitch, opaque, offset), (kind, stitch, opaque, i, j)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_tables_equal_the_model(lib, seed):
    lattice, gradient = np.full(256, 7, dtype=np.uint8), np.full(4 * 256 * 2, 7.0)
    assert lib.crh_turbulence_tables(seed, lattice.ctypes.data_as(C.POINTER(C.c_uint8)), gradient.ctypes.data_as(C.POINTER(C.c_double))) == 0
    model_lattice, model_gradient = M.tables(seed)
    assert sorted(lattice.tolist()) == list(range(256)) and np.array_equal(lattice, model_lattice)
    assert np.array_equal(gradient.view(np.uint64), np.ascontiguousarray(model_gradient).reshape(-1).view(np.uint64))  # exact doubles, the sign of a zero included
    mirror_lattice, mirror_gradient = turbulence_tables(seed)
    assert np.array_equal(mirror_lattice, lattice) and mirror_gradient.shape == (4, 256, 2) and np.array_equal(mirror_gradient.reshape(-1), gradient)
    lengths = np.hypot(model_gradient[..., 0], model_gradient[..., 1])
    assert np.all((np.abs(lengths - 1.0) < 1e-15) | (lengths == 0.0))
    if seed == 346:
        assert tuple(gradient[(1 * 256 + 164) * 2:][:2]) == (0.0, 0.0)


def test_seeds_that_are_the_same():
    assert all(np.array_equal(a, b) for a, b in zip(turbulence_tables(0), turbulence_tables(1)))
    assert all(np.array_equal(a, b) for a, b in zip(turbulence_tables(-1), turbulence_tables(2)))
    assert all(np.array_equal(a, b) for a, b in zip(turbulence_tables(2147483647), turbulence_tables(2147483646)))
    assert not np.array_equal(turbulence_tables(1)[0], turbulence_tables(2)[0])
    assert np.array_equal(turbulence_texels(9, 5, 0.2, 3, 0), turbulence_texels(9, 5, 0.2, 3, 1)) and np.array_equal(turbulence_texels(9, 5, 0.2, 3, -1), turbulence_texels(9, 5, 0.2, 3, 2))
    assert not np.array_equal(turbulence_texels(9, 5, 0.2, 3, 1), turbulence_texels(9, 5, 0.2, 3, 2))


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("kind", M.KINDS, ids=["fractal", "turbulence"])
def test_the_library_and_the_python_mirror_equal_the_model(lib, kind, size):
    w, h = size
    for opaque, stitch, octaves, (frequency, offset) in itertools.product((False, True), (False, True), OCTAVES, PLACES):
        expect = M.turbulence(w, h, frequency, octaves, 346, kind, stitch, opaque, offset)
        what = (size, kind, opaque, stitch, octaves, frequency, offset)
        same(library(lib, w, h, frequency, octaves, 346, kind, stitch, opaque, offset), expect, what)
        same(turbulence_texels(w, h, frequency, octaves, 346, TurbulenceKind(kind), stitch, opaque, offset), expect, what)
        assert (expect[..., :3] <= expect[..., 3:]).all()  # rgb <= a


def test_the_widest_index_range(lib):
    """16384 texels at offsets of +-65536, frequencies at and just below 4, 12 octaves: the largest lattice coordinates, stitched and not."""
    for (w, h), stitch, corner in itertools.product(((16384, 2), (2, 16384)), (False, True), (1.0, -1.0)):
        offset = (65536.0 * corner, 65536.0 * corner)
        for frequency, kind, opaque in ((4.0, M.FRACTAL_NOISE, False), ((3.999, 3.7), M.TURBULENCE, True)):
            expect = M.turbulence(w, h, frequency, 12, 3, kind, stitch, opaque, offset)
            same(library(lib, w, h, frequency, 12, 3, kind, stitch, opaque, offset), expect, (w, h, stitch, offset, frequency))
            assert (len(np.unique(expect.reshape(-1, 4), axis=0)) == 1) == (frequency == 4.0)


def test_constant_images(lib):
    constants = {(M.FRACTAL_NOISE, False): (64, 64, 64, 128), (M.FRACTAL_NOISE, True): (128, 128, 128, 255), (M.TURBULENCE, False): (0, 0, 0, 0), (M.TURBULENCE, True): (0, 0, 0, 255)}
    for (kind, opaque), texel in constants.items():
        for stitch in (False, True):
            for frequency, octaves, offset in ((0.3, 0, (1.5, 2.5)), (0.0, 5, (1.5, 2.5)), ((2.0, 3.0), 12, (-7.0, 65536.0)), (4.0, 3, (0.0, 0.0)), (1.0, 1, (-65536.0, 11.0))):
                got = library(lib, 13, 9, frequency, octaves, 99, kind, stitch, opaque, offset)
                assert (got == np.array(texel, dtype=np.uint8)).all(), (kind, opaque, stitch, frequency, octaves, offset, got[0, 0])
        assert not (library(lib, 13, 9, 1.0, 2, 99, kind, False, opaque, (0.5, 0.0)) == np.array(texel, dtype=np.uint8)).all()  # a fractional offset is not a lattice point


def test_a_window_of_a_larger_image(lib):
    """Without stitch, a 10 x 7 piece at (20, 11) of a 40 x 30 image is the image of that size at the offset moved by (20, 11)."""
    for kind, opaque, offset in ((M.FRACTAL_NOISE, False, (3.0, -5.0)), (M.TURBULENCE, True, (-100.5, 64.25)), (M.TURBULENCE, False, (65000.0, -65000.0))):
        whole = library(lib, 40, 30, (0.05, 0.07), 6, 11, kind, False, opaque, offset)
        piece = library(lib, 10, 7, (0.05, 0.07), 6, 11, kind, False, opaque, (offset[0] + 20.0, offset[1] + 11.0))
        assert np.array_equal(piece, whole[11:18, 20:30]), (kind, opaque, offset)
        assert np.array_equal(whole, M.turbulence(40, 30, (0.05, 0.07), 6, 11, kind, False, opaque, offset))
        assert len(np.unique(whole.reshape(-1, 4), axis=0)) > 100


def test_a_stitched_image_repeats_with_its_size(lib):
    """64 x 32 at frequencies (0.05, 0.07), offsets (3, -5) against (67, 27): byte-equal when stitched, not otherwise."""
    for kind, opaque in itertools.product(M.KINDS, (False, True)):
        here = library(lib, 64, 32, (0.05, 0.07), 5, 7, kind, True, opaque, (3.0, -5.0))
        there = library(lib, 64, 32, (0.05, 0.07), 5, 7, kind, True, opaque, (67.0, 27.0))
        assert np.array_equal(here, there) and len(np.unique(here.reshape(-1, 4), axis=0)) > 100
        assert np.array_equal(here, M.turbulence(64, 32, (0.05, 0.07), 5, 7, kind, True, opaque, (3.0, -5.0)))
        plain = [library(lib, 64, 32, (0.05, 0.07), 5, 7, kind, False, opaque, o) for o in ((3.0, -5.0), (67.0, 27.0))]
        assert not np.array_equal(plain[0], plain[1])
        # the tile is seamless: the column behind the last one is the first one again
        wide = library(lib, 64, 32, (0.05, 0.07), 5, 7, kind, True, opaque, (3.0 + 63.0, -5.0))
        assert np.array_equal(wide[:, 1], here[:, 0])


def test_one_row_and_one_column(lib):
    """base_frequency[1] does not enter when height == 1 and offset[1] makes vy an integer; the same for x."""
    for kind, stitch in itertools.product(M.KINDS, (False, True)):
        rows = [library(lib, 37, 1, (0.11, fy), 4, 21, kind, stitch, False, (2.5, 0.0)) for fy in (0.0, 0.37, 4.0)]
        assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], rows[2]) and len(np.unique(rows[0].reshape(-1, 4), axis=0)) > 10
        columns = [library(lib, 1, 37, (fx, 0.11), 4, 21, kind, stitch, False, (0.0, 2.5)) for fx in (0.0, 0.37, 4.0)]
        assert np.array_equal(columns[0], columns[1]) and np.array_equal(columns[0], columns[2])


def test_errors_statuses_texts_and_untouched_outputs(lib):
    INVALID, NON_FINITE = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_NON_FINITE
    nan, inf = float("nan"), float("inf")
    cases = ((how_of(kind=2), INVALID, "kind is above CRH_TURBULENCE_TURBULENCE"), (how_of(stitch=2), INVALID, "stitch is neither 0 nor 1"), (how_of(opaque=2), INVALID, "opaque is neither 0 nor 1"),
             (how_of(octaves=13), INVALID, "octaves is above CRH_MAX_TURBULENCE_OCTAVES"), (how_of(base_frequency=(nan, 0.1)), NON_FINITE, "a frequency or an offset is not finite"),
             (how_of(base_frequency=(0.1, inf)), NON_FINITE, "a frequency or an offset is not finite"), (how_of(offset=(0.0, nan)), NON_FINITE, "a frequency or an offset is not finite"),
             (how_of(offset=(-inf, 0.0)), NON_FINITE, "a frequency or an offset is not finite"), (how_of(base_frequency=(-0.001, 0.1)), INVALID, "a base_frequency is outside [0, 4]"),
             (how_of(base_frequency=(0.1, 4.001)), INVALID, "a base_frequency is outside [0, 4]"), (how_of(offset=(65537.0, 0.0)), INVALID, "an offset is outside [-65536, 65536]"),
             (how_of(offset=(0.0, -65537.0)), INVALID, "an offset is outside [-65536, 65536]"),
             # the order: a bad enumerator before a non-finite field, a non-finite field before a range
             (how_of(kind=2, base_frequency=(nan, 0.1)), INVALID, "kind is above CRH_TURBULENCE_TURBULENCE"), (how_of(octaves=13, offset=(inf, 0.0)), INVALID, "octaves is above CRH_MAX_TURBULENCE_OCTAVES"),
             (how_of(base_frequency=(9.0, 0.1), offset=(nan, 0.0)), NON_FINITE, "a frequency or an offset is not finite"))
    out = np.full((3, 5, 4), 0xA5, dtype=np.uint8)
    handle = C.c_void_p(0x1234)
    for how, status, text in cases:
        assert lib.crh_turbulence_validate(C.byref(how)) == status, text
        assert lib.crh_last_error().decode() == "crh_turbulence_validate: " + text
        assert lib.crh_turbulence_texels(5, 3, C.byref(how), out.ctypes.data) == status and (out == 0xA5).all(), text
        assert lib.crh_last_error().decode() == "crh_turbulence_validate: " + text
        # (a refused crh_image_turbulence does not touch the device: the renderer is not looked at before the fields)
        assert lib.crh_image_turbulence(C.c_void_p(0x10), 5, 3, C.byref(how), C.byref(handle)) == status and handle.value == 0x1234, text
    good = how_of()
    assert lib.crh_turbulence_validate(C.byref(good)) == 0
    assert lib.crh_turbulence_validate(None) == INVALID and lib.crh_last_error().decode() == "crh_turbulence_validate: a null argument"
    assert lib.crh_turbulence_texels(5, 3, None, out.ctypes.data) == INVALID and lib.crh_turbulence_texels(5, 3, C.byref(good), None) == INVALID and (out == 0xA5).all()
    assert lib.crh_image_turbulence(None, 5, 3, C.byref(good), C.byref(handle)) == INVALID and handle.value == 0x1234
    assert lib.crh_image_turbulence(C.c_void_p(0x10), 5, 3, None, C.byref(handle)) == INVALID and handle.value == 0x1234
    assert lib.crh_image_turbulence(C.c_void_p(0x10), 5, 3, C.byref(good), None) == INVALID
    lattice, gradient = (C.c_uint8 * 256)(), (C.c_double * 2048)()
    assert lib.crh_turbulence_tables(1, None, gradient) == INVALID and lib.crh_turbulence_tables(1, lattice, None) == INVALID
    for w, h in ((0, 3), (5, 0), (16385, 1), (1, 16385)):
        assert lib.crh_turbulence_texels(w, h, C.byref(good), out.ctypes.data) == INVALID and (out == 0xA5).all()
        assert lib.crh_last_error().decode() == "crh_turbulence_validate: width and height lie in [1, 16384]"
        assert lib.crh_image_turbulence(C.c_void_p(0x10), w, h, C.byref(good), C.byref(handle)) == INVALID and handle.value == 0x1234
    # the limits themselves are served
    for how in (how_of(kind=1, octaves=12, base_frequency=(4.0, 0.0), offset=(65536.0, -65536.0), stitch=1, opaque=1), how_of(kind=0, octaves=0, seed=-2147483648)):
        assert lib.crh_turbulence_validate(C.byref(how)) == 0 and lib.crh_turbulence_texels(5, 3, C.byref(how), out.ctypes.data) == 0


def test_unaligned_bytes(lib):
    raw = np.full(7 * 3 * 4 + 3, 0xA5, dtype=np.uint8)
    how = how_of(kind=0, octaves=3, seed=9, base_frequency=(0.2, 0.3))
    assert lib.crh_turbulence_texels(7, 3, C.byref(how), raw.ctypes.data + 1) == 0
    assert np.array_equal(raw[1:-2].reshape(3, 7, 4), M.turbulence(7, 3, (0.2, 0.3), 3, 9, M.FRACTAL_NOISE)) and raw[0] == 0xA5 and (raw[-2:] == 0xA5).all()


def test_the_python_mirror(lib):
    assert np.array_equal(turbulence_texels(12, 5, 0.25), M.turbulence(12, 5, 0.25, 1, 0, M.TURBULENCE))  # the defaults; a scalar frequency serves both axes
    assert np.array_equal(turbulence_texels(12, 5, (0.25, 0.5), octaves=3, seed=4, kind=TurbulenceKind.FractalNoise, stitch=True, opaque=True, offset=(1.5, -2)),
                          M.turbulence(12, 5, (0.25, 0.5), 3, 4, M.FRACTAL_NOISE, True, True, (1.5, -2)))
    for bad in (dict(base_frequency=5.0), dict(base_frequency=0.1, octaves=13), dict(base_frequency=0.1, kind=2), dict(base_frequency=0.1, offset=(1e6, 0)), dict(base_frequency=float("nan"))):
        with pytest.raises(ContrastError):
            turbulence_texels(4, 4, **bad)
    for w, h in ((0, 4), (4, 16385)):
        with pytest.raises(ContrastError):
            turbulence_texels(w, h, 0.1)


def test_the_library_exports_and_the_mirrors_agree_across_header_python_and_ffi_rs(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    exports = open(b.write_export_map()).read()
    for name in NAMES:
        assert f"    {name};\n" in exports
    assert any(os.path.basename(h) == "turbulence.hpp" for h in b.header_deps())
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    assert re.search(r"CRH_TURBULENCE_FRACTAL_NOISE = 0, CRH_TURBULENCE_TURBULENCE = 1", header) and "#define CRH_MAX_TURBULENCE_OCTAVES 12u" in header
    assert C.sizeof(_ffi.TurbulenceC) == 9 * 4
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    assert committed == fresh
    for text in ("pub fn crh_turbulence_validate(how: *const crh_turbulence) -> crh_status;",
                 "pub fn crh_turbulence_tables(seed: i32, lattice: *mut u8, gradient: *mut f64) -> crh_status;",
                 "pub fn crh_turbulence_texels(width: u32, height: u32, how: *const crh_turbulence, out_rgba8: *mut c_void) -> crh_status;",
                 "pub fn crh_image_turbulence(renderer: *mut crh_renderer, width: u32, height: u32, how: *const crh_turbulence, out: *mut *mut crh_image) -> crh_status;",
                 "pub const CRH_TURBULENCE_TURBULENCE: u32 = 1;", "pub const CRH_MAX_TURBULENCE_OCTAVES: usize = 12;",
                 "pub struct crh_turbulence {\n    pub kind: u32,\n    pub octaves: u32,\n    pub seed: i32,\n    pub stitch: u32,\n    pub opaque: u32,\n    pub base_frequency: [f32; 2],\n"
                 "    pub offset: [f32; 2],\n}"):
        assert text in committed, text
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub enum TurbulenceKind {", "pub struct Turbulence {", "pub fn turbulence_validate(turbulence: &Turbulence) -> Result<(), Error>",
                 "pub fn turbulence_tables(seed: i32) -> Result<(Vec<u8>, Vec<f64>), Error>", "pub fn turbulence_texels(width: u32, height: u32, turbulence: &Turbulence) -> Result<Vec<u8>, Error>",
                 "pub fn turbulence(renderer: &Renderer, width: u32, height: u32, turbulence: &Turbulence) -> Result<Image, Error>"):
        assert text in shim, text
    for name in NAMES:
        assert f"ffi::{name}(" in shim, name
    mirror = open(os.path.join(ROOT, "include", "contrast_renderer.hpp")).read()
    for text in ("enum class TurbulenceKind : uint32_t {", "struct Turbulence {", "static Image turbulence(const Renderer& renderer, uint32_t width, uint32_t height, const Turbulence& turbulence)",
                 "inline std::vector<uint8_t> turbulence_texels(uint32_t width, uint32_t height,", "inline TurbulenceTables turbulence_tables(int32_t seed)"):
        assert text in mirror, text
    import contrast_renderer_amd
    for name in ("TurbulenceKind", "turbulence_texels", "turbulence_tables"):
        assert name in contrast_renderer_amd.__all__ and hasattr(contrast_renderer_amd, name)
    assert hasattr(contrast_renderer_amd.Image, "turbulence")


def test_the_cpp_mirror_of_turbulence_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "turbulence_harness.cpp"),
               "-o", os.path.join(tmp, "turbulence_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """A stand-alone program (its own main, no library, nothing loaded into python) around csrc/turbulence.hpp, the rule that crh_turbulence_texels
    runs: compiled as host code with the two sanitizers (the flag goes to the host compilation alone) and run once."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        binary = os.path.join(tmp, "turbulence_sanitize")
        # -x c++ and -Xarch_host: plain host C++, the sanitizers on the host alone (no device pass; clang links the sanitizers' runtime statically, so the program needs nothing preloaded)
        cmd = [hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
               "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), "-I", os.path.join(ROOT, "contrast_renderer_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "turbulence_sanitize.cpp"), "-o", binary]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert re.search(r"\d+ texels, 0 failures$", done.stdout.strip())
