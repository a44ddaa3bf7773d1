"""Conic gradient paints without a GPU: crh_paint_validate (host only), the Python / C++ / Rust mirrors, csrc/paint_angle.hpp through its stand-alone
program against float64 atan2, and the float64 model of tests/test_gpu_conic.py run alone on the scenes those tests draw."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, GradientStop, Paint, Spread, _ffi
from contrast_renderer_amd import renderer as R

import conic_model as CM

ROOT = CM.ROOT
RED, BLUE = (1.0, 0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 0.5)
TURN32 = np.float32(2.0 * math.pi)  # the f32 nearest to 2 pi
QUARTER32 = np.float32(0.5 * math.pi)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def raw(kind=4, spread=0, p0=(0.0, 0.0), p1=(0.0, float(TURN32)), stops=((0.0, RED), (1.0, BLUE))):
    c = _ffi.PaintC()
    c.kind, c.spread, c.n_stops = kind, spread, len(stops)
    c.p0[0], c.p0[1], c.p1[0], c.p1[1] = p0[0], p0[1], p1[0], p1[1]
    for i, (o, col) in enumerate(stops):
        c.stops[i].offset = o
        for ch in range(4):
            c.stops[i].color[ch] = col[ch]
    return c


def _from(start, sweep):
    """(start, end) in f32 with end - start = the f32 `sweep` where the sum is exact in f32 (asserted)."""
    start, end = np.float32(start), np.float32(np.float32(start) + np.float32(sweep))
    assert np.float64(end) - np.float64(start) == np.float64(np.float32(sweep))
    return float(start), float(end)


VALID = {
    "a full turn": raw(p1=(0.0, 2.0 * math.pi)),  # (rounded to f32 by the struct: the f32 nearest to 2 pi)
    "the f32 nearest to 2 pi": raw(p1=(0.0, float(TURN32))),
    "the f32 nearest to 2 pi, clockwise": raw(p1=(0.0, -float(TURN32))),
    "a quarter turn": raw(p1=(1.0, 1.0 + 0.5 * math.pi), spread=2),
    "a negative sweep": raw(p1=(2.0, -1.0), spread=1),
    "a start of 100 rad": raw(p1=(100.0, 103.0)),
    "a start of -100 rad": raw(p1=(-100.0, -101.5)),
    "a full turn from -4 rad": raw(p1=_from(-4.0, TURN32)),
}
INVALID = {
    "sweep 0": raw(p1=(1.25, 1.25)),
    "sweep 0 at 0": raw(p1=(0.0, -0.0)),
    "just above f32(2 pi)": raw(p1=(0.0, float(np.nextafter(TURN32, np.float32(7.0))))),
    "just below -f32(2 pi)": raw(p1=(0.0, -float(np.nextafter(TURN32, np.float32(7.0))))),
    "just above f32(2 pi) from -4 rad": raw(p1=_from(-4.0, np.nextafter(TURN32, np.float32(7.0)))),
    "two turns": raw(p1=(-6.0, 6.5)),
    "a sweep whose k overflows": raw(p1=(0.0, 1e-45)),
    "kind 5": raw(kind=5),
    "kind 3": raw(kind=3),
    "unknown spread": raw(spread=3),
}
NON_FINITE = {
    "start nan": raw(p1=(float("nan"), 1.0)),
    "end nan": raw(p1=(0.0, float("nan"))),
    "start inf": raw(p1=(float("inf"), 1.0)),
    "end -inf": raw(p1=(0.0, float("-inf"))),
    "centre nan": raw(p0=(float("nan"), 0.0)),
    "centre inf": raw(p0=(0.0, float("inf"))),
}


@pytest.mark.parametrize("name", sorted(VALID))
def test_validate_accepts(lib, name):
    assert lib.crh_paint_validate(C.byref(VALID[name])) == _ffi.OK, lib.crh_last_error().decode()


@pytest.mark.parametrize("name", sorted(INVALID))
def test_validate_refuses_with_invalid_argument_and_a_text(lib, name):
    assert lib.crh_paint_validate(C.byref(INVALID[name])) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode().startswith("crh_paint: ")


@pytest.mark.parametrize("name", sorted(NON_FINITE))
def test_validate_refuses_a_non_finite_field(lib, name):
    assert lib.crh_paint_validate(C.byref(NON_FINITE[name])) == _ffi.ERR_NON_FINITE


def test_python_conic_paint_round_trips_field_for_field(lib):
    stops = [GradientStop(0.0, RED), GradientStop(0.25, BLUE), GradientStop(0.25, RED), GradientStop(1.0, (0.5, 0.25, 0.125, 1.0))]
    for paint in (Paint.conic((0.5, -1.0), 0.25, 3.0, stops, Spread.Reflect), Paint.conic((0.25, 0.75), 1.5, -0.5, stops[:1], Spread.Repeat),
                  Paint.conic((0, 0), 0, 1, [(0.0, RED), (1.0, BLUE)])):
        c = paint.to_c()
        assert (c.kind, c.spread, c.n_stops) == (4, int(paint.spread), len(paint.stops))
        assert (tuple(c.p0), tuple(c.p1)) == (paint.p0, paint.p1)
        for i, s in enumerate(paint.stops):
            assert c.stops[i].offset == s.offset and tuple(c.stops[i].color) == tuple(s.color)
        paint.validate()
    assert int(R.PaintKind.Conic) == 4 and C.sizeof(_ffi.PaintC) == 188
    assert Paint.conic((1, 2), 3, 4, [(0.5, RED)]).p1 == (3.0, 4.0) and Paint.conic((1, 2), 3, 4, [(0.5, RED)]).spread == Spread.Pad
    for start, end in ((1.0, 1.0), (0.0, 7.0)):
        with pytest.raises(ContrastError):
            Paint.conic((0, 0), start, end, [(0.0, RED)]).validate()


def test_the_rust_bindings_and_the_shim_carry_the_kind():
    ffi = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    assert "pub const CRH_PAINT_CONIC: u32 = 4;" in ffi
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    assert "pub fn conic(center: [f32; 2], start: f32, end: f32, stops: &[(f32, [f32; 4])], spread: Spread) -> Self" in shim


def test_the_cpp_mirror_of_conic_paints_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "conic_harness.cpp"),
               "-o", os.path.join(tmp, "conic_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


# ---------------------------------------------------------------- the angle: csrc/paint_angle.hpp alone, on the host, against float64 atan2

def circular(got, y, x):
    """|got - atan2(y, x) / 2 pi| in turns, round the circle (1 and 0 are one angle), in float64."""
    ref = np.arctan2(np.float64(y) + 0.0, np.float64(x) + 0.0) / CM.TURN  # (-0 + 0 = +0: a zero of either sign counts as +0)
    ref = np.where(ref < 0.0, ref + 1.0, ref)
    d = np.abs(np.float64(got) - ref)
    return np.minimum(d, 1.0 - d)


def test_paint_turns_is_within_its_stated_bound_of_atan2_and_exact_on_the_axes():
    bound = CM.angle_bound()
    assert 0.0 < bound < 2.0 ** -22  # (a bound of many ulp of 1 would say nothing)
    pairs = np.concatenate([CM.special_pairs(), CM.dense_pairs(), CM.random_pairs(65536)])
    with tempfile.TemporaryDirectory() as tmp:
        program = CM.build_angle_program(tmp)
        got = CM.host_turns(program, pairs, tmp)
        magnitudes = [np.float32(2.0 ** e) for e in (-149, -126, -1, 0, 3, 24)] + [np.float32(3e38), np.float32(1.1)]
        axes = np.float32([q for m in magnitudes for zero in (0.0, -0.0) for q in ((zero, m), (m, zero), (zero, -m), (-m, zero))])
        on_axes = CM.host_turns(program, axes, tmp)
        measured = subprocess.run([program, "--measure", "500"], capture_output=True, text=True)  # the program's own sweep, against its own atan2
        assert measured.returncode == 0, measured.stdout
    y, x = pairs[:, 0], pairs[:, 1]
    assert np.isfinite(got).all() and (got >= 0.0).all() and (got < 1.0).all()
    err = circular(got, y, x)
    worst = int(np.argmax(err))
    print(f"paint_turns: {len(pairs)} pairs, worst {err[worst]:.3e} turns at y {float(y[worst])!r} x {float(x[worst])!r}, bound {bound:.3e}; {measured.stdout.strip()}")
    assert err[worst] <= bound
    # every octant and every magnitude is in the set
    octant = (np.abs(y) > np.abs(x)).astype(int) + 2 * (x < 0) + 4 * (y < 0)
    assert all((octant == k).sum() > 10000 for k in range(8))
    assert np.abs(pairs).max() == 2.0 ** 24 and 0 < np.abs(pairs)[pairs != 0].min() <= 2.0 ** -140
    # the axes exactly, a zero of either sign counting as +0; the origin
    assert np.array_equal(on_axes, np.tile(np.float32([0.0, 0.25, 0.5, 0.75]), len(axes) // 4))
    origin = (y == 0) & (x == 0)
    assert origin.sum() == 4 and (got[origin] == 0.0).all()
    below = (y == -np.float32(2.0 ** -149)) & (x >= 1.0)  # 1 - tiny rounds to 1: folded back to 0
    assert below.sum() >= 5 and (got[below] == 0.0).all()


# ---------------------------------------------------------------- the float64 model alone

def test_the_model_is_the_definition_taken_one_sample_at_a_time():
    rng = np.random.RandomState(2)
    paints = [CM.random_conic(rng, f, s, clockwise=cw) for f in (1.0, 1.0 / 3.0, 0.25) for s in CM.SPREADS for cw in (False, True)]
    paints += [Paint.conic((0.25, -0.5), 100.0, 103.0, [(0.0, RED), (1.0, BLUE)]), Paint.conic((0.0, 0.0), -100.0, -101.5, [(0.0, RED), (1.0, BLUE)])]
    p = rng.uniform(-2.0, 2.0, (64, 2))
    for paint in paints:
        p[:4] = np.float64(np.float32(paint.p0)) + [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]
        t = CM.raw_t(paint, p)
        one = np.array([CM.t_of_one_sample(paint, *q) for q in p])
        assert np.allclose(t, one, rtol=0.0, atol=1e-12)  # (two libraries' atan2: an ulp of float64 apart)
        s, k, direction = CM.table(paint)
        assert 0.0 <= s <= 1.0 and k >= 1.0 - 2.0 ** -24 and (t >= 0.0).all() and (t <= k).all()
    # the corners of the contract: a full turn from 0 has t = the angle in turns; the axes of a quarter turn from pi / 2; clockwise mirrors it
    axes = np.array([(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)])
    wheel = Paint.conic((0, 0), 0.0, float(TURN32), [(0.0, RED), (1.0, BLUE)])
    assert np.allclose(CM.raw_t(wheel, axes), [0.0, 0.25, 0.5, 0.75], rtol=0, atol=1e-7)
    wedge = Paint.conic((0, 0), float(QUARTER32), float(np.float32(math.pi)), [(0.0, RED), (1.0, BLUE)])
    assert np.allclose(CM.raw_t(wedge, axes), [3.0, 0.0, 1.0, 2.0], rtol=0, atol=1e-6)
    back = Paint.conic((0, 0), float(QUARTER32), 0.0, [(0.0, RED), (1.0, BLUE)])
    assert np.allclose(CM.raw_t(back, axes), [1.0, 0.0, 3.0, 2.0], rtol=0, atol=1e-6)
    src, near = CM.conic_source(wedge, (1, 1, 1, 1), np.array([(-1.0, 1.0), (-1.0, -1.0)]), 1e-6)
    assert not near.any() and np.allclose(src[0], [0.5 * 0.75, 0.0, 0.5 * 0.75, 0.75]) and np.allclose(src[1], [0.0, 0.0, 0.5, 0.5])  # PAD holds the last stop
    wedge_repeat = Paint.conic((0, 0), float(QUARTER32), float(np.float32(math.pi)), [(0.0, RED), (1.0, BLUE)], Spread.Repeat)
    src, _ = CM.conic_source(wedge_repeat, (1, 1, 1, 1), np.array([(-1.0, -1.0)]), 1e-6)
    assert np.allclose(src[0], [0.5 * 0.75, 0.0, 0.5 * 0.75, 0.75], atol=1e-6)  # the wedge again: t = 1.5 -> 0.5


def test_the_model_leaves_at_most_a_tenth_of_every_scene_out():
    from test_gpu_blending import random_background
    background = random_background(CM.SIZE)
    for name, (shapes, transforms, colours, regions, paints), counts in CM.gpu_scenes():
        conics = [p for p in paints if CM.is_conic(p)]
        assert conics and all(sum(a.offset == b.offset for a, b in zip(p.stops[:-1], p.stops[1:])) <= 1 for p in conics), name
        for p in conics:
            p.validate()
        for msaa in counts:
            expect, ok, extra, left_out = CM.model(CM.SIZE, msaa, transforms, colours, regions, paints, CM.OVER, False, background)
            print(f"{name} msaa {msaa}: extra {extra * 255:.3f}/255, left out {left_out:.3%}, checkable {ok.mean():.3f}")
            assert extra < 0.25 / 255.0 and left_out <= 0.10 and ok.mean() > 0.5, (name, msaa, extra * 255, left_out, ok.mean())
            assert np.isfinite(expect).all() and (expect >= 0).all() and (expect <= 1).all()
