"""Gradient paints without a GPU: crh_paint_validate (host only), the Python / C++ / Rust mirrors of the new ABI, and the float64 model of
tests/test_gpu_paints.py run alone on the scenes those tests draw."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, GradientStop, Paint, Spread, _ffi
from contrast_renderer_amd import renderer as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RED, BLUE = (1.0, 0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 0.5)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def raw(kind=1, spread=0, p0=(0.0, 0.0), p1=(1.0, 0.0), stops=((0.0, RED), (1.0, BLUE)), n_stops=None):
    c = _ffi.PaintC()
    c.kind, c.spread, c.n_stops = kind, spread, len(stops) if n_stops is None else n_stops
    c.p0[0], c.p0[1], c.p1[0], c.p1[1] = p0[0], p0[1], p1[0], p1[1]
    for i, (o, col) in enumerate(stops):
        c.stops[i].offset = o
        for ch in range(4):
            c.stops[i].color[ch] = col[ch]
    return c


INVALID = {
    "unknown kind": raw(kind=3),
    "kind 0": raw(kind=0),
    "unknown spread": raw(spread=3),
    "no stops": raw(n_stops=0),
    "nine stops": raw(n_stops=9),
    "decreasing offsets": raw(stops=((0.5, RED), (0.25, BLUE))),
    "offset below 0": raw(stops=((-0.25, RED), (1.0, BLUE))),
    "offset above 1": raw(stops=((0.0, RED), (1.5, BLUE))),
    "linear p0 == p1": raw(p0=(0.5, 0.5), p1=(0.5, 0.5)),
    "radius 0": raw(kind=2, p1=(0.0, 0.0)),
    "radius < 0": raw(kind=2, p1=(-1.0, 0.0)),
}
NON_FINITE = {
    "p0": raw(p0=(float("nan"), 0.0)),
    "p1": raw(p1=(float("inf"), 0.0)),
    "offset": raw(stops=((float("nan"), RED), (1.0, BLUE))),
    "colour": raw(stops=((0.0, (1.0, float("inf"), 0.0, 1.0)), (1.0, BLUE))),
    "radius": raw(kind=2, p1=(float("nan"), 0.0)),
}
VALID = {
    "one stop": raw(stops=((0.5, RED),)),
    "eight stops": raw(stops=tuple((i / 7.0, RED if i % 2 else BLUE) for i in range(8))),
    "hard stop": raw(stops=((0.0, RED), (0.5, RED), (0.5, BLUE), (1.0, BLUE))),
    "offsets 0 and 1": raw(stops=((0.0, RED), (1.0, BLUE))),
    "radial reflect": raw(kind=2, spread=2, p1=(0.25, 0.0)),
    "colours out of range": raw(stops=((0.0, (2.0, -1.0, 0.0, 1.0)), (1.0, BLUE))),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_validate_refuses_with_invalid_argument_and_a_text(lib, name):
    assert lib.crh_paint_validate(C.byref(INVALID[name])) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode().startswith("crh_paint: ")


@pytest.mark.parametrize("name", sorted(NON_FINITE))
def test_validate_refuses_a_non_finite_field(lib, name):
    assert lib.crh_paint_validate(C.byref(NON_FINITE[name])) == _ffi.ERR_NON_FINITE


@pytest.mark.parametrize("name", sorted(VALID))
def test_validate_accepts(lib, name):
    assert lib.crh_paint_validate(C.byref(VALID[name])) == _ffi.OK


def test_python_paint_round_trips_field_for_field(lib):
    stops = [GradientStop(0.0, RED), GradientStop(0.25, BLUE), GradientStop(0.25, RED), GradientStop(1.0, (0.5, 0.25, 0.125, 1.0))]
    for paint in (Paint.linear((0.5, -1.0), (2.0, 3.0), stops, Spread.Reflect), Paint.radial((0.25, 0.75), 1.5, stops[:1], Spread.Repeat),
                  Paint.linear((0, 0), (1, 1), [(0.0, RED), (1.0, BLUE)])):
        c = paint.to_c()
        assert (c.kind, c.spread, c.n_stops) == (int(paint.kind), int(paint.spread), len(paint.stops))
        assert (tuple(c.p0), tuple(c.p1)) == (paint.p0, paint.p1)
        for i, s in enumerate(paint.stops):
            assert c.stops[i].offset == s.offset and tuple(c.stops[i].color) == tuple(s.color)
        paint.validate()
    assert C.sizeof(_ffi.PaintC) == 4 * (2 + 4 + 1 + 8 * 5) and int(R.PaintKind.Radial) == 2 and int(Spread.Reflect) == 2
    with pytest.raises(ContrastError):
        Paint.linear((0, 0), (0, 0), [(0.0, RED)]).validate()
    with pytest.raises(ContrastError):
        Paint.linear((0, 0), (1, 0), [(i / 8.0, RED) for i in range(9)]).to_c()


def test_the_library_exports_and_the_rust_bindings_declare_the_new_symbols(lib):
    for name in ("crh_paint_validate", "crh_scene_set_paints"):
        assert getattr(lib, name) is not None
    ffi = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    assert re.search(r"pub fn crh_paint_validate\(paint: \*const crh_paint\) -> crh_status;", ffi)
    assert re.search(r"pub fn crh_scene_set_paints\(scene: \*mut crh_scene, paints: \*const crh_paint, n_paints: u32, instance_paint: \*const i32, n_instances: u32\) -> crh_status;", ffi)
    assert "pub struct crh_paint {" in ffi and "pub stops: [crh_gradient_stop; 8]," in ffi
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    assert "pub fn set_paints(&self, paints: &[Paint], instance_paint: &[i32]) -> Result<(), Error>" in shim


def test_the_cpp_mirror_of_paints_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "paints_harness.cpp"),
               "-o", os.path.join(tmp, "paints_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


# ---------------------------------------------------------------- the float64 model alone, on every scene the GPU tests draw

def _gpu_scenes():
    """Every scene tests/test_gpu_paints.py holds against the model, with the sample counts it draws them at."""
    import paint_model as M
    out = [(f"{kind.name}-{spread.name}", M.scene(kind, spread), (1, 2, 4, 8)) for kind, spread in M.SCENES]
    out.append(("srgb", M.scene(R.PaintKind.Linear, Spread.Reflect, seed=9), (4,)))
    out.append(("blend-states", M.scene(R.PaintKind.Radial, Spread.Reflect, seed=6), (4,)))
    out.append(("sweep", M.sweep_scene(), (4,)))
    _, _, transforms, colours, _, regions, paints, _ = M.recorded_scene()
    out.append(("recorded", (None, transforms, colours, regions, paints), (4,)))
    return out


def test_the_model_leaves_more_than_half_of_every_scene_checkable():
    import paint_model as M
    from test_gpu_blending import random_background
    over = R.ColorTargetState(R.BlendState.PREMULTIPLIED_ALPHA_BLENDING)
    background = random_background(128)
    for name, (shapes, transforms, colours, regions, paints), counts in _gpu_scenes():
        painted = [(p, t) for p, t in zip(paints, transforms) if p is not None]
        assert all(sum(a.offset == b.offset for a, b in zip(p.stops[:-1], p.stops[1:])) <= 1 for p, _ in painted), name
        assert all(M.length_px(p, t, 128) >= 16.0 for p, t in painted), name
        if name != "sweep":  # (the issue's "about 20 random paints" is the one scene above 12 shapes)
            assert len(transforms) <= 12
        for msaa in counts:
            expect, ok, extra = M.model(128, msaa, transforms, colours, regions, paints, over, False, background)
            assert ok.mean() > 0.5, (name, msaa, ok.mean())
            assert extra < 0.25 / 255.0 and np.isfinite(expect).all() and (expect >= 0).all() and (expect <= 1).all()


def test_the_model_follows_the_contract_at_its_corners():
    import paint_model as M
    hard = Paint.linear((0, 0), (1, 0), [(0.0, RED), (0.5, RED), (0.5, BLUE), (1.0, BLUE)])
    t = np.array([-1.0, 0.0, 0.25, 0.5, 0.75, 1.0, 2.0])
    assert np.array_equal(M.stop_colour(hard, M.spread_t(t, Spread.Pad)), np.float64([RED, RED, RED, BLUE, BLUE, BLUE, BLUE]))  # at the shared offset the later stop wins
    assert np.allclose(M.spread_t(np.array([-0.25, 1.25, 2.5]), Spread.Repeat), [0.75, 0.25, 0.5])
    assert np.allclose(M.spread_t(np.array([-0.25, 1.25, 2.5, 3.75]), Spread.Reflect), [0.25, 0.75, 0.5, 0.25])
    same = Paint.radial((0, 0), 1.0, [(0.0, (0.3, 0.6, 0.9, 0.7)), (0.4, (0.3, 0.6, 0.9, 0.7)), (1.0, (0.3, 0.6, 0.9, 0.7))])
    assert (M.stop_colour(same, np.linspace(0, 1, 33)) == np.float64(np.float32([0.3, 0.6, 0.9, 0.7]))).all()
    ramp = Paint.linear((1.0, 1.0), (3.0, 1.0), [(0.0, (0, 0, 0, 1)), (1.0, (1, 1, 1, 1))])
    assert np.allclose(M.raw_t(ramp, np.array([[1.0, 5.0], [2.0, 0.0], [4.0, 1.0]])), [0.0, 0.5, 1.5])
