"""Conic gradient paints of the colour cover (include/contrast_hip.h, crh_scene_set_paints: CRH_PAINT_CONIC) on the GPU: the device's angle bit for
bit against the host's, quadrants byte for byte, and the paint block of k_raster_paint / k_raster_image against the float64 model of
tests/conic_model.py."""
import math
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import Path, batch_from_shapes
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import GradientStop, Paint, PaintKind, Spread

import conic_model as CM
import ground_truth_util as G
import paint_model as M
from test_gpu_blending import STATES, compare, last_pass, no_pins, random_background, stack, tolerance  # noqa: F401
from test_gpu_image_paints import draw  # (the gradient tests' draw with image paints put on the device)
from test_ground_truth import place

pytestmark = pytest.mark.gpu

OVER = CM.OVER
SIZE = CM.SIZE


def tol_of(name, attachment, extra):
    """tolerance() of the blending tests plus what the f32 error of t moves the source by: the largest colour slope per unit t of the scene's
    paints times the t error (conic_model's docstring derives it; paint_model's for the other kinds). The scenes keep it below a quarter unit."""
    assert extra < 0.25 / 255.0, extra * 255
    return tolerance(name, attachment) + extra


def against_model(name, scene, msaa, attachment, state_name="over", background=None):
    shapes, transforms, colours, regions, paints = scene
    fmt = R.FORMAT_RGBA8_ATTACHMENT if attachment else R.FORMAT_RGBA8
    state = OVER if state_name == "over" else STATES[state_name]
    config = R.Configuration(msaa_sample_count=msaa) if state_name == "over" else R.Configuration(msaa_sample_count=msaa, blending=state)
    image, tap = draw(config, batch_from_shapes(shapes), transforms, colours, paints, fmt, background)
    assert tap["raster"] == "ops", tap
    expect, ok, extra, left_out = CM.model(SIZE, msaa, transforms, colours, regions, paints, state, attachment, np.zeros((SIZE, SIZE, 4)) if background is None else background)
    print(f"{name} msaa {msaa}: extra {extra * 255:.3f}/255, left out {left_out:.3%}")
    assert left_out <= 0.10, left_out
    compare(image, expect, ok, tol_of(state_name, attachment, extra), f"{name} msaa {msaa}")


# ---------------------------------------------------------------- 1. the device's angle is the host's, bit for bit

def test_paint_turns_on_the_device_equals_the_host_bit_for_bit(no_pins):
    pairs = CM.special_pairs()
    pairs = np.concatenate([pairs, CM.random_pairs(65536 - len(pairs))])
    assert pairs.shape == (65536, 2)
    with tempfile.TemporaryDirectory() as tmp:
        host = CM.host_turns(CM.build_angle_program(tmp), pairs, tmp)
    r = R.Renderer(R.Configuration(), device=0)
    device = r.selftest_fmath(10, np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1]))
    differ = device.view(np.uint32) != host.view(np.uint32)
    assert not differ.any(), f"{int(differ.sum())} of {len(pairs)} differ, the first at (y, x) = {pairs[differ][0]!r}: device {device[differ][0]!r}, host {host[differ][0]!r}"


# ---------------------------------------------------------------- 2. quadrants, byte for byte

QUADRANT_COLOURS = [(1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0), (1.0, 1.0, 0.0, 1.0)]


def quadrants(transform, paint, msaa):
    """One square under `transform`, painted -> (image, the pixels more than a pixel inside the square and more than a pixel off both axes
    through its centre [H, W], their position in path coordinates [H W, 2])."""
    batch = batch_from_shapes([([], [Path.from_rect((0.0, 0.0), (1.0, 1.0))])])
    white = np.float32([[1.0, 1.0, 1.0, 1.0]])
    image, tap = draw(R.Configuration(msaa_sample_count=msaa), batch, transform.reshape(1, 16), white, [paint])
    assert tap["raster"] == "ops", tap
    p = G.to_path(G.pixel_centres(SIZE), transform, SIZE, SIZE)
    scale = G.min_pixel_scale(transform, SIZE, SIZE)
    margin = 1.5 / scale  # (a pixel, and the half pixel between a pixel's centre and its samples)
    checked = (np.abs(p) < 1.0 - margin).all(axis=1) & (np.abs(p) > margin).all(axis=1)
    return image, checked.reshape(SIZE, SIZE), p


def quadrant_bytes(p, start_quadrant, clockwise, colours):
    """The colour bytes at path positions p, from the definition: the quadrant of the angle from the start ray, counted in the sweep's direction."""
    q = (np.floor(np.arctan2(p[:, 1], p[:, 0]) / (0.5 * math.pi)).astype(int) - start_quadrant) % 4  # counter-clockwise from the start axis
    if clockwise:
        q = 3 - q
    return np.uint8(np.float64(colours)[q] * 255.0).reshape(SIZE, SIZE, 4)


@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirrored"])
@pytest.mark.parametrize("msaa", [1, 4])
def test_quadrants_hold_their_colour_byte_for_byte(msaa, mirror, no_pins):
    """The centre on a pixel corner, four opaque colours with hard stops at 0.25, 0.5 and 0.75: direction, octant and y-flip mistakes that a
    tolerance can hide show as a whole quadrant of the wrong colour."""
    transform = place(SIZE, SIZE, 64, 64, 40, mirror=mirror)
    images = {}
    for name, start_quadrant, clockwise in (("from 0", 0, False), ("from pi/2", 1, False), ("clockwise from 0", 0, True), ("clockwise from pi/2", 1, True)):
        paint = CM.quadrant_paint(start_quadrant * 0.5 * math.pi, clockwise, QUADRANT_COLOURS)
        image, checked, p = quadrants(transform, paint, msaa)
        assert checked.sum() > 4 * 30 * 30
        expect = quadrant_bytes(p, start_quadrant, clockwise, QUADRANT_COLOURS)
        assert all((expect[checked] == np.uint8(np.float64(c) * 255.0)).all(axis=1).sum() > 30 * 30 for c in QUADRANT_COLOURS)
        assert np.array_equal(image[checked], expect[checked]), f"{name}: {int((image != expect).any(axis=2)[checked].sum())} pixels differ"
        images[name] = image
        if clockwise:  # the negative sweep reads the same stops clockwise: the positive sweep with the stop order reversed
            reverse, _, _ = quadrants(transform, CM.quadrant_paint(start_quadrant * 0.5 * math.pi, False, QUADRANT_COLOURS[::-1]), msaa)
            assert np.array_equal(image[checked], reverse[checked]), name
    assert not np.array_equal(images["from 0"], images["from pi/2"]) and not np.array_equal(images["from 0"], images["clockwise from 0"])


# ---------------------------------------------------------------- 3. a paint whose stops all carry the instance's colour is that colour, byte for byte

@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("fmt", [R.FORMAT_RGBA8, R.FORMAT_RGBA8_ATTACHMENT], ids=["rgba8", "attachment"])
def test_stops_of_one_colour_equal_the_oracle_image_of_the_solid_scene(msaa, fmt, no_pins):
    from oracle.binding import Oracle, render_pass
    shapes, transforms, colours, _ = stack(seed=7, size=SIZE, n=12, radius=(16, 36))
    batch = batch_from_shapes(shapes)
    rng = np.random.RandomState(3)
    paints = []
    for i, c in enumerate(colours):
        stops = [GradientStop(float(o), tuple(float(v) for v in c)) for o in np.linspace(0, 1, 1 + i % 8)] if i % 8 else [GradientStop(0.5, tuple(float(v) for v in c))]
        base = CM.random_conic(rng, (1.0, 1.0 / 3.0, 0.25)[i % 3], CM.SPREADS[i % 3], n_stops=2, clockwise=bool(i % 2))
        paints.append(Paint(base.kind, base.spread, base.p0, base.p1, tuple(stops)))
    white = np.ones_like(colours)
    image, tap = draw(R.Configuration(msaa_sample_count=msaa), batch, transforms, white, paints, fmt)
    assert tap["general"] == 1 and tap["raster"] == "ops", tap
    draws = [(i, i, op, 0, 0) for i in range(len(colours)) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)]
    expect, _ = render_pass(Oracle(batch), SIZE, SIZE, msaa, 4, 4, 0, transforms, colours, draws, attachment8=fmt == R.FORMAT_RGBA8_ATTACHMENT)
    assert np.array_equal(image, expect), f"{int((image != expect).any(axis=2).sum())} pixels differ"


# ---------------------------------------------------------------- 4. the model: sweeps x spreads x msaa over a random background

@pytest.mark.parametrize("sweep,spread,msaa", [(name, spread, msaa) for name, spread in CM.GRID for msaa in CM.MSAA_OF_GRID[(name, spread)]],
                         ids=lambda v: v.name if isinstance(v, Spread) else str(v))
def test_conic_gradients_match_the_float64_model(sweep, spread, msaa, no_pins):
    attachment = (len(sweep) + int(spread) + msaa) % 2 == 1  # both frame formats over the grid
    against_model(f"{sweep} {spread.name}", CM.scene(sweep, spread), msaa, attachment, background=random_background(SIZE))


# ---------------------------------------------------------------- 5. one case each: sRGB, a blend state, a camera, strokes

def test_conic_gradients_on_a_bgra8_srgb_target(no_pins):
    shapes, transforms, colours, regions, paints = CM.scene("third", Spread.Reflect, seed=9)
    image, tap = draw(R.Configuration(msaa_sample_count=4), batch_from_shapes(shapes), transforms, colours, paints, R.FORMAT_BGRA8_SRGB)
    expect, ok, extra, left_out = CM.model(SIZE, 4, transforms, colours, regions, paints, OVER, False, np.zeros((SIZE, SIZE, 4)))
    assert extra < 0.25 / 255.0 and left_out <= 0.10
    tol = 512 * G.F32_ULP + extra
    got = image[..., [2, 1, 0, 3]].astype(np.float64)
    lo, hi = M.srgb_decode(np.maximum(got[..., :3] - 0.5, 0.0)) - tol, M.srgb_decode(np.minimum(got[..., :3] + 0.5, 255.0)) + tol
    bad = ok & (((expect[..., :3] < lo) | (expect[..., :3] > hi)).any(axis=2) | (np.abs(got[..., 3] / 255.0 - expect[..., 3]) > 0.5 / 255.0 + tol))
    assert not bad.any(), int(bad.sum())
    assert ok.mean() > 0.5 and (expect[..., 3][ok] > 0).mean() > 0.2


def test_conic_paints_blend_with_the_renderers_state(no_pins):
    against_model("additive", CM.scene("quarter", Spread.Repeat, seed=6), 4, True, "additive", random_background(SIZE, seed=3))


@pytest.mark.parametrize("msaa", [1, 4])
def test_a_conic_painted_blob_under_a_camera_matches_the_unprojected_position(msaa, no_pins):
    """The gradient tests' blob under its tilted camera. The centre lies outside the blob, which spans less than the quarter turn of the sweep:
    neither the centre nor the start ray is on it, and the arc of a unit of t is bounded below over it — from the model itself, as there."""
    from test_perspective_ground_truth import CASES, blob, camera, ground_truth
    size = 96
    m = np.float32(camera(**CASES["tilted"])).reshape(16)
    paint = Paint.conic((-1.6, -1.4), 0.0, 0.5 * math.pi, [(0.0, (1.0, 0.2, 0.1, 1.0)), (0.4, (0.1, 0.9, 0.3, 0.8)), (0.4, (0.9, 0.9, 0.1, 1.0)), (1.0, (0.2, 0.3, 1.0, 1.0))], Spread.Pad)
    colour = np.float32([[1.0, 0.9, 0.8, 0.9]])
    config = R.Configuration(msaa_sample_count=msaa, depth_compare=R.Compare.Less, depth_write_enabled=True)
    r = R.Renderer(config, device=0)
    scene = R.Scene(r, batch_from_shapes([([], [blob()])]))
    scene.set_paints([paint], [0])
    frame = R.Frame(r, size, size)
    frame.clear()
    frame.clear_depth(1.0)
    scene.render(frame, m.reshape(1, 16), colour)
    image = frame.download()
    offsets = G.SAMPLE_OFFSETS[msaa] - 0.5
    pix = G.pixel_centres(size)
    corners = M.to_path_h(np.array([[0.0, 0.0], [size, 0.0], [0.0, size], [size, size]], dtype=np.float64), m, size)
    # pixels per unit of t, from the model itself: the largest step of t between neighbouring covered pixels bounds the local length of a unit
    t = CM.raw_t(paint, M.to_path_h(pix, m, size)).reshape(size, size)
    covered = ground_truth(blob(), m, size, [(0.0, 0.0)])[0].reshape(size, size)
    step = max(np.abs(np.diff(t, axis=0))[covered[1:] & covered[:-1]].max(), np.abs(np.diff(t, axis=1))[covered[:, 1:] & covered[:, :-1]].max())
    assert 0.05 < t[covered].min() and t[covered].max() < 0.95 and step < 0.05
    w = CM.turns_fraction(paint)
    dt = M.t_error(float(np.abs(corners).max()) * size + size, 1.0 / step) + (CM.angle_bound() + 2.0 * G.F32_ULP) / w
    delta = 0.02
    expect, sure = np.zeros((size * size, 4)), np.ones(size * size, dtype=bool)
    for ox, oy in offsets:
        truth = ground_truth(blob(), m, size, [(ox, oy), (ox + delta, oy + delta), (ox - delta, oy + delta), (ox + delta, oy - delta), (ox - delta, oy - delta)])
        sure &= (truth == truth[0]).all(axis=0)
        src, near = CM.conic_source(paint, colour[0], M.to_path_h(pix + np.array([ox, oy]), m, size), dt)
        sure &= ~(near & truth[0])
        expect += np.where(truth[0][:, None], src, 0.0) / len(offsets)
    got = image.reshape(-1, 4).astype(np.float64) / 255.0
    assert np.abs(got - expect)[sure].max() <= tol_of("over", False, M.max_slope(paint) * dt)
    assert sure.mean() > 0.9 and (expect[:, 3][sure] > 0).sum() > 400


def test_conic_painted_strokes_show_the_paint_where_the_stroke_covers(no_pins):
    """As the gradient tests' case 5: the same stroke drawn in opaque white at msaa 1 says which pixels it covers; the painted stroke must show
    the model's colour there and nothing elsewhere. The centre lies off the stroke."""
    from contrast_renderer_amd import Cap, CurveApproximation, DynamicStrokeOptions, Join, StrokeOptions
    size = SIZE
    path = Path(start=(-0.8, -0.5))
    for v in ((-0.2, 0.6), (0.3, -0.6), (0.8, 0.4)):
        path.push_line(v)
    path.stroke_options = StrokeOptions(0.3, 0.0, 4.0, False, 0, CurveApproximation.UniformlySpacedParameters(1))
    batch = batch_from_shapes([([DynamicStrokeOptions.Solid(Join.Round, Cap.Round, Cap.Round)], [path])])
    t = place(size, size, 64, 64, 56, rotate=0.2).reshape(1, 16)
    paint = Paint.conic((0.05, 0.75), 0.3, 0.3 + 0.5 * math.pi, [(0.0, (1.0, 0.9, 0.1, 1.0)), (0.4, (0.9, 0.1, 0.2, 1.0)), (1.0, (0.1, 0.2, 1.0, 1.0))], Spread.Reflect)
    white = np.float32([[1.0, 1.0, 1.0, 1.0]])
    solid, _ = draw(R.Configuration(), batch, t, white, [None])
    image, tap = draw(R.Configuration(), batch, t, white, [paint])
    assert tap["raster"] == "ops", tap
    covered = solid[..., 3] == 255
    assert 600 < covered.sum() and ((solid[..., 3] == 0) | covered).all()
    p = G.to_path(G.samples(size, size, 1).reshape(-1, 2), t[0], size, size)
    rho = np.hypot(*(p - np.float64(np.float32(paint.p0))).T) * G.min_pixel_scale(t[0], size, size)
    assert rho[covered.reshape(-1)].min() > 2 * CM.RHO_MIN
    src, near = CM.conic_source(paint, white[0], p, CM.t_error(paint, size + 80.0, rho), rho)
    expect = np.where(covered.reshape(-1, 1), src, 0.0).reshape(size, size, 4)
    ok = ~(near & covered.reshape(-1)).reshape(size, size)
    assert (~ok).sum() <= 0.10 * covered.sum()
    extra = M.max_slope(paint) * float(CM.t_error(paint, size + 80.0, rho[covered.reshape(-1)].min()))
    compare(image, expect, ok, tol_of("over", False, extra), "conic painted stroke")


# ---------------------------------------------------------------- 6. mixing and routing

def test_one_pass_mixes_every_kind_with_an_image_paint_and_a_solid_instance(no_pins):
    scene = CM.mixed_scene()
    kinds = [int(p.kind) if isinstance(p, Paint) else p for p in scene[4]]
    assert kinds[:3] == [int(PaintKind.Linear), int(PaintKind.Radial), int(PaintKind.Conic)] and kinds[4] is None
    against_model("mixed", scene, 4, False, background=random_background(SIZE, seed=5))


def test_a_conic_paint_the_pass_does_not_draw_changes_nothing_that_is_launched(no_pins):
    from contrast_renderer_amd import scenes
    sc = scenes.scene_mixed(24, (SIZE, SIZE), seed=3)
    transforms, colours = np.float32(sc["transforms"]).reshape(-1, 16), np.float32(sc["colors"]).reshape(-1, 4)
    n = len(colours)
    paint = CM.quadrant_paint()
    r = R.Renderer(R.Configuration(), device=0)
    scene = R.Scene(r, sc["batch"])
    frame = R.Frame(r, SIZE, SIZE)

    def plain():
        frame.clear()
        scene.render(frame, transforms, colours)
        tap = last_pass(frame)
        return frame.download(), (tap["formulation"], tap["general"], tap["raster"], tap["bin"])
    solid, before = plain()
    assert before[1] == 0 and before[2] != "ops"
    draws_first = [(i, i, op, 0, 0) for i in range(n // 2) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)]
    frame.clear()
    scene.render_draws(frame, transforms, colours, draws_first)
    recorded, tap_recorded = frame.download(), last_pass(frame)
    # a table whose conic paint is on an instance the pass does not draw: the recorded pass of the first half, the paint on the last instance
    scene.set_paints([paint], [-1] * (n - 1) + [0])
    frame.clear()
    scene.render_draws(frame, transforms, colours, draws_first)
    tap = last_pass(frame)
    assert np.array_equal(frame.download(), recorded)
    assert (tap["formulation"], tap["general"], tap["raster"]) == (tap_recorded["formulation"], tap_recorded["general"], tap_recorded["raster"])
    # ... and one that names only instances beyond the Scene's Shapes leaves the plain pass alone
    scene.set_paints([paint], [-1] * n + [0])
    image, after = plain()
    assert after == before and np.array_equal(image, solid)
    # drawn: the general kernel
    scene.set_paints([paint], [0] + [-1] * (n - 1))
    painted, tap = plain()
    assert tap[1] == 1 and tap[2] == "ops" and not np.array_equal(painted, solid)
    # a failed call leaves the earlier table in force
    from contrast_renderer_amd import ContrastError
    for bad in (Paint.conic((0, 0), 1.0, 1.0, [(0.0, (1, 0, 0, 1))]), Paint.conic((0, 0), 0.0, 7.0, [(0.0, (1, 0, 0, 1))]), Paint.conic((0, 0), 0.0, float("nan"), [(0.0, (1, 0, 0, 1))])):
        with pytest.raises(ContrastError):
            scene.set_paints([bad], [0])
    again, tap = plain()
    assert tap[2] == "ops" and np.array_equal(again, painted)
    scene.set_paints([], [])
    image, after = plain()
    assert after == before and np.array_equal(image, solid)


# ---------------------------------------------------------------- 7. a seeded sweep: all three kinds and spreads under sheared and mirrored transforms

def test_a_sweep_of_random_paints_and_transforms(no_pins):
    scene = CM.sweep_scene()
    paints = scene[4]
    assert len(paints) == 20 and sum(CM.is_conic(p) for p in paints) >= 5
    assert {int(p.kind) for p in paints if p is not None} == {1, 2, 4} and {int(p.spread) for p in paints if CM.is_conic(p)} == {0, 1, 2}
    against_model("sweep", scene, 4, False)
