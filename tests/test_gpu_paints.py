"""Gradient paints of the colour cover (include/contrast_hip.h, crh_scene_set_paints) on the GPU: k_raster_paint against the float64 model of
tests/paint_model.py, byte-equal to the solid colour where every stop carries it, and launched only for passes that draw a painted instance."""
import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, Path, batch_from_shapes
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import BlendState, ColorTargetState, ColorWrites, GradientStop, Paint, PaintKind, Spread

import ground_truth_util as G
import paint_model as M
from test_gpu_blending import STATES, compare, last_pass, no_pins, random_background, stack, tolerance  # noqa: F401
from test_ground_truth import place

pytestmark = pytest.mark.gpu

OVER = ColorTargetState(BlendState.PREMULTIPLIED_ALPHA_BLENDING)
SIZE = 128


def tol_of(name, attachment, extra):
    """tolerance() of the blending tests — half a unit for the resolve, or one unit per attachment write carried with weight <= 1, plus 512 ulp
    for the blend arithmetic (the stop interpolation's three roundings and the tint's and premultiply's two are of that order) — plus what the
    f32 error of t moves the source by: the largest colour slope per unit t of the scene's paints times paint_model.t_error (derived there from
    the roundings of the documented evaluation, scaled by frame extent / gradient length). The scenes keep that term below a quarter unit."""
    assert extra < 0.25 / 255.0, extra * 255
    return tolerance(name, attachment) + extra


def draw(config, batch, transforms, colours, paints, fmt=R.FORMAT_RGBA8, background=None, size=SIZE, passes=2):
    r = R.Renderer(config, device=0)
    scene = R.Scene(r, batch)
    table = [p for p in paints if p is not None]
    scene.set_paints(table, [table.index(p) if p is not None else -1 for p in paints])
    frame = R.Frame(r, size, size, format=fmt)
    images = []
    for _ in range(passes):  # the verified pass, then one with the buffers sized
        if background is not None:
            frame.upload(background)
        else:
            frame.clear()
        scene.render(frame, transforms, colours)
        images.append(frame.download())
    assert all(np.array_equal(images[0], im) for im in images[1:])
    return images[0], last_pass(frame)


# ---------------------------------------------------------------- 1. a paint whose stops all carry the instance's colour is that colour, byte for byte

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
        base = M.random_paint(rng, (PaintKind.Linear, PaintKind.Radial)[i % 2], (Spread.Pad, Spread.Repeat, Spread.Reflect)[i % 3], n_stops=2)
        paints.append(Paint(base.kind, base.spread, base.p0, base.p1, tuple(stops)))
    white = np.ones_like(colours)
    image, tap = draw(R.Configuration(msaa_sample_count=msaa), batch, transforms, white, paints, fmt)
    assert tap["general"] == 1 and tap["raster"] == "ops", tap
    draws = [(i, i, op, 0, 0) for i in range(len(colours)) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)]
    expect, _ = render_pass(Oracle(batch), SIZE, SIZE, msaa, 4, 4, 0, transforms, colours, draws, attachment8=fmt == R.FORMAT_RGBA8_ATTACHMENT)
    assert np.array_equal(image, expect), f"{int((image != expect).any(axis=2).sum())} pixels differ"


# ---------------------------------------------------------------- 2. the model: kinds x spreads x msaa over a random background

@pytest.mark.parametrize("msaa", [1, 2, 4, 8])
@pytest.mark.parametrize("kind,spread", M.SCENES, ids=[f"{k.name}-{s.name}" for k, s in M.SCENES])
def test_gradients_match_the_float64_model(kind, spread, msaa, no_pins):
    shapes, transforms, colours, regions, paints = M.scene(kind, spread)
    background = random_background(SIZE)
    attachment = (int(kind) + int(spread) + msaa) % 2 == 1  # both frame formats over the grid
    fmt = R.FORMAT_RGBA8_ATTACHMENT if attachment else R.FORMAT_RGBA8
    image, tap = draw(R.Configuration(msaa_sample_count=msaa), batch_from_shapes(shapes), transforms, colours, paints, fmt, background)
    assert tap["raster"] == "ops", tap
    expect, ok, extra = M.model(SIZE, msaa, transforms, colours, regions, paints, OVER, attachment, background)
    compare(image, expect, ok, tol_of("over", attachment, extra), f"{kind.name} {spread.name} msaa {msaa}")


def test_gradients_on_a_bgra8_srgb_target(no_pins):
    """The frame keeps linear f32 colours within the pass and encodes the resolved value: the code read back must be the one whose interval of
    linear values holds the model's value, within the tolerance; alpha is linear."""
    shapes, transforms, colours, regions, paints = M.scene(PaintKind.Linear, Spread.Reflect, seed=9)
    image, tap = draw(R.Configuration(msaa_sample_count=4), batch_from_shapes(shapes), transforms, colours, paints, R.FORMAT_BGRA8_SRGB)
    expect, ok, extra = M.model(SIZE, 4, transforms, colours, regions, paints, OVER, False, np.zeros((SIZE, SIZE, 4)))
    tol = 512 * G.F32_ULP + extra
    got = image[..., [2, 1, 0, 3]].astype(np.float64)
    lo, hi = M.srgb_decode(np.maximum(got[..., :3] - 0.5, 0.0)) - tol, M.srgb_decode(np.minimum(got[..., :3] + 0.5, 255.0)) + tol
    bad = ok & (((expect[..., :3] < lo) | (expect[..., :3] > hi)).any(axis=2) | (np.abs(got[..., 3] / 255.0 - expect[..., 3]) > 0.5 / 255.0 + tol))
    assert not bad.any(), int(bad.sum())
    assert ok.mean() > 0.5 and (expect[..., 3][ok] > 0).mean() > 0.2


# ---------------------------------------------------------------- 3. perspective: the paint follows the unprojected position

@pytest.mark.parametrize("msaa", [1, 4])
def test_a_painted_blob_under_a_camera_matches_the_unprojected_position(msaa, no_pins):
    from test_perspective_ground_truth import CASES, blob, camera, ground_truth
    size = 96
    m = np.float32(camera(**CASES["tilted"])).reshape(16)
    paint = Paint.linear((-0.8, -0.6), (0.7, 0.6), [(0.0, (1.0, 0.2, 0.1, 1.0)), (0.5, (0.1, 0.9, 0.3, 0.8)), (1.0, (0.2, 0.3, 1.0, 1.0))], Spread.Pad)
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
    delta = 0.02
    expect, sure = np.zeros((size * size, 4)), np.ones(size * size, dtype=bool)
    pix = G.pixel_centres(size)
    # the projective evaluation divides by W: one rounding more (paint_model.t_error counts it); the plane is foreshortened, so a unit of t
    # is as short on the frame as the smallest singular value of the homography's Jacobian over the blob — bounded below from the corners
    corners = M.to_path_h(np.array([[0.0, 0.0], [size, 0.0], [0.0, size], [size, size]], dtype=np.float64), m, size)
    for ox, oy in offsets:
        truth = ground_truth(blob(), m, size, [(ox, oy), (ox + delta, oy + delta), (ox - delta, oy + delta), (ox + delta, oy - delta), (ox - delta, oy - delta)])
        sure &= (truth == truth[0]).all(axis=0)
        p = M.to_path_h(pix + np.array([ox, oy]), m, size)
        src, _ = M.paint_source(paint, colour[0], p, 0.0)
        expect += np.where(truth[0][:, None], src, 0.0) / len(offsets)
    # pixels per unit of t, from the model itself: the smallest step of t between neighbouring pixels bounds the local gradient length
    t = M.raw_t(paint, M.to_path_h(pix, m, size)).reshape(size, size)
    covered = (expect[:, 3] > 0).reshape(size, size)
    step = max(np.abs(np.diff(t, axis=0))[covered[1:] & covered[:-1]].max(), np.abs(np.diff(t, axis=1))[covered[:, 1:] & covered[:, :-1]].max())
    extra = M.max_slope(paint) * M.t_error(float(np.abs(corners).max()) * size + size, 1.0 / step)
    got = image.reshape(-1, 4).astype(np.float64) / 255.0
    assert np.abs(got - expect)[sure].max() <= tol_of("over", False, extra)
    assert sure.mean() > 0.9 and (expect[:, 3][sure] > 0).sum() > 400


# ---------------------------------------------------------------- 4. a recorded pass: painted and solid instances, a clip, an opacity group

def test_a_recorded_pass_with_clip_and_opacity_group(no_pins):
    """Two Scene objects in one pass (the frame keeps its pass state): a disc clips two painted covers and a solid one, all inside an opacity
    group. The alpha-context covers are the existing ones: over a cleared frame (saved alpha 0) Scale then Restore leave alpha * a inside the
    clip, ((1 - a) + alpha a) - (1 - 0)(1 - a), and the colours as they are."""
    size = SIZE
    S, CL, U, COL = R.RenderOperation.Stencil, R.RenderOperation.Clip, R.RenderOperation.UnClip, R.RenderOperation.Color
    SAVE, SCALE, REST = R.RenderOperation.SaveAlphaContext, R.RenderOperation.ScaleAlphaContext, R.RenderOperation.RestoreAlphaContext
    disc, rect = Path.from_circle((0.0, 0.0), 1.0), Path.from_rect((0.0, 0.0), (1.0, 1.0))
    r = R.Renderer(R.Configuration(msaa_sample_count=4, clip_nesting_counter_bits=2, alpha_layer_count=1), device=0)
    clipper, content = R.Scene(r, batch_from_shapes([([], [disc])])), R.Scene(r, batch_from_shapes([([], [disc]), ([], [rect])]))
    frame = R.Frame(r, size, size)
    frame.clear()
    t_clip, t_all, (t_a, t_b, t_c), (c_a, c_b, c_c), group, regions, paints, clip_sd = M.recorded_scene(size)
    grad_a, grad_b = paints[0], paints[1]
    p = R.RenderPass(r, frame)
    i_clip, i_a, i_b = p.push_instance(t_clip, (0, 0, 0, 1)), p.push_instance(t_a, c_a, paint=grad_a), p.push_instance(t_b, c_b, paint=grad_b)
    i_c, i_g = p.push_instance(t_c, c_c), p.push_instance(t_all, group)
    p.render(clipper, [i_clip], S)
    p.set_clip_depth(1)
    p.render(clipper, [i_clip], CL)
    p.set_alpha_layer(0)
    p.render(content, [i_g], SAVE, 1)
    for inst, shape in ((i_a, 0), (i_b, 1), (i_c, 0)):
        p.render(content, [inst], S, shape)
        p.render(content, [inst], COL, shape)
    p.render(content, [i_g], SCALE, 1)
    p.render(content, [i_g], REST, 1)
    p.set_clip_depth(0)
    p.render(clipper, [i_clip], U)
    p.submit()
    image = frame.download()
    assert last_pass(frame)["raster"] == "ops"
    transforms, colours = [t_a, t_b, t_c], [c_a, c_b, c_c]
    expect, ok, extra = M.model(size, 4, transforms, colours, regions, paints, OVER, False, np.zeros((size, size, 4)))
    alpha = _per_sample_alpha(size, transforms, colours, regions, paints)
    expect[..., 3] = np.where((clip_sd > 0).reshape(-1, 4), alpha * group[3], alpha).mean(axis=1).reshape(size, size)
    compare(image, expect, ok, tol_of("over", False, extra), "recorded pass")


def _per_sample_alpha(size, transforms, colours, regions, paints):
    pix = G.samples(size, size, 4).reshape(-1, 2)
    dst = np.zeros((len(pix), 4))
    for t, c, region, paint in zip(transforms, colours, regions, paints):
        q = G.to_path(pix, t, size, size)
        if paint is None:
            tint = np.float64(np.float32(c))
            src = np.tile([tint[0] * tint[3], tint[1] * tint[3], tint[2] * tint[3], tint[3]], (len(pix), 1))
        else:
            src, _ = M.paint_source(paint, c, q, 0.0)
        dst = M.blend_src(dst, region(q) > 0, src, OVER, False)
    return dst[:, 3].reshape(-1, 4)


# ---------------------------------------------------------------- 5. painted strokes: the STROKES instantiation

@pytest.mark.parametrize("dashed", [False, True], ids=["solid", "dashed"])
def test_painted_strokes_show_the_paint_where_the_stroke_covers(dashed, no_pins):
    """The stroke stages are the solid pass's own and are held against ground truth elsewhere (tests/test_ground_truth.py); here the same stroke
    drawn in opaque white at msaa 1 says which pixels it covers, and the painted stroke must show the model's colour there and nothing elsewhere."""
    from contrast_renderer_amd import Cap, CurveApproximation, DashInterval, DynamicStrokeOptions, Join, StrokeOptions
    size = SIZE
    path = Path(start=(-0.8, -0.5))
    for v in ((-0.2, 0.6), (0.3, -0.6), (0.8, 0.4)):
        path.push_line(v)
    path.stroke_options = StrokeOptions(0.3, 0.0, 4.0, False, 0, CurveApproximation.UniformlySpacedParameters(1))
    dynamic = DynamicStrokeOptions.Dashed(Join.Round, [DashInterval(0.0, 0.6, Cap.Round, Cap.Round), DashInterval(1.0, 1.5, Cap.Round, Cap.Round)], 0.1) if dashed \
        else DynamicStrokeOptions.Solid(Join.Round, Cap.Round, Cap.Round)
    batch = batch_from_shapes([([dynamic], [path])])
    t = place(size, size, 64, 64, 56, rotate=0.2).reshape(1, 16)
    paint = Paint.radial((0.1, -0.1), 1.0, [(0.0, (1.0, 0.9, 0.1, 1.0)), (0.4, (0.9, 0.1, 0.2, 1.0)), (1.0, (0.1, 0.2, 1.0, 1.0))], Spread.Reflect)
    white = np.float32([[1.0, 1.0, 1.0, 1.0]])
    solid, _ = draw(R.Configuration(), batch, t, white, [None])
    image, tap = draw(R.Configuration(), batch, t, white, [paint])
    assert tap["raster"] == "ops", tap
    covered = solid[..., 3] == 255
    assert 600 < covered.sum() and ((solid[..., 3] == 0) | covered).all()
    src, _ = M.paint_source(paint, white[0], G.to_path(G.samples(size, size, 1).reshape(-1, 2), t[0], size, size), 0.0)
    expect = np.where(covered.reshape(-1, 1), src, 0.0).reshape(size, size, 4)
    extra = M.max_slope(paint) * M.t_error(size + 80.0, M.length_px(paint, t[0], size))
    compare(image, expect, np.ones((size, size), dtype=bool), tol_of("over", False, extra), "painted stroke")


# ---------------------------------------------------------------- 6. a paint under a blend state other than "over"

@pytest.mark.parametrize("name", ["additive", "mask-RA"])
def test_paints_blend_with_the_renderers_state(name, no_pins):
    shapes, transforms, colours, regions, paints = M.scene(PaintKind.Radial, Spread.Reflect, seed=6)
    background = random_background(SIZE, seed=3)
    config = R.Configuration(msaa_sample_count=4, blending=STATES[name])
    image, tap = draw(config, batch_from_shapes(shapes), transforms, colours, paints, R.FORMAT_RGBA8_ATTACHMENT, background)
    assert tap["raster"] == "ops", tap
    expect, ok, extra = M.model(SIZE, 4, transforms, colours, regions, paints, STATES[name], True, background)
    compare(image, expect, ok, tol_of(name, True, extra), name)


# ---------------------------------------------------------------- 7. routing: only a pass that draws a painted instance changes kernels

def test_only_a_pass_that_draws_a_painted_instance_takes_the_paint_kernel(no_pins):
    from contrast_renderer_amd import scenes
    sc = scenes.scene_mixed(24, (SIZE, SIZE), seed=3)
    transforms, colours = np.float32(sc["transforms"]).reshape(-1, 16), np.float32(sc["colors"]).reshape(-1, 4)
    n = len(colours)
    paint = Paint.linear((-1, 0), (1, 0), [(0.0, (1, 0, 0, 1)), (1.0, (0, 0, 1, 1))])
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
    # a table whose painted instance is not drawn in the pass: the recorded pass of the first half, the paint on the last instance
    scene.set_paints([paint], [-1] * (n - 1) + [0])
    frame.clear()
    scene.render_draws(frame, transforms, colours, draws_first)
    tap = last_pass(frame)
    assert np.array_equal(frame.download(), recorded) and (tap["formulation"], tap["general"], tap["raster"]) == (tap_recorded["formulation"], tap_recorded["general"], tap_recorded["raster"])
    # ... and a table that names only instances beyond the Scene's Shapes leaves the plain pass alone
    scene.set_paints([paint], [-1] * n + [0])
    image, after = plain()
    assert after == before and np.array_equal(image, solid)
    # drawn: the general kernel
    scene.set_paints([paint], [0] + [-1] * (n - 1))
    painted, tap = plain()
    assert tap[1] == 1 and tap[2] == "ops" and not np.array_equal(painted, solid)
    # a failed call leaves the earlier table in force
    for bad_paints, bad_assoc in (([paint], [1]), ([Paint.linear((0, 0), (0, 0), [(0.0, (1, 0, 0, 1))])], [0]), ([paint], [-2])):
        with pytest.raises(ContrastError):
            scene.set_paints(bad_paints, bad_assoc)
    again, tap = plain()
    assert tap[2] == "ops" and np.array_equal(again, painted)
    # cleared: as before the first call
    scene.set_paints([], [])
    image, after = plain()
    assert after == before and np.array_equal(image, solid)


# ---------------------------------------------------------------- 8. a seeded sweep: random paints under random affine transforms

def test_a_sweep_of_random_paints_and_transforms(no_pins):
    size = SIZE
    shapes, transforms, colours, regions, paints = M.sweep_scene(size)
    for t, q in zip(transforms, paints):
        assert q is None or M.length_px(q, t, size) >= 16.0
    image, tap = draw(R.Configuration(msaa_sample_count=4), batch_from_shapes(shapes), transforms, colours, paints)
    assert tap["raster"] == "ops", tap
    expect, ok, extra = M.model(size, 4, transforms, colours, regions, paints, OVER, False, np.zeros((size, size, 4)))
    compare(image, expect, ok, tol_of("over", False, extra), "sweep")


# ---------------------------------------------------------------- 9. a pass's paints do not outlive the pass

def test_a_pass_without_paints_after_a_painted_pass_is_the_solid_pass(no_pins):
    """RenderPass hands its paints to the Scenes it draws. The next pass numbers its instances from 0 again: one without paints must show the
    solid image and run what it ran before any paint was set — as must a plain Scene.render — while a table the caller set stays in force."""
    size = SIZE
    S, COL = R.RenderOperation.Stencil, R.RenderOperation.Color
    shapes, transforms, colours, _, paints = M.scene(PaintKind.Linear, Spread.Pad, n=6)
    r = R.Renderer(R.Configuration(msaa_sample_count=4), device=0)
    scene = R.Scene(r, batch_from_shapes(shapes))
    frame = R.Frame(r, size, size)

    def run(with_paints):
        frame.clear()
        p = R.RenderPass(r, frame)
        for i in range(len(colours)):
            k = p.push_instance(transforms[i], colours[i], paint=paints[i] if with_paints else None)
            p.render(scene, [k], S, i)
            p.render(scene, [k], COL, i)
        p.submit()
        tap = last_pass(frame)
        # (not the binning route: the edge pass bins a frame's later passes in the batches its first verified pass measured, paints or none)
        return frame.download(), (tap["formulation"], tap["general"], tap["raster"])
    solid, before = run(False)
    assert before[1] == 0 and before[2] != "ops"
    painted, tap = run(True)
    assert tap[2] == "ops" and not np.array_equal(painted, solid)
    again, tap = run(True)  # the same table: not installed a second time, the same image
    assert np.array_equal(again, painted) and scene._pass_paints is not None
    image, after = run(False)
    assert after == before and np.array_equal(image, solid) and scene._pass_paints is None
    run(True)
    frame.clear()
    scene.render(frame, transforms, colours)  # the plain pass after a painted RenderPass: solid too
    plain_after, tap_after = frame.download(), last_pass(frame)
    scene2 = R.Scene(r, batch_from_shapes(shapes))
    frame.clear()
    scene2.render(frame, transforms, colours)
    assert np.array_equal(plain_after, frame.download()) and tap_after["general"] == 0 and tap_after["raster"] != "ops"
    # the caller's own table is not a pass's: a pass without paints leaves it in force
    scene.set_paints([paints[0]], [0])
    kept, tap = run(False)
    assert tap[2] == "ops" and not np.array_equal(kept, solid)
