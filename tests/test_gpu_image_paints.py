"""Image paints of the colour cover (include/contrast_hip.h, crh_scene_set_paints_with_images) on the GPU: k_raster_image against the float64
model of tests/image_paint_model.py, byte-equal to the solid colour for a white image and to the image for an identity blit, and launched only
for passes that draw an image-painted instance."""
import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, Path, batch_from_shapes
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Filter, Image, ImagePaint, Paint, Spread

import ground_truth_util as G
import image_paint_model as IM
import paint_model as M
from test_gpu_blending import STATES, compare, last_pass, no_pins, random_background, stack, tolerance  # noqa: F401
from test_ground_truth import place

pytestmark = pytest.mark.gpu

OVER = IM.OVER
SIZE = IM.SIZE
FILTERS = [Filter.Nearest, Filter.Linear]


def tol_of(name, attachment, extra):
    """tolerance() of the blending tests plus the image paint's own term: the largest channel difference between neighbouring texels of the
    wrapped image times the f32 error of (u, v) in texels (image_paint_model's docstring derives it). The scenes keep it below a quarter unit."""
    assert extra < 0.25 / 255.0, extra * 255
    return tolerance(name, attachment) + extra


def on_device(r, paints, images=None):
    """The model's paints (None, Paint, ImageSpec) -> what Scene.set_paints takes; one Image per distinct texel array."""
    images = {} if images is None else images
    out = []
    for p in paints:
        if isinstance(p, IM.ImageSpec):
            if id(p.pixels) not in images:
                images[id(p.pixels)] = Image(r, p.pixels)
            p = ImagePaint(images[id(p.pixels)], p.matrix, p.filter, p.spread_x, p.spread_y)
        out.append(p)
    return out


def draw(config, batch, transforms, colours, paints, fmt=R.FORMAT_RGBA8, background=None, size=SIZE, passes=2):
    r = R.Renderer(config, device=0)
    scene = R.Scene(r, batch)
    paints = on_device(r, paints)
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


# ---------------------------------------------------------------- 1. a white image is the instance's colour, byte for byte

@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("filter", FILTERS, ids=["nearest", "linear"])
@pytest.mark.parametrize("fmt", [R.FORMAT_RGBA8, R.FORMAT_RGBA8_ATTACHMENT], ids=["rgba8", "attachment"])
def test_a_white_image_equals_the_oracle_image_of_the_solid_scene(msaa, filter, fmt, no_pins):
    from oracle.binding import Oracle, render_pass
    shapes, transforms, colours, _ = stack(seed=7, size=SIZE, n=12, radius=(16, 36))
    batch = batch_from_shapes(shapes)
    white = np.full((8, 8, 4), 255, dtype=np.uint8)
    spreads = (Spread.Pad, Spread.Repeat, Spread.Reflect)
    rng = np.random.RandomState(3)
    paints = [IM.placed(white, 0.3, rng.uniform(0.0, 1.5), (rng.uniform(-4, 12), rng.uniform(-4, 12)), filter, spreads[i % 3], spreads[(i // 3) % 3]) for i in range(len(colours))]
    image, tap = draw(R.Configuration(msaa_sample_count=msaa), batch, transforms, colours, paints, fmt)
    assert tap["general"] == 1 and tap["raster"] == "ops", tap
    draws = [(i, i, op, 0, 0) for i in range(len(colours)) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)]
    expect, _ = render_pass(Oracle(batch), SIZE, SIZE, msaa, 4, 4, 0, transforms, colours, draws, attachment8=fmt == R.FORMAT_RGBA8_ATTACHMENT)
    assert np.array_equal(image, expect), f"{int((image != expect).any(axis=2).sum())} pixels differ"


# ---------------------------------------------------------------- 2. the identity blit gives the image's bytes back

def _blit(r, image, filter, size=SIZE):
    """One rectangle over the whole frame, path coordinates = pixel coordinates (x right, y down from the top left), m = the identity."""
    scene = R.Scene(r, batch_from_shapes([([], [Path.from_rect((size / 2.0, size / 2.0), (size / 2.0, size / 2.0))])]))
    t = np.zeros(16, dtype=np.float32)
    t[0], t[5], t[10], t[15], t[12], t[13] = 2.0 / size, -2.0 / size, 1.0, 1.0, -1.0, 1.0
    scene.set_paints([ImagePaint(image, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), filter)], [0])
    frame = R.Frame(r, size, size)
    frame.clear()
    scene.render(frame, t.reshape(1, 16), np.float32([[1.0, 1.0, 1.0, 1.0]]))
    return frame.download()


@pytest.mark.parametrize("filter", FILTERS, ids=["nearest", "linear"])
def test_an_identity_blit_returns_the_bytes_of_the_image(filter, no_pins):
    """LINEAR sits on texel centres: its fraction is the f32 error of (u, v), far below the 1 / 510 of a texel difference of 255 codes that
    would move a byte."""
    r = R.Renderer(R.Configuration(), device=0)
    pixels = random_background(SIZE, seed=17)  # premultiplied: rgb <= a
    assert np.array_equal(_blit(r, Image(r, pixels), filter), pixels)
    # ... and through a snapshot of a frame that holds a drawn scene; later passes into the frame do not change the snapshot
    shapes, transforms, colours, _ = stack(seed=7, size=SIZE, n=12, radius=(16, 36))
    scene = R.Scene(r, batch_from_shapes(shapes))
    source = R.Frame(r, SIZE, SIZE)
    source.clear()
    scene.render(source, transforms, colours)
    drawn = source.download()
    assert (drawn[..., 3] > 0).mean() > 0.3
    snapshot = Image.from_frame(source)
    assert (snapshot.width, snapshot.height) == (SIZE, SIZE)
    source.clear()
    scene.render(source, transforms[::-1].copy(), colours)
    assert np.array_equal(_blit(r, snapshot, filter), drawn)
    cleared = R.Frame(r, SIZE, SIZE)
    cleared.clear()
    assert not _blit(r, Image.from_frame(cleared), filter).any()
    for fmt in (R.FORMAT_BGRA8, R.FORMAT_RGBA16F):
        with pytest.raises(ContrastError):
            Image.from_frame(R.Frame(r, SIZE, SIZE, format=fmt))
    sliced = R.Frame(r, SIZE, SIZE)
    sliced.set_tile_rows(0, 64)
    with pytest.raises(ContrastError):
        Image.from_frame(sliced)
    for shape in ((0, 4, 4), (4, 0, 4), (16385, 1, 4)):
        with pytest.raises(ContrastError):
            Image(r, np.zeros(shape, dtype=np.uint8))


# ---------------------------------------------------------------- 3. the model: filters x spreads x msaa over a random background

def _against_model(name, scene, msaa, attachment, state_name="over", background=None):
    shapes, transforms, colours, regions, paints = scene
    background = random_background(SIZE) if background is None else background
    fmt = R.FORMAT_RGBA8_ATTACHMENT if attachment else R.FORMAT_RGBA8
    state = OVER if state_name == "over" else STATES[state_name]
    config = R.Configuration(msaa_sample_count=msaa) if state_name == "over" else R.Configuration(msaa_sample_count=msaa, blending=state)
    image, tap = draw(config, batch_from_shapes(shapes), transforms, colours, paints, fmt, background)
    assert tap["raster"] == "ops", tap
    expect, ok, extra, seams = IM.model(SIZE, msaa, transforms, colours, regions, paints, state, attachment, background)
    assert seams <= 0.02
    compare(image, expect, ok, tol_of(state_name, attachment, extra), f"{name} msaa {msaa}")


@pytest.mark.parametrize("msaa", [1, 2, 4, 8])
@pytest.mark.parametrize("spreads", IM.SPREADS, ids=[f"{a.name}-{b.name}" for a, b in IM.SPREADS])
@pytest.mark.parametrize("filter", FILTERS, ids=["nearest", "linear"])
def test_image_paints_match_the_float64_model(filter, spreads, msaa, no_pins):
    attachment = (int(filter) + int(spreads[0]) + msaa) % 2 == 1  # both frame formats over the grid
    _against_model(f"{filter.name} {spreads[0].name} {spreads[1].name}", IM.scene(filter, *spreads), msaa, attachment)


@pytest.mark.parametrize("filter", FILTERS, ids=["nearest", "linear"])
def test_an_image_of_one_texel(filter, no_pins):
    _against_model("one texel", IM.one_texel_scene(filter), 4, filter == Filter.Linear)


@pytest.mark.parametrize("msaa", [1, 4])
def test_a_minified_smooth_image(msaa, no_pins):
    _against_model("minified", IM.minified_scene(), msaa, False)


# ---------------------------------------------------------------- 4. perspective: the image follows the unprojected position

@pytest.mark.parametrize("msaa,filter", IM.CAMERA_CASES, ids=["1-nearest", "4-linear"])
def test_an_image_painted_blob_under_a_camera_matches_the_unprojected_position(msaa, filter, no_pins):
    from test_perspective_ground_truth import blob
    size = 96
    m, colour, spec, expect, sure, extra, _ = IM.camera_case(msaa, filter, size)
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, depth_compare=R.Compare.Less, depth_write_enabled=True), device=0)
    scene = R.Scene(r, batch_from_shapes([([], [blob()])]))
    scene.set_paints(on_device(r, [spec]), [0])
    frame = R.Frame(r, size, size)
    frame.clear()
    frame.clear_depth(1.0)
    scene.render(frame, m.reshape(1, 16), colour.reshape(1, 4))
    got = frame.download().reshape(-1, 4).astype(np.float64) / 255.0
    assert np.abs(got - expect)[sure].max() <= tol_of("over", False, extra)
    assert sure.mean() > 0.9 and (expect[:, 3][sure] > 0).sum() > 400


# ---------------------------------------------------------------- 5. a recorded pass: a gradient, an image paint and a solid cover, a clip, an opacity group

def test_a_recorded_pass_with_a_gradient_an_image_paint_and_a_solid_cover(no_pins):
    """Two Scene objects in one pass, as the gradient tests' recorded pass (tests/test_gpu_paints.py): the second cover is image painted."""
    size = SIZE
    S, CL, U, COL = R.RenderOperation.Stencil, R.RenderOperation.Clip, R.RenderOperation.UnClip, R.RenderOperation.Color
    SAVE, SCALE, REST = R.RenderOperation.SaveAlphaContext, R.RenderOperation.ScaleAlphaContext, R.RenderOperation.RestoreAlphaContext
    disc, rect = Path.from_circle((0.0, 0.0), 1.0), Path.from_rect((0.0, 0.0), (1.0, 1.0))
    r = R.Renderer(R.Configuration(msaa_sample_count=4, clip_nesting_counter_bits=2, alpha_layer_count=1), device=0)
    clipper, content = R.Scene(r, batch_from_shapes([([], [disc])])), R.Scene(r, batch_from_shapes([([], [disc]), ([], [rect])]))
    frame = R.Frame(r, size, size)
    frame.clear()
    (t_clip, t_all, (t_a, t_b, t_c), (c_a, c_b, c_c), group, paints), expect, ok, extra, _ = IM.recorded_case(size)
    gradient, textured, _ = on_device(r, paints)
    p = R.RenderPass(r, frame)
    i_clip, i_a, i_b = p.push_instance(t_clip, (0, 0, 0, 1)), p.push_instance(t_a, c_a, paint=gradient), p.push_instance(t_b, c_b, paint=textured)
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
    compare(image, expect, ok, tol_of("over", False, extra), "recorded pass")


# ---------------------------------------------------------------- 6. image painted strokes: the STROKES instantiations

@pytest.mark.parametrize("filter", FILTERS, ids=["nearest", "linear"])
@pytest.mark.parametrize("dashed", [False, True], ids=["solid", "dashed"])
def test_image_painted_strokes_show_the_image_where_the_stroke_covers(dashed, filter, no_pins):
    """As the gradient tests' strokes: the same stroke drawn in opaque white at msaa 1 says which pixels it covers."""
    from contrast_renderer_amd import Cap, CurveApproximation, DashInterval, DynamicStrokeOptions, Join, StrokeOptions
    size = SIZE
    path = Path(start=(-0.8, -0.5))
    for v in ((-0.2, 0.6), (0.3, -0.6), (0.8, 0.4)):
        path.push_line(v)
    path.stroke_options = StrokeOptions(0.3, 0.0, 4.0, False, 0, CurveApproximation.UniformlySpacedParameters(1))
    dynamic = DynamicStrokeOptions.Dashed(Join.Round, [DashInterval(0.0, 0.6, Cap.Round, Cap.Round), DashInterval(1.0, 1.5, Cap.Round, Cap.Round)], 0.1) if dashed \
        else DynamicStrokeOptions.Solid(Join.Round, Cap.Round, Cap.Round)
    batch = batch_from_shapes([([dynamic], [path])])
    t, spec, src, seam, extra = IM.stroke_case(filter, size)
    white = np.float32([[1.0, 1.0, 1.0, 1.0]])
    solid, _ = draw(R.Configuration(), batch, t.reshape(1, 16), white, [None])
    image, tap = draw(R.Configuration(), batch, t.reshape(1, 16), white, [spec])
    assert tap["raster"] == "ops", tap
    covered = solid[..., 3] == 255
    assert 600 < covered.sum() and ((solid[..., 3] == 0) | covered).all()
    expect = np.where(covered.reshape(-1, 1), src, 0.0).reshape(size, size, 4)
    ok = ~(seam.reshape(size, size) & covered)
    assert (~ok).sum() <= 0.02 * covered.sum()
    compare(image, expect, ok, tol_of("over", False, extra), "image painted stroke")


# ---------------------------------------------------------------- 7. an image paint under a blend state other than "over"

@pytest.mark.parametrize("name", ["additive", "mask-RA"])
def test_image_paints_blend_with_the_renderers_state(name, no_pins):
    _against_model(name, IM.scene(Filter.Linear, Spread.Reflect, Spread.Repeat, seed=6), 4, True, name, random_background(SIZE, seed=3))


# ---------------------------------------------------------------- 8. an sRGB target

def test_image_paints_on_a_bgra8_srgb_target(no_pins):
    """As test_gradients_on_a_bgra8_srgb_target: the code read back must be the one whose interval of linear values holds the model's value."""
    shapes, transforms, colours, regions, paints = IM.scene(Filter.Linear, Spread.Repeat, Spread.Reflect, seed=9)
    image, tap = draw(R.Configuration(msaa_sample_count=4), batch_from_shapes(shapes), transforms, colours, paints, R.FORMAT_BGRA8_SRGB)
    expect, ok, extra, _ = IM.model(SIZE, 4, transforms, colours, regions, paints, OVER, False, np.zeros((SIZE, SIZE, 4)))
    assert extra < 0.25 / 255.0
    tol = 512 * G.F32_ULP + extra
    got = image[..., [2, 1, 0, 3]].astype(np.float64)
    lo, hi = M.srgb_decode(np.maximum(got[..., :3] - 0.5, 0.0)) - tol, M.srgb_decode(np.minimum(got[..., :3] + 0.5, 255.0)) + tol
    bad = ok & (((expect[..., :3] < lo) | (expect[..., :3] > hi)).any(axis=2) | (np.abs(got[..., 3] / 255.0 - expect[..., 3]) > 0.5 / 255.0 + tol))
    assert not bad.any(), int(bad.sum())
    assert ok.mean() > 0.5 and (expect[..., 3][ok] > 0).mean() > 0.2


# ---------------------------------------------------------------- 9. routing: only a pass that draws an image-painted instance takes the image kernel

def test_only_a_pass_that_draws_an_image_painted_instance_changes_what_is_launched(no_pins):
    from contrast_renderer_amd import scenes
    sc = scenes.scene_mixed(24, (SIZE, SIZE), seed=3)
    transforms, colours = np.float32(sc["transforms"]).reshape(-1, 16), np.float32(sc["colors"]).reshape(-1, 4)
    n = len(colours)
    r = R.Renderer(R.Configuration(), device=0)
    scene = R.Scene(r, sc["batch"])
    frame = R.Frame(r, SIZE, SIZE)
    gradient = Paint.linear((-1, 0), (1, 0), [(0.0, (1, 0, 0, 1)), (1.0, (0, 0, 1, 1))])
    picture = Image(r, IM.random_image(np.random.RandomState(2), 8, 8))
    textured = ImagePaint(picture, (3.0, 1.0, 4.0, -1.0, 3.0, 4.0), Filter.Linear, Spread.Repeat, Spread.Reflect)

    def plain():
        frame.clear()
        scene.render(frame, transforms, colours)
        tap = last_pass(frame)
        return frame.download(), (tap["formulation"], tap["general"], tap["raster"], tap["bin"])
    draws_first = [(i, i, op, 0, 0) for i in range(n // 2) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)]

    def recorded():
        frame.clear()
        scene.render_draws(frame, transforms, colours, draws_first)
        tap = last_pass(frame)
        return frame.download(), (tap["formulation"], tap["general"], tap["raster"])
    # a Scene without a table
    solid, before = plain()
    solid_first, before_first = recorded()
    assert before[1] == 0 and before[2] != "ops"
    # a gradient-only table: what it drew and launched before any image table existed
    scene.set_paints([gradient], [0] + [-1] * (n - 1))
    graded, tap_graded = plain()
    assert tap_graded[2] == "ops" and not np.array_equal(graded, solid)
    # image paints on instances the pass does not draw
    scene.set_paints([textured], [-1] * (n - 1) + [0])
    image, tap = recorded()
    assert tap == before_first and np.array_equal(image, solid_first)
    scene.set_paints([gradient, textured], [-1] * n + [1, 0])
    image, after = plain()
    assert after == before and np.array_equal(image, solid)
    # drawn: the general kernel, another image
    scene.set_paints([textured, gradient], [0, 1] + [-1] * (n - 2))
    painted, tap = plain()
    assert tap[1] == 1 and tap[2] == "ops" and not np.array_equal(painted, solid) and not np.array_equal(painted, graded)
    # a failed call leaves the table in place
    other = R.Renderer(R.Configuration(), device=0)
    foreign = ImagePaint(Image(other, np.zeros((2, 2, 4), dtype=np.uint8)), textured.matrix)
    bad = [([textured], [1]), ([textured], [-2]), ([foreign], [0]), ([ImagePaint(picture, textured.matrix, filter=2)], [0]),
           ([ImagePaint(picture, textured.matrix, spread_y=3)], [0]), ([ImagePaint(picture, (float("nan"),) * 6)], [0]),
           ([textured, Paint.linear((0, 0), (0, 0), [(0.0, (1, 0, 0, 1))])], [0])]
    for bad_paints, bad_assoc in bad:
        with pytest.raises(ContrastError):
            scene.set_paints(bad_paints, bad_assoc)
    again, tap_again = plain()
    assert tap_again == tap and np.array_equal(again, painted)
    # Image.destroy() while the table names the image: the table keeps the pixels
    picture.destroy()
    with pytest.raises(ContrastError):
        scene.set_paints([textured], [0])  # (the mirror's paint now carries a null image; the table stays)
    again, tap_again = plain()
    assert tap_again == tap and np.array_equal(again, painted)
    # a gradient-only painted pass after the image table: the same image and kernel as before it
    scene.set_paints([gradient], [0] + [-1] * (n - 1))
    image, tap = plain()
    assert tap == tap_graded and np.array_equal(image, graded)
    # cleared: as before the first call
    scene.set_paints([], [])
    image, after = plain()
    assert after == before and np.array_equal(image, solid)


# ---------------------------------------------------------------- 10. the tile split: two slabs of rows equal the whole frame

def test_two_slabs_of_tile_rows_equal_the_whole_image_painted_frame(no_pins):
    shapes, transforms, colours, _, paints = IM.scene(Filter.Linear, Spread.Repeat, Spread.Reflect)
    r = R.Renderer(R.Configuration(msaa_sample_count=4), device=0)
    scene = R.Scene(r, batch_from_shapes(shapes))
    paints = on_device(r, paints)
    table = [p for p in paints if p is not None]
    scene.set_paints(table, [table.index(p) if p is not None else -1 for p in paints])

    def rows(begin, end):
        frame = R.Frame(r, SIZE, SIZE)
        if (begin, end) != (0, SIZE):
            frame.set_tile_rows(begin, end)
        frame.clear()
        scene.render(frame, transforms, colours)
        return frame.download()
    whole, upper, lower = rows(0, SIZE), rows(0, 64), rows(64, SIZE)
    assert (whole[..., 3] > 0).mean() > 0.3
    assert np.array_equal(upper[:64], whole[:64]) and np.array_equal(lower[64:], whole[64:]) and not upper[64:].any() and not lower[:64].any()


# ---------------------------------------------------------------- 11. the coordinate rule at its ends: NaN -> 0, the clamp to +-2^24, the wrap of what is left

def blit_rectangle(r, size):
    """The Scene and the transform of _blit without a table: path coordinates = pixel coordinates, the rectangle covers the frame."""
    scene = R.Scene(r, batch_from_shapes([([], [Path.from_rect((size / 2.0, size / 2.0), (size / 2.0, size / 2.0))])]))
    t = np.zeros(16, dtype=np.float32)
    t[0], t[5], t[10], t[15], t[12], t[13] = 2.0 / size, -2.0 / size, 1.0, 1.0, -1.0, 1.0
    return scene, t.reshape(1, 16), np.float32([[1.0, 1.0, 1.0, 1.0]])


def differing(got, expect):
    bad = (got != expect).any(axis=2)
    return f"{int(bad.sum())} of {bad.size} pixels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}" if bad.any() else None


@pytest.mark.parametrize("spreads", IM.EXTREME_SPREADS, ids=[f"{a.name}-{b.name}" for a, b in IM.EXTREME_SPREADS])
@pytest.mark.parametrize("filter", FILTERS, ids=["nearest", "linear"])
def test_coordinates_at_and_beyond_the_clamp_read_the_texel_the_rule_names(filter, spreads, no_pins):
    """image_paint_model.extreme_matrices: offsets next to 2^23, at 2^24 and beyond it, 3e38, products that overflow to inf, on either axis
    and on both. The expectation is the header's rule evaluated exactly (tests/test_image_paints_cpu.py holds it stable against an f32 error
    of the position), so the comparison is of bytes. Every index is formed by image_wrap from an int of magnitude <= 2^24 + 1."""
    size = IM.EXTREME_SIZE
    r = R.Renderer(R.Configuration(), device=0)
    pixels = IM.random_image(np.random.RandomState(5), *IM.EXTREME_IMAGE)
    image = Image(r, pixels)
    scene, t, white = blit_rectangle(r, size)
    frame = R.Frame(r, size, size)
    for name, matrix in IM.extreme_matrices():
        scene.set_paints([ImagePaint(image, matrix, filter, *spreads)], [0])
        frame.clear()
        scene.render(frame, t, white)
        what = differing(frame.download(), IM.extreme_expectation(pixels, matrix, filter, *spreads))
        assert what is None, f"{name} {matrix}: {what}"
        assert last_pass(frame)["raster"] == "ops"


@pytest.mark.parametrize("filter", [Filter.Nearest, Filter.LinearMipmap], ids=["nearest", "linear-mipmap"])
def test_a_white_image_under_a_camera_through_the_near_plane_equals_the_solid_blob(filter, no_pins):
    """The projective coordinates divide by a W that goes through 0 across the frame: whatever (u, v) comes of it — inf, NaN — is a texel of
    the all-255 image, so the cover is the solid colour's, byte for byte the oracle's."""
    from oracle.binding import Oracle, render_pass
    from test_perspective_ground_truth import CASES, blob, camera
    size = 96
    m = np.float32(camera(**CASES["through_the_near_plane"])).reshape(1, 16)
    colour = np.float32([[1.0, 0.9, 0.8, 0.9]])
    batch = batch_from_shapes([([], [blob()])])
    r = R.Renderer(R.Configuration(), device=0)
    white = Image(r, np.full((5, 8, 4), 255, dtype=np.uint8))
    white.generate_mipmaps()
    scene = R.Scene(r, batch)
    scene.set_paints([ImagePaint(white, (3.0, 1.0, 4.0, -1.0, 3.0, 4.0), filter, Spread.Repeat, Spread.Reflect)], [0])
    frame = R.Frame(r, size, size)
    frame.clear()
    scene.render(frame, m, colour)
    tap = last_pass(frame)
    assert tap["general"] == 1 and tap["raster"] == "ops", tap
    draws = [(0, 0, op, 0, 0) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)]
    expect, _ = render_pass(Oracle(batch), size, size, 1, 4, 4, 0, m, colour, draws)
    assert 400 < (expect[..., 3] > 0).sum() < size * size - 400
    what = differing(frame.download(), expect)
    assert what is None, what
