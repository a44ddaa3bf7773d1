"""Mipmapped image paints (include/contrast_hip.h, crh_image_generate_mipmaps and CRH_FILTER_MIPMAP) on the GPU: k_image_downsample bit for bit
against the integer chain of tests/mip_model.py, k_raster_mip against its float64 model, byte-equal to the base filter where f = 0 and to the
solid colour for a constant image, and launched only for passes that draw a flagged image paint of an image with levels."""
import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, Path, batch_from_shapes
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Filter, Image, ImagePaint, Paint, Spread

import ground_truth_util as G
import image_paint_model as IM
import mip_model as MM
import paint_model as M
from test_gpu_blending import STATES, compare, last_pass, no_pins, random_background, stack, tolerance  # noqa: F401
from test_gpu_image_paints import tol_of
from test_ground_truth import place

pytestmark = pytest.mark.gpu

OVER = IM.OVER
SIZE = MM.SIZE
MIP_FILTERS = [Filter.NearestMipmap, Filter.LinearMipmap]


def on_device(r, paints, images=None):
    """The model's paints (None, Paint, ImageSpec, MipSpec) -> what Scene.set_paints takes; one Image per distinct texel array, with its mipmaps
    when a MipSpec holds a chain."""
    images = {} if images is None else images
    out = []
    for p in paints:
        if isinstance(p, (IM.ImageSpec, MM.MipSpec)):
            if id(p.pixels) not in images:
                images[id(p.pixels)] = Image(r, p.pixels)
            if isinstance(p, MM.MipSpec) and len(p.levels) > 1:
                images[id(p.pixels)].generate_mipmaps()
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


# ---------------------------------------------------------------- 1. the chain, bit for bit

def _check_chain(image, pixels):
    expect = MM.chain(pixels)
    assert image.levels == 1 and np.array_equal(image.download_level(0), pixels)
    with pytest.raises(ContrastError):
        image.download_level(1)
    image.generate_mipmaps()
    assert image.levels == len(expect) == MM.level_count(pixels.shape[1], pixels.shape[0])
    got = [image.download_level(l) for l in range(image.levels)]
    for l, (a, b) in enumerate(zip(got, expect)):
        assert a.shape == b.shape and np.array_equal(a, b), (l, a.shape, b.shape)
    image.generate_mipmaps()  # a second call changes nothing
    assert image.levels == len(expect) and all(np.array_equal(image.download_level(l), a) for l, a in enumerate(got))
    for level in (image.levels, image.levels + 7):
        with pytest.raises(ContrastError):
            image.download_level(level)


@pytest.mark.parametrize("width,height", [(1, 1), (1, 7), (7, 1), (5, 3), (8, 8), (33, 17), (64, 64), (16384, 1)])
def test_the_chain_equals_the_integer_model(width, height, no_pins):
    r = R.Renderer(R.Configuration(), device=0)
    pixels = IM.random_image(np.random.RandomState(width + 3 * height), width, height)
    _check_chain(Image(r, pixels), pixels)


def test_the_chain_of_a_frame_snapshot(no_pins):
    r = R.Renderer(R.Configuration(), device=0)
    shapes, transforms, colours, _ = stack(seed=7, size=SIZE, n=12, radius=(16, 36))
    scene = R.Scene(r, batch_from_shapes(shapes))
    source = R.Frame(r, SIZE, SIZE)
    source.clear()
    scene.render(source, transforms, colours)
    drawn = source.download()
    assert (drawn[..., 3] > 0).mean() > 0.3
    _check_chain(Image.from_frame(source), drawn)


# ---------------------------------------------------------------- 2. f = 0 is the base filter, byte for byte

@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("filter", MIP_FILTERS, ids=["nearest", "linear"])
@pytest.mark.parametrize("levels", ["one-level", "magnified"])
def test_a_mipmap_paint_with_f_zero_gives_the_bytes_of_its_base_filter(levels, filter, msaa, no_pins):
    """A one-level image has nothing to blend; a magnified placement (a texel is at least a pixel on both axes: rho <= 1) has lod 0."""
    shapes, transforms, colours, regions, plain = IM.scene(Filter(int(filter) & 1), Spread.Repeat, Spread.Reflect)
    specs = [p for p, t in zip(plain, transforms) if isinstance(p, IM.ImageSpec)]
    assert all(IM.texel_px(p, t, SIZE) >= 4.0 for p, t in zip(plain, transforms) if isinstance(p, IM.ImageSpec)) and len(specs) >= 4
    chains = {}
    flagged = []
    for p in plain:
        if isinstance(p, IM.ImageSpec):
            chain = chains.setdefault(id(p.pixels), MM.chain(p.pixels) if levels == "magnified" else [p.pixels])
            p = MM.MipSpec(p.pixels, p.matrix, int(filter), p.spread_x, p.spread_y, chain)
        flagged.append(p)
    background = random_background(SIZE)
    base, tap_base = draw(R.Configuration(msaa_sample_count=msaa), batch_from_shapes(shapes), transforms, colours, plain, background=background)
    image, tap = draw(R.Configuration(msaa_sample_count=msaa), batch_from_shapes(shapes), transforms, colours, flagged, background=background)
    assert tap["raster"] == tap_base["raster"] == "ops"
    assert np.array_equal(image, base), f"{int((image != base).any(axis=2).sum())} pixels differ"
    assert (image != background).any(axis=2).mean() > 0.3


# ---------------------------------------------------------------- 3. equal levels: a constant image is the instance's colour

@pytest.mark.parametrize("spreads", IM.SPREADS, ids=[f"{a.name}-{b.name}" for a, b in IM.SPREADS])
@pytest.mark.parametrize("filter", MIP_FILTERS, ids=["nearest", "linear"])
def test_a_constant_image_minified_equals_the_oracle_image_of_the_solid_scene(filter, spreads, no_pins):
    from oracle.binding import Oracle, render_pass
    shapes, transforms, colours, _ = stack(seed=7, size=SIZE, n=12, radius=(16, 36))
    batch = batch_from_shapes(shapes)
    white = np.full((17, 33, 4), 255, dtype=np.uint8)
    chain = MM.chain(white)
    assert len(chain) == 6 and all((l == 255).all() for l in chain)
    rng = np.random.RandomState(3)
    paints = [MM.placed_minified(white, t, SIZE, 5.0, rng.uniform(0.3, 1.2), (rng.uniform(-4, 40), rng.uniform(-4, 20)), filter, spreads[0], spreads[1], chain) for t in transforms]
    image, tap = draw(R.Configuration(msaa_sample_count=4), batch, transforms, colours, paints)
    assert tap["general"] == 1 and tap["raster"] == "ops", tap
    draws = [(i, i, op, 0, 0) for i in range(len(colours)) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)]
    expect, _ = render_pass(Oracle(batch), SIZE, SIZE, 4, 4, 4, 0, transforms, colours, draws, attachment8=False)
    assert np.array_equal(image, expect), f"{int((image != expect).any(axis=2).sum())} pixels differ"


# ---------------------------------------------------------------- 4. the model: minifications x spreads x msaa over a random background

def _against_model(name, scene, msaa, attachment, state_name="over", background=None):
    shapes, transforms, colours, regions, paints = scene
    background = random_background(SIZE) if background is None else background
    fmt = R.FORMAT_RGBA8_ATTACHMENT if attachment else R.FORMAT_RGBA8
    state = OVER if state_name == "over" else STATES[state_name]
    config = R.Configuration(msaa_sample_count=msaa) if state_name == "over" else R.Configuration(msaa_sample_count=msaa, blending=state)
    image, tap = draw(config, batch_from_shapes(shapes), transforms, colours, paints, fmt, background)
    assert tap["raster"] == "ops", tap
    expect, ok, extra, seams = MM.model(SIZE, msaa, transforms, colours, regions, paints, state, attachment, background)
    assert seams <= 0.02
    compare(image, expect, ok, tol_of(state_name, attachment, extra), f"{name} msaa {msaa}")


@pytest.mark.parametrize("msaa", [1, 2, 4, 8])
@pytest.mark.parametrize("spreads", IM.SPREADS, ids=[f"{a.name}-{b.name}" for a, b in IM.SPREADS])
def test_trilinear_paints_match_the_float64_model(spreads, msaa, no_pins):
    attachment = (int(spreads[0]) + msaa) % 2 == 1  # both frame formats over the grid
    _against_model(f"LinearMipmap {spreads[0].name} {spreads[1].name}", MM.scene(Filter.LinearMipmap, *spreads), msaa, attachment)


@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("spreads", IM.SPREADS, ids=[f"{a.name}-{b.name}" for a, b in IM.SPREADS])
def test_nearest_mipmap_paints_match_the_float64_model(spreads, msaa, no_pins):
    attachment = (int(spreads[0]) + msaa) % 2 == 0
    _against_model(f"NearestMipmap {spreads[0].name} {spreads[1].name}", MM.scene(Filter.NearestMipmap, *spreads), msaa, attachment)


# ---------------------------------------------------------------- 5. the point of the feature: a minified checkerboard is grey, not moire

def test_a_minified_checkerboard_is_flat_with_mipmaps_and_aliases_without(no_pins):
    shapes, t, colour, region, spec = MM.checkerboard_case()
    batch = batch_from_shapes(shapes)
    pix = G.samples(SIZE, SIZE, 1).reshape(-1, 2)
    inside = (region(G.to_path(pix, t, SIZE, SIZE)) * G.min_pixel_scale(t, SIZE, SIZE) > 1.0).reshape(SIZE, SIZE)  # fully covered pixels
    assert inside.sum() > 3000
    smooth, tap = draw(R.Configuration(), batch, t.reshape(1, 16), colour.reshape(1, 4), [spec])
    assert tap["raster"] == "ops"
    tint = np.float64(colour)
    flat = np.array([tint[0] * tint[3], tint[1] * tint[3], tint[2] * tint[3], 0.0]) * (128.0 / 255.0) + np.array([0.0, 0.0, 0.0, tint[3]])
    _, _, extra, _ = MM.model(SIZE, 1, [t], [colour], [region], [spec], OVER, False, np.zeros((SIZE, SIZE, 4)))
    worst = np.abs(smooth[inside].astype(np.float64) / 255.0 - flat).max()
    assert worst <= tol_of("over", False, extra), worst * 255.0
    plain = IM.ImageSpec(spec.pixels, spec.matrix, Filter.Linear, spec.spread_x, spec.spread_y)
    aliased, _ = draw(R.Configuration(), batch, t.reshape(1, 16), colour.reshape(1, 4), [plain])
    green = aliased[inside][:, 1].astype(int)
    assert green.max() - green.min() > 64, (green.min(), green.max())


# ---------------------------------------------------------------- 6. perspective: lod per sample

@pytest.mark.parametrize("msaa", [1, 4])
def test_a_mipmapped_blob_under_a_camera_matches_the_per_sample_model(msaa, no_pins):
    from test_perspective_ground_truth import blob
    size = 96
    m, colour, spec, expect, sure, extra, _, lod_range = MM.camera_case(msaa, size=size)
    assert lod_range > 1.5
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, depth_compare=R.Compare.Less, depth_write_enabled=True), device=0)
    scene = R.Scene(r, batch_from_shapes([([], [blob()])]))
    scene.set_paints(on_device(r, [spec]), [0])
    frame = R.Frame(r, size, size)
    frame.clear()
    frame.clear_depth(1.0)
    scene.render(frame, m.reshape(1, 16), colour.reshape(1, 4))
    got = frame.download().reshape(-1, 4).astype(np.float64) / 255.0
    worst = np.abs(got - expect)[sure].max()
    assert worst <= tol_of("over", False, extra), worst * 255.0
    assert sure.mean() > 0.9 and (expect[:, 3][sure] > 0).sum() > 400


# ---------------------------------------------------------------- 7. STROKES, XFMT, a blend state, the tile split

def test_a_mipmapped_dashed_stroke_shows_the_image_where_the_stroke_covers(no_pins):
    """As the image paint tests' strokes: the same stroke drawn in opaque white at msaa 1 says which pixels it covers."""
    from contrast_renderer_amd import Cap, CurveApproximation, DashInterval, DynamicStrokeOptions, Join, StrokeOptions
    path = Path(start=(-0.8, -0.5))
    for v in ((-0.2, 0.6), (0.3, -0.6), (0.8, 0.4)):
        path.push_line(v)
    path.stroke_options = StrokeOptions(0.3, 0.0, 4.0, False, 0, CurveApproximation.UniformlySpacedParameters(1))
    dynamic = DynamicStrokeOptions.Dashed(Join.Round, [DashInterval(0.0, 0.6, Cap.Round, Cap.Round), DashInterval(1.0, 1.5, Cap.Round, Cap.Round)], 0.1)
    batch = batch_from_shapes([([dynamic], [path])])
    t, spec, src, extra = MM.stroke_case()
    white = np.float32([[1.0, 1.0, 1.0, 1.0]])
    solid, _ = draw(R.Configuration(), batch, t.reshape(1, 16), white, [None])
    image, tap = draw(R.Configuration(), batch, t.reshape(1, 16), white, [spec])
    assert tap["raster"] == "ops", tap
    covered = solid[..., 3] == 255
    assert 600 < covered.sum() and ((solid[..., 3] == 0) | covered).all()
    expect = np.where(covered.reshape(-1, 1), src, 0.0).reshape(SIZE, SIZE, 4)
    compare(image, expect, np.ones((SIZE, SIZE), dtype=bool), tol_of("over", False, extra), "mipmapped stroke")


def test_trilinear_paints_on_a_bgra8_srgb_target(no_pins):
    """As test_image_paints_on_a_bgra8_srgb_target: the code read back must be the one whose interval of linear values holds the model's value."""
    shapes, transforms, colours, regions, paints = MM.scene(Filter.LinearMipmap, Spread.Repeat, Spread.Reflect, seed=9)
    image, tap = draw(R.Configuration(msaa_sample_count=4), batch_from_shapes(shapes), transforms, colours, paints, R.FORMAT_BGRA8_SRGB)
    expect, ok, extra, _ = MM.model(SIZE, 4, transforms, colours, regions, paints, OVER, False, np.zeros((SIZE, SIZE, 4)))
    assert extra < 0.25 / 255.0
    tol = 512 * G.F32_ULP + extra
    got = image[..., [2, 1, 0, 3]].astype(np.float64)
    lo, hi = M.srgb_decode(np.maximum(got[..., :3] - 0.5, 0.0)) - tol, M.srgb_decode(np.minimum(got[..., :3] + 0.5, 255.0)) + tol
    bad = ok & (((expect[..., :3] < lo) | (expect[..., :3] > hi)).any(axis=2) | (np.abs(got[..., 3] / 255.0 - expect[..., 3]) > 0.5 / 255.0 + tol))
    assert not bad.any(), int(bad.sum())
    assert ok.mean() > 0.5 and (expect[..., 3][ok] > 0).mean() > 0.2


def test_trilinear_paints_blend_with_the_additive_state(no_pins):
    _against_model("additive", MM.scene(Filter.LinearMipmap, Spread.Reflect, Spread.Repeat, seed=6), 4, True, "additive", random_background(SIZE, seed=3))


def test_two_slabs_of_tile_rows_equal_the_whole_mipmapped_frame(no_pins):
    shapes, transforms, colours, _, paints = MM.scene(Filter.LinearMipmap, Spread.Repeat, Spread.Reflect)
    r = R.Renderer(R.Configuration(msaa_sample_count=4), device=0)
    scene = R.Scene(r, batch_from_shapes(shapes))
    paints = on_device(r, paints)
    scene.set_paints(paints, list(range(len(paints))))

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


# ---------------------------------------------------------------- 8. routing: only a pass that draws a flagged paint changes what is drawn

def test_only_a_pass_that_draws_a_flagged_image_paint_changes_what_is_launched(no_pins):
    from contrast_renderer_amd import scenes
    sc = scenes.scene_mixed(24, (SIZE, SIZE), seed=3)
    transforms, colours = np.float32(sc["transforms"]).reshape(-1, 16), np.float32(sc["colors"]).reshape(-1, 4)
    n = len(colours)
    r = R.Renderer(R.Configuration(), device=0)
    scene = R.Scene(r, sc["batch"])
    frame = R.Frame(r, SIZE, SIZE)
    gradient = Paint.linear((-1, 0), (1, 0), [(0.0, (1, 0, 0, 1)), (1.0, (0, 0, 1, 1))])
    pixels = MM.checkerboard(64)
    picture, late = Image(r, pixels), Image(r, pixels)
    picture.generate_mipmaps()
    matrix = (300.0, 100.0, 4.0, -100.0, 300.0, 4.0)  # hundreds of texels per path unit: minified wherever the scene draws it
    unflagged = ImagePaint(picture, matrix, Filter.Linear, Spread.Repeat, Spread.Reflect)
    flagged = ImagePaint(picture, matrix, Filter.LinearMipmap, Spread.Repeat, Spread.Reflect)

    def plain():
        frame.clear()
        scene.render(frame, transforms, colours)
        tap = last_pass(frame)
        return frame.download(), (tap["formulation"], tap["general"], tap["raster"], tap["bin"])
    half = [(i, i, op, 0, 0) for i in range(n // 2) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)]

    def recorded():
        frame.clear()
        scene.render_draws(frame, transforms, colours, half)
        tap = last_pass(frame)
        return frame.download(), (tap["formulation"], tap["general"], tap["raster"])
    # before any flagged paint existed: solid, gradient-only, an unflagged image paint
    solid, tap_solid = plain()
    solid_half, tap_solid_half = recorded()
    scene.set_paints([gradient], [0] + [-1] * (n - 1))
    graded, tap_graded = plain()
    scene.set_paints([unflagged], [0] + [-1] * (n - 1))
    textured, tap_textured = plain()
    textured_half, tap_textured_half = recorded()
    assert not np.array_equal(textured, solid) and not np.array_equal(textured, graded)
    # one flagged and one unflagged paint in the table, the flagged one on an instance the pass does not draw
    scene.set_paints([unflagged, flagged], [0] + [-1] * (n - 2) + [1])
    image, tap = recorded()
    assert tap == tap_textured_half and np.array_equal(image, textured_half)
    scene.set_paints([unflagged, flagged], [-1] * n + [0, 1])  # both beyond the Scene's instances: a solid pass
    image, tap = plain()
    assert tap == tap_solid and np.array_equal(image, solid)
    image, tap = recorded()
    assert tap == tap_solid_half and np.array_equal(image, solid_half)
    scene.set_paints([gradient, flagged], [0] + [-1] * (n - 1) + [1])
    image, tap = plain()
    assert tap == tap_graded and np.array_equal(image, graded)
    # drawn: another image, and the unflagged item beside it keeps its bytes' worth — the whole frame differs only where instance 0 covers
    scene.set_paints([unflagged, flagged], [1, 0] + [-1] * (n - 2))
    mipped, tap_mipped = plain()
    assert tap_mipped[1] == 1 and tap_mipped[2] == "ops" and not np.array_equal(mipped, textured)
    scene.set_paints([unflagged], [0, 0] + [-1] * (n - 2))
    both_plain, _ = plain()
    assert not np.array_equal(mipped, both_plain)
    # a failed call leaves the table in place
    scene.set_paints([unflagged, flagged], [1, 0] + [-1] * (n - 2))
    for bad_paints, bad_assoc in (([flagged], [1]), ([ImagePaint(picture, matrix, filter=0x102)], [0]), ([ImagePaint(picture, matrix, filter=5)], [0]),
                                  ([ImagePaint(picture, matrix, filter=0x200)], [0])):
        with pytest.raises(ContrastError):
            scene.set_paints(bad_paints, bad_assoc)
    again, tap_again = plain()
    assert tap_again == tap_mipped and np.array_equal(again, mipped)
    # Image.destroy() under the live table: the table keeps the pixels and their levels
    picture.destroy()
    again, tap_again = plain()
    assert tap_again == tap_mipped and np.array_equal(again, mipped)
    # a table built before generate_mipmaps keeps drawing its one-level image: the flag on one level is the base filter
    scene.set_paints([ImagePaint(late, matrix, Filter.Linear, Spread.Repeat, Spread.Reflect)], [0] + [-1] * (n - 1))
    one_level, _ = plain()
    assert np.array_equal(one_level, textured)
    scene.set_paints([ImagePaint(late, matrix, Filter.LinearMipmap, Spread.Repeat, Spread.Reflect)], [0] + [-1] * (n - 1))
    image, _ = plain()
    assert np.array_equal(image, one_level)
    late.generate_mipmaps()
    assert late.levels == 7
    image, _ = plain()
    assert np.array_equal(image, one_level)
    scene.set_paints([ImagePaint(late, matrix, Filter.LinearMipmap, Spread.Repeat, Spread.Reflect)], [0] + [-1] * (n - 1))
    image, _ = plain()
    assert not np.array_equal(image, one_level)
    # cleared: as before the first call
    scene.set_paints([], [])
    image, tap = plain()
    assert tap == tap_solid and np.array_equal(image, solid)


# ---------------------------------------------------------------- 10. lod at its ends: rho huge or +inf, rho = 0

@pytest.mark.parametrize("spreads", IM.EXTREME_SPREADS, ids=[f"{a.name}-{b.name}" for a, b in IM.EXTREME_SPREADS])
@pytest.mark.parametrize("filter", MIP_FILTERS, ids=["nearest", "linear"])
def test_lod_at_its_ends_reads_the_last_level_or_the_base_filter(filter, spreads, no_pins):
    """m0 = m4 = 1e30 or 3e38: rho^2 overflows to +inf in f32, lod = L - 1 and f = 0, every pixel holds the bytes of the 1 x 1 level whatever
    the clamped (u, v) wrap to. m0 = m1 = m3 = m4 = 0: rho = 0, lod = 0, every pixel is texel (wrap(floor(m2)), wrap(floor(m5))) of level 0.
    The extreme matrices of the plain filters have rho = 1 or beyond on an axis that is constant: those with lod = 0 must give the plain
    filter's bytes. A Jacobian column that is NaN: the placement turned by 45 degrees with dX/dsx = dY/dsx = 2, so that m0 = 3e38, m1 = -3e38
    give du/dsx = inf - inf (the library is built without contraction: both products are rounded) while du/dsy = -inf; the NaN column wins,
    lod = 0. There X >= 272 on the whole frame, u = fma(Y, m1, +inf) = +inf is clamped to 2^24, v = 1.5: one texel of level 0."""
    from test_gpu_image_paints import blit_rectangle, differing
    size = IM.EXTREME_SIZE
    r = R.Renderer(R.Configuration(), device=0)
    pixels = IM.random_image(np.random.RandomState(5), *IM.EXTREME_IMAGE)
    chain = MM.chain(pixels)
    assert len(chain) == 4 and chain[-1].shape == (1, 1, 4)
    image = Image(r, pixels)
    image.generate_mipmaps()
    scene, t, white = blit_rectangle(r, size)
    frame = R.Frame(r, size, size)

    def drawn(matrix):
        scene.set_paints([ImagePaint(image, matrix, filter, *spreads)], [0])
        frame.clear()
        scene.render(frame, t, white)
        assert last_pass(frame)["raster"] == "ops"
        return frame.download()
    for big in (1e30, 3e38):
        what = differing(drawn((big, 0.0, 0.0, 0.0, big, 0.0)), np.broadcast_to(chain[-1], (size, size, 4)))
        assert what is None, f"m0 = m4 = {big}: {what}"
    for m2, m5 in ((3.5, 1.5), (-1027.5, 16777216.0), (3e38, -3e38)):
        matrix = (0.0, 0.0, m2, 0.0, 0.0, m5)
        expect = IM.extreme_expectation(pixels, matrix, Filter(int(filter) & 1), *spreads)
        assert len(np.unique(expect.reshape(-1, 4), axis=0)) == 1
        what = differing(drawn(matrix), expect)
        assert what is None, f"rho = 0 at {m2}, {m5}: {what}"
    for name, matrix in IM.extreme_matrices():  # lod = 0 where both columns of J have a norm of at most 1: the plain filter's bytes
        columns = (np.hypot(matrix[0], matrix[3]), np.hypot(matrix[1], matrix[4]))
        if max(columns) <= 1.0:
            what = differing(drawn(matrix), IM.extreme_expectation(pixels, matrix, Filter(int(filter) & 1), *spreads))
            assert what is None, f"{name}: {what}"
    turned = R.Scene(r, batch_from_shapes([([], [Path.from_rect((400.0, 128.0), (200.0, 200.0))])]))
    k, ox, oy = 0.25, -100.0, 100.0  # pixel = (k (X + Y) + ox, k (Y - X) + oy): X = 2 (sx - sy + 200), Y = 2 (sx + sy), exact
    t2 = np.zeros(16, dtype=np.float32)
    t2[0], t2[4], t2[12], t2[1], t2[5], t2[13], t2[10], t2[15] = 2 * k / size, 2 * k / size, 2 * ox / size - 1.0, 2 * k / size, -2 * k / size, 1.0 - 2 * oy / size, 1.0, 1.0
    turned.set_paints([ImagePaint(image, (3e38, -3e38, 0.0, 0.0, 0.0, 1.5), filter, *spreads)], [0])
    frame.clear()
    turned.render(frame, t2.reshape(1, 16), white)
    texel = pixels[int(IM.wrap(np.int64(1), 5, spreads[1])), int(IM.wrap(np.int64(2 ** 24), 8, spreads[0]))]
    assert not np.array_equal(texel, chain[-1][0, 0])
    what = differing(frame.download(), np.broadcast_to(texel, (size, size, 4)))
    assert what is None, f"a NaN column of J: {what}"
