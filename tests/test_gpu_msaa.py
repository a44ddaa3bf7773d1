"""msaa_sample_count 2 and 8 (renderer.rs:393-394, :490-494): the triangle pass at S = 2 and S = 8, checked against float64 geometry and by
exact internal cross-checks. The oracle draws msaa 1 and 4 only, so the ground truth here is the standard sample pattern of
include/contrast_hip.h, read back per sample through the depth attachment, and the float64 models of test_ground_truth.py at the new counts."""
import copy
import os

import numpy as np
import pytest

from contrast_renderer_amd import Path, batch_from_shapes

import ground_truth_util as G
import test_ground_truth as T

pytestmark = pytest.mark.gpu

# the standard patterns of 2 and 8 samples (Vulkan standardSampleLocations = D3D), in 1/16 pixel, x right, y down, sample-index order
PATTERNS = {1: [(8, 8)], 2: [(12, 12), (4, 4)], 4: [(6, 2), (14, 6), (2, 10), (10, 14)],
            8: [(9, 5), (7, 11), (13, 9), (5, 3), (3, 13), (1, 7), (11, 15), (15, 1)]}
for _n in (2, 8):  # additive: the module's 1x / 4x entries stay as they are
    G.SAMPLE_OFFSETS.setdefault(_n, np.array(PATTERNS[_n], dtype=np.float64) / 16.0)

NEW = (2, 8)


def _R():
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import renderer as R
    return R


@pytest.fixture
def no_pins(monkeypatch):
    """A pin of the whole suite's run (CRH_TRIANGLE_PASS, CRH_EDGE_PASS, ...) is cancelled where a test sets its own."""
    from test_gpu_fuzz import _no_path_pins
    _no_path_pins(monkeypatch)
    return monkeypatch


def unit_rect():
    return ([], [Path.from_rect((0.0, 0.0), (1.0, 1.0))])


def box_transform(x0, x1, y0, y1, width, height, z=0.0):
    """The instance that maps the unit rect's [-1, 1]^2 onto the pixel box [x0, x1] x [y0, y1] (y down) at depth z (exact in f32 for dyadic
    boxes in a power-of-two frame)."""
    m = np.zeros(16, dtype=np.float64)
    m[0], m[5], m[10], m[15] = (x1 - x0) / width, (y1 - y0) / height, 1.0, 1.0
    m[12], m[13], m[14] = (x0 + x1) / width - 1.0, 1.0 - (y0 + y1) / height, z
    return m.astype(np.float32)


# ---------------------------------------------------------------- 1. configuration

@pytest.mark.parametrize("msaa", NEW)
def test_renderer_accepts_2_and_8(msaa):
    R = _R()
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, depth_write_enabled=True), device=0)
    assert r.get_config().msaa_sample_count == msaa
    frame = R.Frame(r, 40, 24)
    frame.clear_depth(0.5)
    depth = frame.download_depth()
    assert depth.shape == (24, 40, msaa) and (depth == 0.5).all()


@pytest.mark.parametrize("msaa", [0, 3, 5, 6, 7, 16, 32])
def test_other_counts_stay_unsupported(msaa):
    R = _R()
    from contrast_renderer_amd._ffi import ERR_UNSUPPORTED, ContrastError
    with pytest.raises(ContrastError) as e:
        R.Renderer(R.Configuration(msaa_sample_count=msaa), device=0)
    assert e.value.status == ERR_UNSUPPORTED


# ---------------------------------------------------------------- 2. per-sample positions and order

def painted_depth(boxes, width, height, msaa):
    """Float64: the depth every sample holds after the boxes (x0, x1, y0, y1, z) were drawn in order with Always + depth write, 1.0 where
    none covers it. No box edge lies on a sample (odd multiples of 1/32 px), so membership is exact."""
    pos = G.samples(width, height, msaa)  # [pixels, msaa, 2]
    out = np.ones((height * width, msaa))
    for x0, x1, y0, y1, z in boxes:
        inside = (pos[..., 0] > x0) & (pos[..., 0] < x1) & (pos[..., 1] > y0) & (pos[..., 1] < y1)
        out = np.where(inside, z, out)
    return out.reshape(height, width, msaa)


def probe_boxes(msaa, size, seed):
    """Random boxes plus, for every sample offset of the pattern, a sliver one sixteenth of a pixel wide around that offset's column (row)
    in the first and the last pixel column (row) of a tile: it covers that sample column (row) only, and the tile walk must keep it."""
    rng = np.random.RandomState(seed)
    odd = lambda lo, hi: (2 * rng.randint(lo * 16, hi * 16) + 1) / 32.0
    boxes = []
    for _ in range(24):  # corners at odd multiples of 1/32 px, sides multiples of 1/16 px
        x0, y0 = odd(0, size - 9), odd(0, size - 9)
        boxes.append((x0, x0 + rng.randint(1, 128) / 16.0, y0, y0 + rng.randint(1, 128) / 16.0))
    tiles = size // 16
    for k, (ox, oy) in enumerate(PATTERNS[msaa]):
        for first in (True, False):
            t = (k * 2 + first) % tiles
            col = t * 16 + (0 if first else 15)
            c = col + ox / 16.0
            boxes.append((c - 1 / 32, c + 1 / 32, t * 16 + 2 + 1 / 32, t * 16 + 13 + 1 / 32))  # one sample column, rows of one tile
            r = col + oy / 16.0
            boxes.append((((t + 1) % tiles) * 16 + 2 + 1 / 32, ((t + 1) % tiles) * 16 + 13 + 1 / 32, r - 1 / 32, r + 1 / 32))
    return [(x0, x1, y0, y1, (i + 1) / 256.0) for i, (x0, x1, y0, y1) in enumerate(boxes)]


@pytest.mark.parametrize("msaa", [1, 2, 4, 8])
@pytest.mark.parametrize("seed", [0, 1])
def test_samples_sit_where_the_table_says(msaa, seed, no_pins):
    R = _R()
    size = 64
    boxes = probe_boxes(msaa, size, seed)
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, depth_write_enabled=True), device=0)
    scene = R.Scene(r, batch_from_shapes([unit_rect() for _ in boxes]))
    assert scene.status() == 0
    t = np.stack([box_transform(x0, x1, y0, y1, size, size, z) for x0, x1, y0, y1, z in boxes])
    c = np.tile(np.float32([1, 1, 1, 1]), (len(boxes), 1))
    frame = R.Frame(r, size, size)
    frame.clear()
    frame.clear_depth(1.0)
    scene.render(frame, t, c)
    got = frame.download_depth()
    expect = painted_depth(boxes, size, size, msaa)
    bad = got != expect
    assert not bad.any(), f"msaa {msaa}: {int(bad.sum())} samples differ, first (y, x, k) {np.argwhere(bad)[:5].tolist()}"
    # every sample index is covered by some box and missed by some other
    for k in range(msaa):
        assert (got[..., k] < 1.0).any() and (got[..., k] == 1.0).any()


# ---------------------------------------------------------------- 3. float64 coverage (the cases of test_ground_truth.py at 2x and 8x)

def _at(case, msaa):
    out = copy.copy(case)
    out.msaa = msaa
    out.name = f"{case.name}-msaa{msaa}"
    return out


def _colour_case(msaa):
    base = next(c for c in T.CASES if c.name == "colour-over-rgba8-msaa4")
    out = _at(base, msaa)
    inner = base.model
    # the model's own tolerance covers 28 blends and a 4-sample average; 8 samples add four roundings of values <= 1
    out.model = lambda case: inner(case)[:2] + (0.5 / 255.0 + 40 * G.F32_ULP,)
    return out


GT_CASES = [_at(c, m) for m in NEW for c in T.CASES if c.kind == "coverage" and c.width * c.height <= 1 << 20] + [_colour_case(m) for m in NEW]


def render_case(case, R, general):
    r = R.Renderer(R.Configuration(msaa_sample_count=case.msaa, clip_nesting_counter_bits=0, winding_counter_bits=case.winding_bits), device=0)
    scene = R.Scene(r, case.batch)
    assert scene.status() == 0
    frame = R.Frame(r, case.width, case.height, format=case.fmt)
    images, passes = [], []
    from test_gpu_fuzz import last_pass
    for _ in range(2):  # the verified pass, then the pass with the lists in place
        frame.clear()
        if general:
            frame.keep_pass_state()
        scene.render(frame, case.transforms, case.colors)
        images.append(frame.download())
        passes.append(last_pass(frame))
    return images, passes


@pytest.mark.parametrize("general", [False, True], ids=["tile", "ops"])
@pytest.mark.parametrize("case", GT_CASES, ids=[c.name for c in GT_CASES])
def test_gpu_matches_the_model(case, general):
    R = _R()
    images, passes = render_case(case, R, general)
    for t in passes:  # msaa 2 / 8: the triangle pass under every pin of the suite's run
        assert t["formulation"] == 2 and t["raster"] == ("ops" if general else "tile"), t
    for image in images:
        T.check(case, image)


# ---------------------------------------------------------------- 4. RenderOperations at 8x against float64 regions

def rect(cx, cy, hx, hy):
    return ([], [Path.from_rect((cx, cy), (hx, hy))])


def _polygon_region(path):
    v = G.flatten(path, samples=1, closed=False)  # the vertices (line segments only)
    return lambda p: G.convex_polygon(p, v)


def ops_scenes():
    """Clip ... UnClip with a nested clip, and an opacity group (alpha contexts): test_render_ops.py's scenes under an instance that is
    rotated a little, so that edges cross the sample columns of the pattern."""
    from test_render_ops import alpha_scene, clip_scene
    out = {}
    for name, make, shapes in (("clip", clip_scene, lambda: [([], [Path.from_regular_polygon((0.0, 0.0), 0.6, 0.0, 24)]), rect(-0.3, 0.0, 0.5, 0.2),
                                                                 rect(0.3, 0.3, 0.5, 0.2), rect(0.0, 0.0, 0.25, 0.9), rect(0.0, -0.6, 0.9, 0.1)]),
                               ("alpha", alpha_scene, lambda: [rect(0.0, 0.0, 0.9, 0.9), rect(0.0, 0.0, 0.6, 0.6), rect(-0.2, 0.1, 0.3, 0.5), rect(0.3, -0.2, 0.4, 0.2)])):
        batch, t, c, draws = make()
        t = t.copy().reshape(-1, 4, 4)
        t[:, 0, 1] = 0.07
        t[:, 1, 0] = -0.05
        out[name] = (batch, t.reshape(-1, 16), c, draws, [_polygon_region(paths[0]) for _, paths in shapes()])
    return out


def ops_model(regions, t, colors, draws, size, msaa, layers=2):
    """Float64 per-sample statement of the stencil / blend states (renderer.rs:565-582, 692-754, 761-861; shaders.wgsl:304-331) over convex
    regions: every Shape here is one convex polygon, so its winding is +-1 inside and 0 outside, and its cover hull is the polygon.
    -> (resolved [size, size, 4], checkable [size, size])."""
    from contrast_renderer_amd.renderer import RenderOperation as Op
    pix = G.samples(size, size, msaa).reshape(-1, 2)
    n = len(pix)
    clip = np.zeros(n, dtype=np.int64)
    wind = np.zeros(n, dtype=np.int64)
    col = np.zeros((n, 4))
    saved = np.zeros((layers, n))
    near = np.zeros(n, dtype=bool)
    eps = T.f32_eps(size, size, size)
    for shape, inst, op, ref, layer in draws:
        sd = regions[shape](G.to_path(pix, t[inst], size, size)) * G.min_pixel_scale(t[inst], size, size)
        near |= np.abs(sd) <= eps
        inside = sd > 0
        c = np.float64(colors[inst])
        if op == Op.Stencil:  # LessEqual(ref <= stencil)
            wind = np.where(inside & (clip >= ref), wind + 1, wind)
        elif op == Op.Color:  # Less(ref < stencil) -> blend; Zero
            go = inside & ((clip > ref) | ((clip == ref) & (wind != 0)))
            src = np.array([c[0] * c[3], c[1] * c[3], c[2] * c[3], c[3]])
            col = np.where(go[:, None], src + col * (1.0 - c[3]), col)
            wind = np.where(inside, 0, wind)
        elif op == Op.Clip:  # NotEqual(winding) -> Replace(ref)
            go = inside & (wind != 0)
            clip, wind = np.where(go, ref, clip), np.where(go, 0, wind)
        elif op == Op.UnClip:  # Less(ref < clip) -> Replace(ref)
            go = inside & (ref < clip)
            clip, wind = np.where(go, ref, clip), np.where(go, 0, wind)
        else:  # the alpha-context covers: LessEqual(ref <= stencil), stencil untouched
            go = inside & (clip >= ref)
            if op == Op.SaveAlphaContext:
                saved[layer] = np.where(go, col[:, 3], saved[layer])
            elif op == Op.ScaleAlphaContext:
                s = 1.0 - c[3]
                col[:, 3] = np.where(go, s + col[:, 3] * (1.0 - s), col[:, 3])
            else:
                col[:, 3] = np.where(go, col[:, 3] - (1.0 - saved[layer]) * (1.0 - c[3]), col[:, 3])
    resolved = col.reshape(size * size, msaa, 4).mean(axis=1).reshape(size, size, 4)
    ok = ~near.reshape(-1, msaa).any(axis=1).reshape(size, size)
    return resolved, ok


@pytest.mark.parametrize("case", ["clip", "alpha"])
@pytest.mark.parametrize("msaa", NEW)
def test_render_operations_match_the_model(case, msaa):
    R = _R()
    batch, t, c, draws, regions = ops_scenes()[case]
    size = 192
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, clip_nesting_counter_bits=4, winding_counter_bits=4, alpha_layer_count=2), device=0)
    scene = R.Scene(r, batch)
    assert scene.status() == 0
    frame = R.Frame(r, size, size)
    frame.clear()
    scene.render_draws(frame, t, c, draws)
    got = frame.download().astype(np.float64) / 255.0
    expect, ok = ops_model(regions, t, c, draws, size, msaa)
    diff = np.abs(got - np.clip(expect, 0.0, 1.0)).max(axis=2)
    tol = 0.5 / 255.0 + 64 * G.F32_ULP
    assert ok.mean() > 0.9 and (expect[..., 3][ok] > 0).sum() > 5000
    bad = ok & (diff > tol)
    assert not bad.any(), f"{case} msaa {msaa}: {int(bad.sum())} pixels off (worst {diff[ok].max():.4f})"


def _separate_shapes(r, shapes):
    from contrast_renderer_amd import renderer as R
    return [R.Shape.from_paths(r, opts, paths) for opts, paths in shapes]


@pytest.mark.parametrize("case", ["clip", "alpha"])
def test_pass_state_spans_scene_objects_at_8x(case):
    """A recorded pass cut over one Scene object per Shape (carried pass state) gives the bytes of the same draws in one Scene."""
    R = _R()
    from test_render_ops import _shapes_of, _submit_per_shape
    batch, t, c, draws, _ = ops_scenes()[case]
    r = R.Renderer(R.Configuration(msaa_sample_count=8, clip_nesting_counter_bits=4, winding_counter_bits=4, alpha_layer_count=2), device=0)
    scene = R.Scene(r, batch)
    frame = R.Frame(r, 192, 192)
    frame.clear()
    scene.render_draws(frame, t, c, draws)
    whole = frame.download()
    objects = _separate_shapes(r, _shapes_of(case))
    for _ in range(2):
        frame.clear()
        _submit_per_shape(r, frame, objects, t, c, draws)
        assert np.array_equal(frame.download(), whole)
    assert (whole[..., 3] > 0).mean() > 0.02


def _perspective(cx, cy, scale, z, tilt, mirror=False):
    """clip = (sx * x + cx, scale * y + cy, z, 1 + tilt * x) for path points (x, y), sx = -+scale: a projective instance (clip.w varies)."""
    m = np.zeros((4, 4))  # [column][row] of the column-major mat4
    m[0, 0], m[1, 1], m[0, 3] = -scale if mirror else scale, scale, tilt
    m[3, 0], m[3, 1], m[3, 2], m[3, 3] = cx, cy, z, 1.0
    return m.reshape(-1).astype(np.float32)


def perspective_depth_model(transforms, drawn, size, msaa):
    """Float64: per sample, the LessEqual + write result of the unit squares `drawn` (in draw order) under their projective instances — the
    depth z / w of the surface through the sample, 1.0 where none — and the samples within 1e-3 px of a projected edge."""
    pix = G.samples(size, size, msaa).reshape(-1, 2)
    nx, ny = pix[:, 0] / size * 2.0 - 1.0, 1.0 - pix[:, 1] / size * 2.0
    depth = np.ones(len(pix))
    near = np.zeros(len(pix), dtype=bool)
    for k in drawn:
        m = transforms[k].astype(np.float64).reshape(4, 4)
        corners = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], dtype=np.float64)
        cl = corners[:, 0:1] * m[0] + corners[:, 1:2] * m[1] + m[3]
        quad = np.stack([(cl[:, 0] / cl[:, 3] * 0.5 + 0.5) * size, (0.5 - cl[:, 1] / cl[:, 3] * 0.5) * size], axis=1)
        sd = G.convex_polygon(pix, quad)
        near |= np.abs(sd) < 1e-3
        x = (m[3, 0] - nx) / (nx * m[0, 3] - m[0, 0])  # nx * (1 + tilt x) = sx * x + cx
        zw = m[3, 2] / (1.0 + m[0, 3] * x)
        depth = np.where((sd > 0) & (zw <= depth), zw, depth)
    return depth.reshape(-1, msaa), near.reshape(-1, msaa).any(axis=1)


def test_perspective_depth_and_culling_at_8x():
    """Projective instances with a depth test and back-face culling: two tilted squares that interpenetrate in depth, and a mirrored
    instance (clockwise on screen) in front of both, which is culled. Per sample the nearer surface wins (LessEqual + write); checked per
    sample through the depth attachment, away from the projected edges."""
    R = _R()
    size = 128
    t = np.stack([_perspective(0.1, 0.05, 0.6, 0.5, 0.3), _perspective(-0.1, -0.05, 0.45, 0.45, -0.35), _perspective(0.0, 0.0, 0.8, 0.2, 0.2, mirror=True)])
    c = np.float32([[1, 0, 0, 1], [0, 0, 1, 1], [0, 1, 0, 1]])
    r = R.Renderer(R.Configuration(msaa_sample_count=8, cull_mode=R.Cull.Back, depth_compare=R.Compare.LessEqual, depth_write_enabled=True), device=0)
    scene = R.Scene(r, batch_from_shapes([unit_rect() for _ in range(3)]))
    frame = R.Frame(r, size, size)
    frame.clear()
    frame.clear_depth(1.0)
    scene.render(frame, t, c)
    got = frame.download_depth().reshape(-1, 8).astype(np.float64)
    want, near = perspective_depth_model(t, (0, 1), size, 8)
    ok = ~near
    assert (want[ok] < 1.0).sum() > 2000 and (want[ok] == 1.0).sum() > 2000
    assert ((want[ok] == 1.0) == (got[ok] == 1.0)).all(), "covered samples differ"
    assert np.abs(got[ok] - want[ok]).max() < 1e-5
    # the two squares interpenetrate: each is the nearer surface somewhere
    want, near = perspective_depth_model(t, (0, 1), size, 8)
    only0, _ = perspective_depth_model(t, (0,), size, 8)
    only1, _ = perspective_depth_model(t, (1,), size, 8)
    assert ((want == only0) & (only0 < only1))[~near].sum() > 500 and ((want == only1) & (only1 < only0))[~near].sum() > 500


# ---------------------------------------------------------------- 5. exact internal equalities at 8x

def _render_plain(R, msaa, batch, t, c, size, fmt=None, blending=None, winding_bits=4):
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, winding_counter_bits=winding_bits, blending=blending), device=0)
    scene = R.Scene(r, batch)
    assert scene.status() == 0
    frame = R.Frame(r, size, size, format=fmt)
    frame.clear()
    scene.render(frame, t, c)
    return frame.download(), (r, scene, frame)


def _plain_shapes():
    from contrast_renderer_amd import scenes
    sc = scenes.scene_mixed(24, (256, 256), seed=5)
    return sc


def test_bgra_is_rgba_swapped_at_8x(no_pins):
    R = _R()
    sc = _plain_shapes()
    out = []
    for fmt in (R.FORMAT_RGBA8, R.FORMAT_BGRA8):
        r = R.Renderer(R.Configuration(msaa_sample_count=8, winding_counter_bits=sc["winding_bits"]), device=0)
        scene = R.Scene(r, sc["batch"])
        frame = R.Frame(r, sc["width"], sc["height"], format=fmt)
        frame.clear()
        scene.render(frame, sc["transforms"], sc["colors"])
        out.append(frame.download())
    assert np.array_equal(out[0], out[1][..., [2, 1, 0, 3]]) and (out[0][..., 3] > 0).mean() > 0.05


def test_tile_row_slabs_are_the_frame_rows_at_8x(no_pins):
    R = _R()
    sc = _plain_shapes()
    r = R.Renderer(R.Configuration(msaa_sample_count=8, winding_counter_bits=sc["winding_bits"]), device=0)
    scene = R.Scene(r, sc["batch"])
    w, h = sc["width"], sc["height"]
    frame = R.Frame(r, w, h)
    frame.clear()
    scene.render(frame, sc["transforms"], sc["colors"])
    whole = frame.download()
    for a, b in ((0, 64), (64, 160), (160, h)):
        frame.set_tile_rows(a, b)
        frame.clear()
        scene.render(frame, sc["transforms"], sc["colors"])
        img = frame.download()
        assert np.array_equal(img[a:b], whole[a:b]), (a, b)
        assert not img[:a].any() and not img[b:].any()
    frame.set_tile_rows(0, h)


def test_a_pass_that_draws_nothing_keeps_uploaded_bytes_at_8x(no_pins):
    R = _R()
    rng = np.random.RandomState(3)
    r = R.Renderer(R.Configuration(msaa_sample_count=8), device=0)
    scene = R.Scene(r, batch_from_shapes([unit_rect()]))
    frame = R.Frame(r, 96, 80)
    a = rng.randint(0, 256, (80, 96, 1)).astype(np.uint8)
    image = np.concatenate([np.minimum(rng.randint(0, 256, (80, 96, 3)), a).astype(np.uint8), a], axis=2)  # premultiplied
    frame.upload(image)
    far = box_transform(-40.0, -20.0, -40.0, -20.0, 96, 80)  # off the frame
    scene.render(frame, far[None], np.float32([[1, 0, 0, 1]]))
    assert np.array_equal(frame.download(), image)


def test_a_replace_blend_on_an_opaque_scene_equals_over_at_8x(no_pins):
    R = _R()
    sc = _plain_shapes()
    c = sc["colors"].copy()
    c[:, 3] = 1.0
    args = (sc["batch"], sc["transforms"], c, sc["width"])
    over, _ = _render_plain(R, 8, *args, winding_bits=sc["winding_bits"])
    replace, (_, _, frame) = _render_plain(R, 8, *args, winding_bits=sc["winding_bits"], blending=R.ColorTargetState(R.BlendState.REPLACE))
    from test_gpu_fuzz import last_pass
    assert last_pass(frame)["raster"] == "ops"
    assert np.array_equal(over, replace) and (over[..., 3] > 0).mean() > 0.05


PINS = [("CRH_TRIANGLE_PASS", "1"), ("CRH_EDGE_PASS", "1"), ("CRH_ROWS", "1"), ("CRH_FILL_KERNEL", "0"), ("CRH_NO_ROWS", "1"), ("CRH_LONG_LISTS", "1"),
        ("CRH_NO_DIRECT_LISTS", "1")]


@pytest.mark.parametrize("msaa", NEW)
def test_every_pin_gives_the_same_bytes_and_the_triangle_pass(msaa, no_pins):
    R = _R()
    from contrast_renderer_amd import scenes
    from test_gpu_fuzz import last_pass
    sc = scenes.scene_mixed(300, (512, 384), seed=2)  # >= 256 Shapes: past the small-scene shortcut, into the measured trial at 1x / 4x

    def run():
        r = R.Renderer(R.Configuration(msaa_sample_count=msaa, winding_counter_bits=sc["winding_bits"]), device=0)
        scene = R.Scene(r, sc["batch"])
        frame = R.Frame(r, sc["width"], sc["height"])
        images = []
        for _ in range(24):  # through what would be the trial of the formulations at 1x / 4x
            frame.clear()
            scene.render(frame, sc["transforms"], sc["colors"])
            images.append(frame.download())
            t = last_pass(frame)
            assert t["formulation"] == 2 and not t["measured"] and t["raster"] == "tile" and t["bin"] == "triangles", t
        assert all(np.array_equal(images[0], im) for im in images[1:])
        return images[0]

    base = run()
    assert (base[..., 3] > 0).mean() > 0.05
    for name, value in PINS:
        no_pins.setenv(name, value)
        assert np.array_equal(run(), base), name
        no_pins.delenv(name)


# ---------------------------------------------------------------- 6. a short fuzz

FUZZ_SEEDS = int(os.environ.get("CRH_FUZZ_MSAA_SEEDS", "24"))


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz_fills_at_8x_match_the_model(seed, no_pins):
    """Random polygon fills (self-intersecting ones included) at 8x against the float64 winding model away from edges; the same scene at
    1x and 4x still equals the oracle byte for byte (the shared tile body)."""
    R = _R()
    rng = np.random.RandomState(1000 + seed)
    size = 128
    polys, shapes = [], []
    for _ in range(int(rng.randint(2, 7))):
        pts = rng.uniform(-0.95, 0.95, (int(rng.randint(3, 9)), 2)).astype(np.float32).astype(np.float64)
        shapes.append(([], [Path.from_polygon([tuple(p) for p in pts])]))
    t = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (len(shapes), 1))
    c = np.tile(np.float32([1, 1, 1, 1]), (len(shapes), 1))
    case = T.Case(f"fuzz-{seed}", shapes, t, size, size, msaa=8, winding_bits=4)
    batch = batch_from_shapes(shapes)
    img8, _ = _render_plain(R, 8, batch, t, c, size)
    # a union of opaque white covers: coverage = samples inside any shape (each shape its own stencil pass)
    inside = np.zeros((size * size, 8), dtype=bool)
    near = np.full((size * size, 8), np.inf)
    eps = 0.0
    for s, (_, paths) in enumerate(shapes):
        sub = copy.copy(case)
        sub.shapes, sub.transforms = [shapes[s]], t[s:s + 1]
        ins, sd, e, _ = T.fill_model([paths], min_near=0)(sub)
        inside |= ins
        near = np.minimum(near, np.abs(sd))
        eps = max(eps, e)
    covered = np.rint(img8[..., 3].reshape(-1).astype(np.float64) / 255.0 * 8).astype(int)
    G.check_coverage(covered, inside, near, eps, 0, case.name)
    from oracle.binding import Oracle
    for msaa in (1, 4):
        img, _ = _render_plain(R, msaa, batch, t, c, size)
        assert np.array_equal(img, Oracle(batch).render(size, size, msaa, 4, t, c)), msaa
