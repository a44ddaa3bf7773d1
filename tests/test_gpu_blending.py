"""Configuration::blending (renderer.rs:380-382, the colour cover's pipeline at :736-754) on the GPU: the "over" state keeps the fast paths,
other states run on k_raster_blend and match the oracle (opaque replace) or a float64 per-sample model of the blend (include/contrast_hip.h,
crh_renderer_create_blended), Frame.upload is LoadOp::Load of caller content, and the multi-GPU exchanges handle (or refuse) such layers."""
import math

import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, Path, _ffi
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import BlendComponent as BC
from contrast_renderer_amd.renderer import BlendFactor as F
from contrast_renderer_amd.renderer import BlendOperation as O
from contrast_renderer_amd.renderer import BlendState, ColorTargetState, ColorWrites

import ground_truth_util as G
from test_ground_truth import f32_eps, place

pytestmark = pytest.mark.gpu

OVER = ColorTargetState(BlendState.PREMULTIPLIED_ALPHA_BLENDING)
REPLACE = ColorTargetState(None)
ADD = BC(F.One, F.One, O.Add)


def state(color, alpha=None, mask=ColorWrites.ALL, constant=(0.0, 0.0, 0.0, 0.0)):
    return ColorTargetState(BlendState(color, alpha or color), mask, constant)


STATES = {
    "additive": state(ADD),
    "erase": state(BC(F.Zero, F.OneMinusSrcAlpha, O.Add)),
    "multiply": state(BC(F.Dst, F.Zero, O.Add)),
    "screen": state(BC(F.One, F.OneMinusSrc, O.Add)),
    "subtract": state(BC(F.One, F.One, O.Subtract)),
    "reverse-subtract": state(BC(F.SrcAlpha, F.One, O.ReverseSubtract), BC(F.One, F.OneMinusDstAlpha, O.ReverseSubtract)),
    "min": state(BC(F.One, F.One, O.Min), BC(F.One, F.OneMinusSrcAlpha, O.Add)),
    "max": state(BC(F.One, F.One, O.Max)),
    "saturated": state(BC(F.SrcAlphaSaturated, F.One, O.Add)),
    "constant": state(BC(F.Constant, F.OneMinusConstant, O.Add), BC(F.OneMinusConstant, F.DstAlpha, O.Add), constant=(0.8, 0.3, -0.5, 0.6)),
    "alpha-blending": ColorTargetState(BlendState.ALPHA_BLENDING),
    "replace": REPLACE,
    "mask-RA": state(BC.OVER, mask=ColorWrites.RED | ColorWrites.ALPHA),
    "mask-0": state(ADD, mask=0),
}


def last_pass(frame):
    from test_gpu_fuzz import last_pass as tap
    return tap(frame)


@pytest.fixture
def no_pins(monkeypatch):
    import torch
    assert torch.cuda.is_available()
    from test_gpu_fuzz import _no_path_pins
    _no_path_pins(monkeypatch)


# ---------------------------------------------------------------- the float64 model (include/contrast_hip.h, crh_renderer_create_blended)

def blend(dst, cover, colour, s, attachment):
    """One colour cover, per sample: dst [N, 4] float64, cover [N] bool, colour = straight RGBA f32 -> dst."""
    c = np.float64(colour)
    src = np.clip(np.nan_to_num(np.array([c[0] * c[3], c[1] * c[3], c[2] * c[3], c[3]]), nan=0.0), 0.0, 1.0)
    k = np.clip(np.float64(s.constant), 0.0, 1.0)
    out = dst.copy()
    for ch in range(4):
        comp = (s.blend.alpha if ch == 3 else s.blend.color) if s.blend else None
        d, da = dst[:, ch], dst[:, 3]

        def factor(f):
            return {F.Zero: 0.0, F.One: 1.0, F.Src: src[ch], F.OneMinusSrc: 1.0 - src[ch], F.SrcAlpha: src[3], F.OneMinusSrcAlpha: 1.0 - src[3],
                    F.Dst: d, F.OneMinusDst: 1.0 - d, F.DstAlpha: da, F.OneMinusDstAlpha: 1.0 - da,
                    F.SrcAlphaSaturated: np.minimum(src[3], 1.0 - da) if ch < 3 else 1.0, F.Constant: k[ch], F.OneMinusConstant: 1.0 - k[ch]}[F(f)]
        if comp is None:
            v = np.full_like(d, src[ch])
        elif comp.operation == O.Min:
            v = np.minimum(src[ch], d)
        elif comp.operation == O.Max:
            v = np.maximum(src[ch], d)
        else:
            ps, qd = src[ch] * factor(comp.src_factor), d * factor(comp.dst_factor)
            v = {O.Add: ps + qd, O.Subtract: ps - qd, O.ReverseSubtract: qd - ps}[O(comp.operation)]
        v = np.clip(v, 0.0, 1.0)
        if attachment:
            v = np.floor(v * 255.0 + 0.5) / 255.0
        if (int(s.write_mask) >> ch) & 1:
            out[:, ch] = np.where(cover, v, d)
    return out


def stack(seed=5, size=128, n=28, radius=(6, 36), alpha=(0.15, 0.85)):
    """The translucent disc / rectangle stack of test_ground_truth.colour_cases (same construction): shapes, transforms, colours and each
    shape's signed distance in path coordinates."""
    rng = np.random.RandomState(seed)
    shapes, colours, regions, ts = [], [], [], []
    for k in range(n):
        cx, cy = rng.uniform(20, size - 20, 2)
        if k % 2:
            hx, hy = rng.uniform(radius[0] + 2, radius[1] + 4, 2)
            shapes.append(([], [Path.from_rect((0.0, 0.0), (1.0, hy / hx))]))
            regions.append((lambda a: lambda p: G.convex_polygon(p, [(-1, -a), (-1, a), (1, a), (1, -a)]))(float(np.float32(hy / hx))))
            scale = hx
        else:
            scale = rng.uniform(*radius)
            shapes.append(([], [Path.from_circle((0.0, 0.0), 1.0)]))
            regions.append(lambda p: G.disc(p, (0.0, 0.0), 1.0))
        ts.append(place(size, size, cx, cy, scale, rotate=rng.uniform(0, 1)))
        colours.append([rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(*alpha)])
    return shapes, np.float32(np.stack(ts)), np.float32(colours), regions


def model(size, msaa, layers, s, attachment, background):
    """layers = [(transforms, colours, regions)] drawn in order over `background` (RGBA8, every sample starts at the pixel's value) ->
    (expected [H, W, 4] float64, checkable [H, W]): pixels with a sample within eps of a boundary are not checked."""
    pix = G.samples(size, size, msaa).reshape(-1, 2)
    dst = np.repeat(background.reshape(-1, 4).astype(np.float64) / 255.0, msaa, axis=0)
    near = np.zeros(len(pix), dtype=bool)
    for transforms, colours, regions in layers:
        for t, c, region in zip(transforms, colours, regions):
            sd = region(G.to_path(pix, t, size, size)) * G.min_pixel_scale(t, size, size)
            near |= np.abs(sd) <= f32_eps(size, size, 2 * 40.0)
            dst = blend(dst, sd > 0, c, s, attachment)
    expect = dst.reshape(size * size, msaa, 4).mean(axis=1).reshape(size, size, 4)
    return expect, ~near.reshape(-1, msaa).any(axis=1).reshape(size, size)


def random_background(size, seed=11):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (size, size, 1))
    rgb = np.floor(rng.uniform(0, 1, (size, size, 3)) * (a + 1)).astype(int)  # premultiplied: rgb <= a
    return np.concatenate([rgb, a], axis=2).astype(np.uint8)


def tolerance(name, attachment):
    # RGBA8: the frame blends in f32 and rounds the resolved value once, half a unit. Each blend rounds the factor, two products and the
    # operation (no fma), four roundings of values <= 2; a target error is carried on with a weight of at most 2 (SrcAlphaSaturated: through
    # Ad and D) and at most 1 elsewhere, so 28 blends, the premultiply and the resolve stay far below 512 x 2^-24.
    # RGBA8 attachment: every write is rounded in the model and on the device alike; an f32 value within that bound of a rounding boundary
    # may round the other way, one unit, carried on with weight <= 1 — or <= 2 for SrcAlphaSaturated / One, whose factor reads Ad.
    if not attachment:
        return 0.5 / 255.0 + 512 * G.F32_ULP
    return (2.0 if name == "saturated" else 1.0) / 255.0 + 512 * G.F32_ULP


def compare(image, expect, ok, tol, what):
    got = image.astype(np.float64) / 255.0
    diff = np.abs(got - expect).max(axis=2)
    bad = ok & (diff > tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels off by more than {tol * 255:.3f}/255 (worst {diff[ok].max() * 255:.3f}/255)"
    assert ok.mean() > 0.5


def draws_of(n):
    return [(i, i, op, 0, 0) for i in range(n) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)]


# ---------------------------------------------------------------- 1. the "over" state is the default, on the default paths

@pytest.mark.parametrize("msaa", [1, 4])
def test_explicit_over_state_is_the_default_and_takes_the_fast_path(msaa, no_pins):
    from contrast_renderer_amd import scenes
    sc = scenes.scene_mixed(48, (256, 256), seed=3)
    images = []
    for blending in (None, OVER):
        r = R.Renderer(R.Configuration(msaa_sample_count=msaa, blending=blending), device=0)
        assert r.get_blending() == OVER
        scene = R.Scene(r, sc["batch"])
        frame = R.Frame(r, 256, 256)
        for _ in range(2):  # the verified pass, then one with the lists in place
            frame.clear()
            scene.render(frame, sc["transforms"], sc["colors"])
            images.append(frame.download())
            t = last_pass(frame)
            assert t["general"] == 0 and t["raster"] != "ops", t
    assert all(np.array_equal(images[0], im) for im in images[1:])


# ---------------------------------------------------------------- 2. the generic path, bit for bit: opaque replace == opaque "over"

@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("fmt", [R.FORMAT_RGBA8, R.FORMAT_RGBA8_ATTACHMENT], ids=["rgba8", "attachment"])
def test_opaque_replace_equals_the_oracle_on_the_blend_kernel(msaa, fmt, no_pins):
    from contrast_renderer_amd import scenes
    from oracle.binding import Oracle, render_pass
    size = 192
    sc = scenes.scene_mixed(24, (size, size), seed=9)
    rng = np.random.RandomState(msaa + 10 * fmt)
    t = np.array(sc["transforms"], dtype=np.float32).reshape(-1, 16)
    t[:, 14] = rng.uniform(0.05, 0.95, len(t))  # depths for the Less test with writes
    t[::3, 0:4] *= -1.0  # mirrored instances: back faces for the culling
    c = np.array(sc["colors"], dtype=np.float32).reshape(-1, 4)
    c[:, 3] = 1.0  # opaque: "over" is exactly replace
    n = len(t)
    S, CL, U, COL = R.RenderOperation.Stencil, R.RenderOperation.Clip, R.RenderOperation.UnClip, R.RenderOperation.Color
    draws = [(0, 0, S, 0, 0), (0, 0, CL, 1, 0)]
    draws += [(i, i, op, 1, 0) for i in range(1, n // 2) for op in (S, COL)]
    draws += [(0, 0, U, 0, 0), (1, 1, R.RenderOperation.SaveAlphaContext, 0, 0), (2, 2, S, 0, 0), (2, 2, COL, 0, 0),
              (3, 3, R.RenderOperation.ScaleAlphaContext, 0, 0), (4, 4, R.RenderOperation.RestoreAlphaContext, 0, 0)]
    draws += [(i, i, op, 0, 0) for i in range(n // 2, n) for op in (S, COL)]
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, clip_nesting_counter_bits=2, winding_counter_bits=4, alpha_layer_count=1,
                                   cull_mode=R.Cull.Back, depth_compare=R.Compare.Less, depth_write_enabled=True, blending=REPLACE), device=0)
    assert r.get_blending() == REPLACE
    scene = R.Scene(r, sc["batch"])
    frame = R.Frame(r, size, size, format=fmt)
    o = Oracle(sc["batch"])
    expect, _ = render_pass(o, size, size, msaa, 4, 2, 1, t, c, draws, cull_mode=2, depth_compare=2, depth_write=1,
                            depth=np.ones((size, size), dtype=np.float32), attachment8=fmt == R.FORMAT_RGBA8_ATTACHMENT)
    for _ in range(2):
        frame.clear()
        scene.render_draws(frame, t, c, draws)
        image = frame.download()
        tap = last_pass(frame)
        assert tap["general"] == 1 and tap["raster"] == "ops", tap
        assert np.array_equal(image, expect), f"{int((image != expect).any(axis=2).sum())} pixels differ"
    # the plain (not recorded) pass of the Scene takes the blend kernel too
    plain = R.Renderer(R.Configuration(msaa_sample_count=msaa, blending=REPLACE), device=0)
    scene_plain = R.Scene(plain, sc["batch"])
    frame_plain = R.Frame(plain, size, size, format=fmt)
    frame_plain.clear()
    scene_plain.render(frame_plain, sc["transforms"], c)
    assert last_pass(frame_plain)["raster"] == "ops"
    expect_plain = o.render(size, size, msaa, 4, sc["transforms"], c, attachment8=fmt == R.FORMAT_RGBA8_ATTACHMENT)
    assert np.array_equal(frame_plain.download(), expect_plain)


# ---------------------------------------------------------------- 3. every blend state against the float64 model

@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("name", list(STATES))
def test_blend_states_over_uploaded_content_match_the_model(name, msaa, no_pins):
    s = STATES[name]
    size = 128
    shapes, t, c, regions = stack()
    from contrast_renderer_amd import batch_from_shapes
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, winding_counter_bits=8, clip_nesting_counter_bits=0, blending=s), device=0)
    assert r.get_blending() == ColorTargetState.from_c(s.to_c())
    scene = R.Scene(r, batch_from_shapes(shapes))
    background = random_background(size)
    for fmt in (R.FORMAT_RGBA8, R.FORMAT_RGBA8_ATTACHMENT):
        attachment = fmt == R.FORMAT_RGBA8_ATTACHMENT
        frame = R.Frame(r, size, size, format=fmt)
        frame.upload(background)
        scene.render(frame, t, c)
        image = frame.download()
        tap = last_pass(frame)
        assert tap["general"] == 1 and tap["raster"] == "ops", tap
        expect, ok = model(size, msaa, [(t, c, regions)], s, attachment, background)
        compare(image, expect, ok, tolerance(name, attachment), f"{name} msaa {msaa} fmt {fmt}")
        if name == "mask-0":
            assert np.array_equal(image, background)


# ---------------------------------------------------------------- 4. upload

@pytest.mark.parametrize("msaa", [1, 4])
def test_upload_is_load_of_caller_content(msaa, no_pins):
    from contrast_renderer_amd import scenes
    from oracle.binding import Oracle, render_pass
    size = 160
    sc = scenes.scene_mixed(30, (size, size), seed=4)
    img = random_background(size, seed=msaa)
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa), device=0)
    scene = R.Scene(r, sc["batch"])
    o = Oracle(sc["batch"])
    n = len(np.asarray(sc["colors"]).reshape(-1, 4))
    for fmt in (R.FORMAT_RGBA8, R.FORMAT_RGBA8_ATTACHMENT):
        frame = R.Frame(r, size, size, format=fmt)
        frame.upload(img)
        assert np.array_equal(frame.download(), img)
        frame.clear()
        scene.render(frame, sc["transforms"], sc["colors"])  # a pass into the frame, then the upload replaces it
        frame.upload(img)
        assert np.array_equal(frame.download(), img)
        scene.render_draws(frame, sc["transforms"], sc["colors"], draws_of(n))
        expect, _ = render_pass(o, size, size, msaa, 4, 4, 0, sc["transforms"], sc["colors"], draws_of(n), load=img,
                                attachment8=fmt == R.FORMAT_RGBA8_ATTACHMENT)
        assert np.array_equal(frame.download(), expect)
    with pytest.raises(ContrastError) as e:
        R.Frame(r, size, size, format=R.FORMAT_RGBA16F).upload(img)
    assert e.value.status == _ffi.ERR_INVALID_ARGUMENT
    slab = R.Frame(r, size, size)
    slab.set_tile_rows(0, 64)
    with pytest.raises(ContrastError) as e:
        slab.upload(img)
    assert e.value.status == _ffi.ERR_INVALID_ARGUMENT
    with pytest.raises(ContrastError):
        R.Frame(r, size, size).upload(img[:-1])


# ---------------------------------------------------------------- 5. no double application

def test_additive_over_upload_then_a_much_larger_pass_without_a_clear(no_pins):
    """The second pass has far more entries per tile than the first: its tile lists are grown before it is drawn (a frame that is not cleared
    is never drawn twice). The uploaded background is neither lost nor added twice, nor is the first pass."""
    from contrast_renderer_amd import batch_from_shapes
    size = 128
    s = STATES["additive"]
    shapes_a, ta, ca, regions_a = stack()
    ca[:, 3] *= 0.3
    shapes_b, tb, cb, regions_b = stack(seed=8, n=1500, radius=(2, 7), alpha=(0.01, 0.04))
    r = R.Renderer(R.Configuration(msaa_sample_count=1, winding_counter_bits=8, clip_nesting_counter_bits=0, blending=s), device=0)
    scene_a, scene_b = R.Scene(r, batch_from_shapes(shapes_a)), R.Scene(r, batch_from_shapes(shapes_b))
    background = random_background(size, seed=3) // 3
    frame = R.Frame(r, size, size)
    frame.upload(background)
    scene_a.render(frame, ta, ca)
    first = frame.download()
    expect, ok = model(size, 1, [(ta, ca, regions_a)], s, False, background)
    compare(first, expect, ok, tolerance("additive", False), "first pass")
    scene_b.render(frame, tb, cb)  # no clear: loads the first pass' RGBA8 image
    expect, ok = model(size, 1, [(tb, cb, regions_b)], s, False, first)
    compare(frame.download(), expect, ok, tolerance("additive", False), "second pass")


@pytest.mark.parametrize("msaa", [1, 4])
def test_additive_pass_split_over_two_calls_equals_one_call(msaa, no_pins):
    from contrast_renderer_amd import batch_from_shapes
    shapes, t, c, _ = stack()
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, winding_counter_bits=8, clip_nesting_counter_bits=0, blending=STATES["additive"]), device=0)
    scene = R.Scene(r, batch_from_shapes(shapes))
    draws = draws_of(len(shapes))
    whole = R.Frame(r, 128, 128)
    whole.clear()
    scene.render_draws(whole, t, c, draws)
    split = R.Frame(r, 128, 128)
    split.clear()
    split.keep_pass_state()
    scene.render_draws(split, t, c, draws[:23])
    scene.render_draws(split, t, c, draws[23:])
    assert last_pass(split)["raster"] == "ops"
    assert np.array_equal(whole.download(), split.download())


# ---------------------------------------------------------------- 6. the multi-GPU exchanges

def test_loopback_exchanges_refuse_path_split_layers_and_gather_tile_slabs(no_pins):
    from contrast_renderer_amd import batch_from_shapes
    size, world = 128, 2
    shapes, t, c, _ = stack()
    r = R.Renderer(R.Configuration(msaa_sample_count=1, winding_counter_bits=8, clip_nesting_counter_bits=0, blending=STATES["additive"]), device=0)
    scene = R.Scene(r, batch_from_shapes(shapes))
    scene.set_instances(t, c)
    comms = [R.Comm(r, 0, world)]
    comms += [R.Comm(r, k, world, rank0=comms[0]) for k in range(1, world)]
    result = R.Frame(r, size, size)
    # the path split composites layers with "over": not what this renderer drew
    layers = [R.Frame(r, size, size) for _ in range(world)]
    for f in layers:
        f.clear()
        scene.render(f)
    with pytest.raises(ContrastError) as e:
        comms[0].local_exchange(layers, result)
    assert e.value.status == _ffi.ERR_UNSUPPORTED
    # the tile split moves pixels only
    whole = R.Frame(r, size, size)
    whole.clear()
    scene.render(whole)
    expect = whole.download()
    for rank, f in enumerate(layers):
        f.set_tile_rows(*R.slab_rows(size, rank, world))
        f.clear()
        scene.render(f)
    comms[0].local_gather_slabs(layers, result)
    assert np.array_equal(result.download(), expect)
    assert math.isfinite(float(expect.mean())) and expect[..., 3].max() > 0
