"""The BGRA / sRGB frame formats on the GPU (include/contrast_hip.h at CRH_FORMAT_BGRA8 .. CRH_FORMAT_BGRA8_SRGB_ATTACHMENT).

BGRA frames are checked byte for byte against the oracle's RGBA8 image with channels 0 and 2 swapped (f32 mode) or against the library's
RGBA8 attachment frame of the same scene; sRGB frames against things the kernels do not compute: the committed codec on the host, the
oracle's choice of colour in opaque scenes, a float32 model of pixel-aligned translucent stacks, and the RGBA16F frame of the same scene."""
import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, Path, _ffi, scenes
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import BlendComponent as BC
from contrast_renderer_amd.renderer import BlendFactor as F
from contrast_renderer_amd.renderer import BlendOperation as O
from contrast_renderer_amd.renderer import BlendState, ColorTargetState, TextureFormat

from test_formats_cpu import committed_tables, decode, encode

pytestmark = pytest.mark.gpu

SWAP = [2, 1, 0, 3]


def last_pass(frame):
    from test_gpu_fuzz import last_pass as tap
    return tap(frame)


@pytest.fixture
def no_pins(monkeypatch):
    import torch
    assert torch.cuda.is_available()
    from test_gpu_fuzz import _no_path_pins
    _no_path_pins(monkeypatch)


def draw(r, batch, fmt, width, height, transforms, colors, upload=None, passes=1):
    scene = R.Scene(r, batch)
    assert scene.status() == 0
    frame = R.Frame(r, width, height, fmt)
    for _ in range(passes):  # (each pass over a cleared frame or the upload: the later ones with the tile lists in place)
        frame.clear()
        if upload is not None:
            frame.upload(upload)
        scene.render(frame, transforms, colors)
    return frame.download(), last_pass(frame)


# ---------------------------------------------------------------- 1. the codec the kernels run

def test_device_codec_equals_the_host_tables(no_pins):
    d, t = committed_tables()
    r = R.Renderer(R.Configuration(), device=0)
    near = []
    for k in range(1, 256):
        bits = int(t[k].view(np.uint32))
        near.append(np.arange(bits - 6, bits + 7, dtype=np.uint32).view(np.float32))
    rng = np.random.RandomState(3)
    special = np.array([0.0, -0.0, -1e-30, -0.5, -np.inf, 1.0, 1.0000001, 7.0, np.inf, np.nan, -np.nan, 1e-45, 3e-3, 0.0031308], dtype=np.float32)
    x = np.concatenate([d, np.concatenate(near), special, rng.uniform(-0.1, 1.1, 700_000).astype(np.float32),
                        np.exp(rng.uniform(np.log(1e-8), 0.0, 300_000)).astype(np.float32)])
    codes, decoded = r.selftest_srgb(x)
    assert np.array_equal(decoded.view(np.uint32), d.view(np.uint32))
    want = encode(x)
    bad = np.nonzero(codes != want)[0]
    assert bad.size == 0, [(float(x[i]), int(codes[i]), int(want[i])) for i in bad[:8]]
    assert np.array_equal(codes[:256], np.arange(256))


# ---------------------------------------------------------------- 2. BGRA is RGBA with channels 0 and 2 swapped, on every formulation

def fill_scene(seed, msaa):
    from test_gpu_fuzz import fill_case
    c = fill_case(seed, n_frames=2)
    assert c["msaa"] == msaa
    return c


@pytest.mark.parametrize("pin", [None, ("CRH_TRIANGLE_PASS", "1"), ("CRH_ROWS", "1"), ("CRH_FILL_KERNEL", "0")], ids=["default", "triangles", "rows", "no-fill"])
@pytest.mark.parametrize("seed,msaa", [(0, 1), (3, 4)])
def test_bgra_fill_scenes_are_the_oracles_rgba_swapped(seed, msaa, pin, no_pins, monkeypatch, oracle_lib):
    from oracle.binding import Oracle
    if pin:
        monkeypatch.setenv(*pin)
    c = fill_scene(seed, msaa)
    o = Oracle(c["batch"])
    t = c["frames"][-1]
    expect = o.render(c["width"], c["height"], c["msaa"], c["winding_bits"], t, c["colors"])
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, clip_nesting_counter_bits=2, winding_counter_bits=c["winding_bits"]), device=0)
    taps = {}
    images = {}
    for fmt in (R.FORMAT_RGBA8, R.FORMAT_BGRA8, R.FORMAT_RGBA8_ATTACHMENT, R.FORMAT_BGRA8_ATTACHMENT):
        images[fmt], taps[fmt] = draw(r, c["batch"], fmt, c["width"], c["height"], t, c["colors"], passes=2)
    assert np.array_equal(images[R.FORMAT_RGBA8], expect)
    assert np.array_equal(images[R.FORMAT_BGRA8], expect[..., SWAP])
    assert np.array_equal(images[R.FORMAT_BGRA8_ATTACHMENT], images[R.FORMAT_RGBA8_ATTACHMENT][..., SWAP])
    assert taps[R.FORMAT_BGRA8] == taps[R.FORMAT_RGBA8] and taps[R.FORMAT_BGRA8_ATTACHMENT] == taps[R.FORMAT_RGBA8_ATTACHMENT], taps


@pytest.mark.parametrize("msaa", [1, 4])
def test_bgra_strokes_recorded_passes_and_uploads(msaa, no_pins, oracle_lib):
    """Strokes on the edge path; a recorded pass with Clip and alpha contexts (the triangle path's general kernel); a pass over uploaded
    BGRA bytes; an additive blend state (k_raster_blend): each the RGBA frame's bytes, swapped."""
    from oracle.binding import Oracle
    sc = scenes.scene_mixed(40, (200, 168), seed=11)
    o = Oracle(sc["batch"])
    cfg = dict(msaa_sample_count=msaa, winding_counter_bits=sc["winding_bits"], alpha_layer_count=2)
    r = R.Renderer(R.Configuration(**cfg), device=0)
    w, h = sc["width"], sc["height"]
    rgba, tap = draw(r, sc["batch"], R.FORMAT_RGBA8, w, h, sc["transforms"], sc["colors"])
    assert np.array_equal(rgba, o.render(w, h, msaa, sc["winding_bits"], sc["transforms"], sc["colors"]))
    bgra, tap_b = draw(r, sc["batch"], R.FORMAT_BGRA8, w, h, sc["transforms"], sc["colors"])
    assert np.array_equal(bgra, rgba[..., SWAP]) and tap == tap_b
    # recorded pass: Clip by shape 0, an opacity group of shapes 1-5, colours of the rest
    Op = R.RenderOperation
    draws = [(0, 0, Op.Stencil, 0, 0), (0, 0, Op.Clip, 0, 0)]
    draws += [(1, 1, Op.Stencil, 1, 0), (1, 1, Op.SaveAlphaContext, 1, 0)]
    draws += [(i, i, op, 1, 0) for i in range(2, 6) for op in (Op.Stencil, Op.Color)]
    draws += [(1, 1, Op.ScaleAlphaContext, 1, 0), (1, 1, Op.Stencil, 1, 0), (1, 1, Op.RestoreAlphaContext, 1, 0)]
    draws += [(i, i, op, 1, 0) for i in range(6, 20) for op in (Op.Stencil, Op.Color)]
    background = np.random.RandomState(2).randint(0, 256, (h, w, 4)).astype(np.uint8)
    background[..., :3] = np.minimum(background[..., :3], background[..., 3:])
    out = {}
    for fmt in (R.FORMAT_RGBA8, R.FORMAT_BGRA8, R.FORMAT_RGBA8_ATTACHMENT, R.FORMAT_BGRA8_ATTACHMENT):
        scene = R.Scene(r, sc["batch"])
        frame = R.Frame(r, w, h, fmt)
        frame.upload(background if fmt in (R.FORMAT_RGBA8, R.FORMAT_RGBA8_ATTACHMENT) else background[..., SWAP])
        scene.render_draws(frame, sc["transforms"], sc["colors"], draws)
        out[fmt] = (frame.download(), last_pass(frame))
    assert out[R.FORMAT_RGBA8][1]["formulation"] == 2 and out[R.FORMAT_RGBA8][1]["general"] == 1
    for a, b in ((R.FORMAT_RGBA8, R.FORMAT_BGRA8), (R.FORMAT_RGBA8_ATTACHMENT, R.FORMAT_BGRA8_ATTACHMENT)):
        assert np.array_equal(out[b][0], out[a][0][..., SWAP]) and out[a][1] == out[b][1]
    # a blend state other than "over"
    add = ColorTargetState(BlendState(BC(F.One, F.One, O.Add), BC(F.One, F.One, O.Add)))
    ra = R.Renderer(R.Configuration(blending=add, **cfg), device=0)
    for a, b in ((R.FORMAT_RGBA8, R.FORMAT_BGRA8), (R.FORMAT_RGBA8_ATTACHMENT, R.FORMAT_BGRA8_ATTACHMENT)):
        ia, ta = draw(ra, sc["batch"], a, w, h, sc["transforms"], sc["colors"], upload=background if a == R.FORMAT_RGBA8 else background)
        ib, tb = draw(ra, sc["batch"], b, w, h, sc["transforms"], sc["colors"], upload=background[..., SWAP])
        assert np.array_equal(ib, ia[..., SWAP]) and ta == tb and ta["raster"] == "ops"


def test_frame_defaults_to_the_renderers_format(no_pins):
    for tf in TextureFormat:
        r = R.Renderer(R.Configuration(blending=ColorTargetState(BlendState.PREMULTIPLIED_ALPHA_BLENDING, format=tf)), device=0)
        assert r.get_blending().format == tf
        f = R.Frame(r, 16, 16)
        fmt = C_format(f)
        assert fmt == int(tf) and f.format == int(tf)
    assert C_format(R.Frame(R.Renderer(R.Configuration(), device=0), 16, 16)) == R.FORMAT_RGBA8


def C_format(frame):
    import ctypes as C
    out = C.c_uint32()
    _ffi.check(frame.lib.crh_frame_format(frame.handle, C.byref(out)))
    return out.value


# ---------------------------------------------------------------- 3. sRGB, opaque scenes at msaa 1: the last colour, encoded

@pytest.mark.parametrize("pin", [None, ("CRH_TRIANGLE_PASS", "1"), ("CRH_EDGE_PASS", "1"), ("CRH_ROWS", "1"), ("CRH_FILL_KERNEL", "0")],
                         ids=["default", "triangles", "edges", "rows", "no-fill"])
@pytest.mark.parametrize("family", ["fill", "mixed"])
def test_srgb_opaque_scenes_are_the_encoded_last_colour(family, pin, no_pins, monkeypatch, oracle_lib):
    from oracle.binding import Oracle
    if pin:
        monkeypatch.setenv(*pin)
    if family == "fill":
        c = fill_scene(0, 1)
        batch, t, w, h, wb = c["batch"], c["frames"][-1], c["width"], c["height"], c["winding_bits"]
    else:
        sc = scenes.scene_mixed(36, (160, 144), seed=5)
        batch, t, w, h, wb = sc["batch"], sc["transforms"], sc["width"], sc["height"], sc["winding_bits"]
    n = batch.n_shapes
    rng = np.random.RandomState(7)
    codes = rng.choice(255 ** 3, n, replace=False)
    colours = np.stack([(codes % 255 + 1) / 255.0 - 0.3 / 255.0, ((codes // 255) % 255 + 1) / 255.0 - 0.2 / 255.0, (codes // 65025 + 1) / 255.0 - 0.1 / 255.0,
                        np.ones(n)], axis=1).astype(np.float32)
    unorm = np.floor(colours[:, :3].astype(np.float32) * np.float32(255.0) + np.float32(0.5)).astype(np.int64)
    assert len({tuple(u) for u in unorm}) == n
    expect_rgba = Oracle(batch).render(w, h, 1, wb, t, colours)
    index = {tuple(u): k for k, u in enumerate(unorm)}
    lut = np.concatenate([encode(colours[:, :3]), np.full((n, 1), 255, np.uint8)], axis=1)
    ids = np.array([index.get(tuple(p[:3].astype(np.int64)), -1) if p[3] else -2 for p in expect_rgba.reshape(-1, 4)])
    assert (ids != -1).all()
    expect = np.where((ids >= 0)[:, None], lut[np.maximum(ids, 0)], 0).reshape(h, w, 4).astype(np.uint8)
    assert (ids >= 0).any()
    r = R.Renderer(R.Configuration(msaa_sample_count=1, winding_counter_bits=wb), device=0)
    rgba, tap = draw(r, batch, R.FORMAT_RGBA8, w, h, t, colours)
    assert np.array_equal(rgba, expect_rgba)
    for fmt in (R.FORMAT_RGBA8_SRGB, R.FORMAT_RGBA8_SRGB_ATTACHMENT, R.FORMAT_BGRA8_SRGB):
        img, tap_s = draw(r, batch, fmt, w, h, t, colours)
        want = expect[..., SWAP] if fmt == R.FORMAT_BGRA8_SRGB else expect
        assert np.array_equal(img, want), f"format {fmt}: {(img != want).any(axis=2).sum()} pixels differ"
        assert tap_s == tap


# ---------------------------------------------------------------- 4. sRGB translucent stacks: a float32 model in the kernels' order

def rect_stack(size, n, seed):
    rng = np.random.RandomState(seed)
    x0, y0 = rng.randint(0, size - 8, n), rng.randint(0, size - 8, n)
    x1, y1 = x0 + rng.randint(4, size // 2, n), y0 + rng.randint(4, size // 2, n)
    x1, y1 = np.minimum(x1, size + 3), np.minimum(y1, size + 3)
    paths = [([], [Path.from_rect(((a + c) / 2.0, (b + d) / 2.0), ((c - a) / 2.0, (d - b) / 2.0))]) for a, b, c, d in zip(x0, y0, x1, y1)]
    colours = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(0.1, 0.9, (n, 1))], axis=1).astype(np.float32)
    return paths, (x0, y0, x1, y1), colours


def model_stack(size, msaa, boxes, colours, fmt, blend, start):
    """Per pixel (every sample of a pixel-aligned rectangle is covered alike): the kernels' operation order, f32 (oracle/raster.hpp)."""
    f = np.float32
    srgb_att = fmt in (R.FORMAT_RGBA8_SRGB_ATTACHMENT, R.FORMAT_BGRA8_SRGB_ATTACHMENT)
    d = start.astype(np.float32).copy()  # [size, size, 4] linear, y-up rows
    for (a, b, c, e), col in zip(zip(*boxes), colours):
        src = np.array([col[0] * col[3], col[1] * col[3], col[2] * col[3], col[3]], dtype=np.float32)
        region = d[max(b, 0):min(e, size), max(a, 0):min(c, size)]
        if blend == "over":
            new = src + region * (f(1.0) - src[3])
        else:
            s = np.clip(src, 0, 1)
            if blend == "additive":
                new = s * f(1.0) + region * f(1.0)
            else:  # erase: Zero, OneMinusSrcAlpha
                new = s * f(0.0) + region * (f(1.0) - s[3])
            new = np.clip(new, 0, 1).astype(np.float32)
        if srgb_att:
            new = np.concatenate([decode(encode(new[..., :3])), (np.floor(np.clip(new[..., 3:], 0, 1) * f(255.0) + f(0.5)) / f(255.0)).astype(np.float32)], axis=-1)
        region[...] = new
    s = np.zeros_like(d)
    for _ in range(msaa):
        s = (s + d).astype(np.float32)
    avg = (s * f(1.0 / msaa)).astype(np.float32)
    out = np.concatenate([encode(avg[..., :3]), np.floor(np.clip(avg[..., 3:], 0, 1) * f(255.0) + f(0.5)).astype(np.uint8)], axis=-1)
    return out[::-1]  # row 0 = top


def loaded(image):
    """What a load reads of an sRGB RGBA image (row 0 = top) -> linear, y-up rows."""
    lin = np.concatenate([decode(image[..., :3]), image[..., 3:].astype(np.float32) * np.float32(1.0 / 255.0)], axis=-1)
    return lin[::-1].astype(np.float32)


@pytest.mark.parametrize("blend", ["over", "additive", "erase"])
@pytest.mark.parametrize("fmt", [R.FORMAT_RGBA8_SRGB, R.FORMAT_RGBA8_SRGB_ATTACHMENT, R.FORMAT_BGRA8_SRGB_ATTACHMENT])
@pytest.mark.parametrize("msaa", [1, 4])
def test_srgb_translucent_rect_stacks_match_the_float32_model(msaa, fmt, blend, no_pins):
    from contrast_renderer_amd import batch_from_shapes
    size = 64
    paths, boxes, colours = rect_stack(size, 24, seed=msaa * 10 + fmt)
    batch = batch_from_shapes(paths)
    t = np.tile(scenes.ortho_pixels(size, size), (len(paths), 1))
    states = {"over": None, "additive": ColorTargetState(BlendState(BC(F.One, F.One, O.Add), BC(F.One, F.One, O.Add))),
              "erase": ColorTargetState(BlendState(BC(F.Zero, F.OneMinusSrcAlpha, O.Add), BC(F.Zero, F.OneMinusSrcAlpha, O.Add)))}
    r = R.Renderer(R.Configuration(msaa_sample_count=msaa, blending=states[blend]), device=0)
    scene = R.Scene(r, batch)
    frame = R.Frame(r, size, size, fmt)
    swap = SWAP if fmt == R.FORMAT_BGRA8_SRGB_ATTACHMENT else [0, 1, 2, 3]
    # pass 1 over a clear frame, pass 2 loads its result; then a pass over uploaded sRGB bytes
    frame.clear()
    half = len(paths) // 2
    scene.render_draws(frame, t, colours, [(i, i, op, 0, 0) for i in range(half) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)])
    first = frame.download()[..., swap]
    expect1 = model_stack(size, msaa, [b[:half] for b in boxes], colours[:half], fmt, blend, np.zeros((size, size, 4), np.float32))
    assert np.array_equal(first, expect1), f"pass 1: {(first != expect1).any(axis=2).sum()} pixels differ"
    scene.render_draws(frame, t, colours, [(i, i, op, 0, 0) for i in range(half, len(paths)) for op in (R.RenderOperation.Stencil, R.RenderOperation.Color)])
    second = frame.download()[..., swap]
    expect2 = model_stack(size, msaa, [b[half:] for b in boxes], colours[half:], fmt, blend, loaded(first))
    assert np.array_equal(second, expect2), f"pass 2: {(second != expect2).any(axis=2).sum()} pixels differ"
    background = np.random.RandomState(4).randint(0, 256, (size, size, 4)).astype(np.uint8)
    frame.upload(background[..., swap])
    scene.render(frame, t, colours)
    third = frame.download()[..., swap]
    expect3 = model_stack(size, msaa, boxes, colours, fmt, blend, loaded(background))
    assert np.array_equal(third, expect3), f"upload: {(third != expect3).any(axis=2).sum()} pixels differ"


# ---------------------------------------------------------------- 5. sRGB on real scenes: the RGBA16F frame's colours, encoded

def f16_interval_codes(f):
    """encode of the ends of every f16 value's rounding interval (the exact f32 colour lies within it)."""
    f = f.astype(np.float32)
    lo = np.nextafter(f.astype(np.float16), np.float16(-np.inf)).astype(np.float32)
    hi = np.nextafter(f.astype(np.float16), np.float16(np.inf)).astype(np.float32)
    return encode((f + lo) * np.float32(0.5)), encode((f + hi) * np.float32(0.5))


@pytest.mark.parametrize("which", ["s10k", "glyphs", "dashed"])
@pytest.mark.parametrize("msaa", [1, 4])
def test_srgb_real_scenes_are_the_rgba16f_colours_encoded(which, msaa, no_pins, monkeypatch):
    if which == "s10k":
        sc = scenes.scene_cubic_fill(n_paths=1500, size=(512, 512))
    elif which == "glyphs":
        sc = scenes.scene_glyphs(n_glyphs=600, size=(384, 384))
    else:
        sc = scenes.scene_dashed_strokes(n_paths=200, size=(384, 384), msaa=msaa)
    w, h = sc["width"], sc["height"]
    pins = [None, ("CRH_TRIANGLE_PASS", "1"), ("CRH_EDGE_PASS", "1")] + ([("CRH_ROWS", "1"), ("CRH_FILL_KERNEL", "0")] if msaa == 1 else [])
    results = []
    for pin in pins:
        if pin:
            monkeypatch.setenv(*pin)
        r = R.Renderer(R.Configuration(msaa_sample_count=msaa, winding_counter_bits=sc["winding_bits"]), device=0)
        srgb, _ = draw(r, sc["batch"], R.FORMAT_RGBA8_SRGB, w, h, sc["transforms"], sc["colors"])
        results.append(srgb)
        if pin is None:
            f16, _ = draw(r, sc["batch"], R.FORMAT_RGBA16F, w, h, sc["transforms"], sc["colors"])
            rgba, _ = draw(r, sc["batch"], R.FORMAT_RGBA8, w, h, sc["transforms"], sc["colors"])
            bgra, _ = draw(r, sc["batch"], R.FORMAT_BGRA8_SRGB, w, h, sc["transforms"], sc["colors"])
            assert np.array_equal(bgra, srgb[..., SWAP])
            assert np.array_equal(srgb[..., 3], rgba[..., 3])
            exact = encode(f16[..., :3].astype(np.float32))
            lo, hi = f16_interval_codes(f16[..., :3])
            ok = (srgb[..., :3] == exact) | ((lo != hi) & ((srgb[..., :3] == lo) | (srgb[..., :3] == hi)))
            assert ok.all(), f"{int((~ok).sum())} channels differ from the encoded RGBA16F colour"
            assert (srgb[..., 3] > 0).mean() > 0.02
        if pin:
            monkeypatch.delenv(pin[0])
    for k, img in enumerate(results[1:], 1):
        assert np.array_equal(img, results[0]), f"pin {pins[k]}: {(img != results[0]).any(axis=2).sum()} pixels differ"


# ---------------------------------------------------------------- 6. errors and the multi-GPU entry points

def test_format_errors(no_pins):
    r = R.Renderer(R.Configuration(), device=0)
    with pytest.raises(ContrastError):
        R.Frame(r, 16, 16, 9)
    for fmt in range(3, 9):
        f = R.Frame(r, 16, 16, fmt)
        f.clear()
        assert (f.download() == 0).all()
        out = np.zeros((16, 16, 4), np.float16)
        assert f.lib.crh_frame_download_f16(f.handle, out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT


def test_loopback_exchange_and_gathers_with_the_new_formats(no_pins):
    sc = scenes.scene_mixed(30, (128, 96), seed=2)
    w, h, world = sc["width"], sc["height"], 2
    r = R.Renderer(R.Configuration(msaa_sample_count=1, winding_counter_bits=sc["winding_bits"]), device=0)
    scene = R.Scene(r, sc["batch"])
    comms = [R.Comm(r, 0, world)]
    comms.append(R.Comm(r, 1, world, rank0=comms[0]))

    def layers(fmt, slabs):
        out = []
        for k in range(world):
            f = R.Frame(r, w, h, fmt)
            if slabs:
                f.set_tile_rows(*R.slab_rows(h, k, world))
            f.clear()
            scene.render(f, sc["transforms"], sc["colors"])
            out.append(f)
        return out

    for fmt in (R.FORMAT_BGRA8, R.FORMAT_RGBA8_SRGB):
        with pytest.raises(ContrastError) as e:
            comms[0].local_exchange(layers(fmt, False), R.Frame(r, w, h, R.FORMAT_RGBA8))
        assert e.value.status == _ffi.ERR_UNSUPPORTED
    with pytest.raises(ContrastError) as e:
        comms[0].local_exchange(layers(R.FORMAT_RGBA8, False), R.Frame(r, w, h, R.FORMAT_BGRA8))
    assert e.value.status == _ffi.ERR_UNSUPPORTED
    for fmt, att in ((R.FORMAT_BGRA8, R.FORMAT_BGRA8_ATTACHMENT), (R.FORMAT_RGBA8_SRGB, R.FORMAT_RGBA8_SRGB_ATTACHMENT), (R.FORMAT_BGRA8_SRGB, R.FORMAT_BGRA8_SRGB)):
        whole, _ = draw(r, sc["batch"], fmt, w, h, sc["transforms"], sc["colors"])
        result = R.Frame(r, w, h, att)  # X and X_ATTACHMENT store one encoding
        comms[0].local_gather_slabs(layers(fmt, True), result)
        assert np.array_equal(result.download(), whole)
        with pytest.raises(ContrastError) as e:
            comms[0].local_gather_slabs(layers(fmt, True), R.Frame(r, w, h, R.FORMAT_RGBA8))
        assert e.value.status == _ffi.ERR_INVALID_ARGUMENT
    mixed = layers(R.FORMAT_BGRA8, True)[:1] + layers(R.FORMAT_RGBA8, True)[1:]
    with pytest.raises(ContrastError) as e:
        comms[0].local_gather_slabs(mixed, R.Frame(r, w, h, R.FORMAT_BGRA8))
    assert e.value.status == _ffi.ERR_INVALID_ARGUMENT
