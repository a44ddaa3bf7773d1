"""Mipmapped image paints without a GPU: crh_image_paint_validate with CRH_FILTER_MIPMAP (host only), the Python / C++ / Rust mirrors of the new
entry points, and the float64 model of tests/mip_model.py alone — the chain by hand, lod at its corners, and its caps on every scene
tests/test_gpu_mipmaps.py draws."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, Filter, ImagePaint, Spread, _ffi
from contrast_renderer_amd import renderer as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
NAMES = ("crh_image_generate_mipmaps", "crh_image_level_count", "crh_image_download_level")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def raw(filter):
    c = _ffi.ImagePaintC()
    c.image, c.filter, c.spread_x, c.spread_y = 0x1000, filter, 0, 0  # (the handle is only compared with null)
    for i in range(6):
        c.m[i] = IDENTITY[i]
    return c


@pytest.mark.parametrize("filter", [0, 1, 0x100, 0x101])
def test_validate_accepts_the_four_filter_words(lib, filter):
    assert lib.crh_image_paint_validate(C.byref(raw(filter))) == _ffi.OK


@pytest.mark.parametrize("filter", [2, 5, 0x102, 0x200, 0x300, 0x1101])
def test_validate_still_refuses_every_other_filter_word(lib, filter):
    assert lib.crh_image_paint_validate(C.byref(raw(filter))) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode() == "crh_image_paint: unknown filter"


def test_the_taps_refuse_null_arguments_without_a_device(lib):
    n = C.c_uint32(7)
    assert lib.crh_image_generate_mipmaps(None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_image_level_count(None, C.byref(n)) == _ffi.ERR_INVALID_ARGUMENT and n.value == 7
    assert lib.crh_image_download_level(None, 0, None, None, None) == _ffi.ERR_INVALID_ARGUMENT
    assert C.sizeof(_ffi.ImagePaintC) == 48  # crh_image_paint keeps its size: the flag lives in the filter word


def test_the_library_exports_and_a_fresh_ffi_rs_declares_the_new_symbols(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    for ffi in (committed, fresh):
        assert "pub const CRH_FILTER_MIPMAP: u32 = 0x100;" in ffi and "pub const CRH_FILTER_LINEAR: u32 = 1;" in ffi
        assert re.search(r"pub fn crh_image_generate_mipmaps\(image: \*mut crh_image\) -> crh_status;", ffi)
        assert re.search(r"pub fn crh_image_level_count\(image: \*const crh_image, count: \*mut u32\) -> crh_status;", ffi)
        assert re.search(r"pub fn crh_image_download_level\(image: \*const crh_image, level: u32, rgba8: \*mut c_void, width: \*mut u32, height: \*mut u32\) -> crh_status;", ffi)
    assert committed == fresh
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub fn generate_mipmaps(&mut self) -> Result<(), Error>", "pub fn levels(&self) -> Result<u32, Error>",
                 "pub fn download_level(&self, level: u32) -> Result<(u32, u32, Vec<u8>), Error>", "NearestMipmap = 0x100,", "LinearMipmap = 0x101,"):
        assert text in shim, text


def test_the_cpp_mirror_of_mipmaps_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mipmaps_harness.cpp"),
               "-o", os.path.join(tmp, "mipmaps_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


class _Handle:  # stands for an Image where no device is at hand: ImagePaint only carries it
    def __init__(self, handle, width=8, height=4):
        self.handle, self.width, self.height = handle, width, height


def test_the_python_mirror_round_trips_the_flag(lib):
    assert (int(Filter.NearestMipmap), int(Filter.LinearMipmap)) == (0x100, 0x101)
    assert Filter.LinearMipmap == Filter.Linear | 0x100 and Filter(0x101) is Filter.LinearMipmap
    image = _Handle(0x2000)
    for f in (Filter.NearestMipmap, Filter.LinearMipmap):
        paint = ImagePaint(image, IDENTITY, f, Spread.Repeat, Spread.Reflect)
        c = paint.to_c()
        assert (c.image, c.filter, c.spread_x, c.spread_y, tuple(c.m)) == (0x2000, int(f), 1, 2, IDENTITY)
        paint.validate()
        assert paint != ImagePaint(image, IDENTITY, Filter(int(f) & 1), Spread.Repeat, Spread.Reflect)
    assert ImagePaint.fit(image, (0, 0), (1, 1), Filter.LinearMipmap).filter == Filter.LinearMipmap
    for bad in (2, 5, 0x102, 0x200):
        with pytest.raises(ContrastError):
            ImagePaint(image, IDENTITY, filter=bad).validate()
    for name in ("generate_mipmaps", "levels", "download_level"):
        assert hasattr(R.Image, name)


# ---------------------------------------------------------------- the float64 model alone

def test_the_chain_by_hand():
    import mip_model as MM
    # 1 x 1: one level, itself
    one = np.uint8([[[9, 8, 7, 200]]])
    assert MM.level_count(1, 1) == 1 and len(MM.chain(one)) == 1 and np.array_equal(MM.chain(one)[0], one)
    # 1 x 7 (width 7, height 1): 7 -> 3 -> 1, rows clamped to the one row; the odd width drops its last column at each step
    row = np.zeros((1, 7, 4), dtype=np.uint8)
    row[0, :, 0] = [10, 20, 30, 41, 50, 61, 255]
    row[..., 3] = 255
    levels = MM.chain(row)
    assert [l.shape[:2] for l in levels] == [(1, 7), (1, 3), (1, 1)]
    assert levels[1][0, :, 0].tolist() == [(10 + 20 + 10 + 20 + 2) >> 2, (30 + 41 + 30 + 41 + 2) >> 2, (50 + 61 + 50 + 61 + 2) >> 2] == [15, 36, 56]
    assert levels[2][0, 0, 0] == (15 + 36 + 15 + 36 + 2) >> 2 == 26 and (levels[1][..., 3] == 255).all() and levels[2][0, 0, 3] == 255
    # 5 x 3 (width 5, height 3): -> 2 x 1 -> 1 x 1
    img = np.arange(3 * 5 * 4, dtype=np.uint8).reshape(3, 5, 4) * 4
    levels = MM.chain(img)
    assert [l.shape[:2] for l in levels] == [(3, 5), (1, 2), (1, 1)]
    t = img.astype(int)
    assert np.array_equal(levels[1][0, 0], (t[0, 0] + t[0, 1] + t[1, 0] + t[1, 1] + 2) >> 2) and np.array_equal(levels[1][0, 1], (t[0, 2] + t[0, 3] + t[1, 2] + t[1, 3] + 2) >> 2)
    a, b = levels[1][0, 0].astype(int), levels[1][0, 1].astype(int)
    assert np.array_equal(levels[2][0, 0], (a + b + a + b + 2) >> 2)  # the one row stands for both rows of the block
    # 8 x 8: four levels, each texel the rounded mean of its block; rounding is half up on the sum (1 + 0 + 0 + 0 + 2) >> 2 = 0, (1 + 1 + 0 + 0 + 2) >> 2 = 1
    img = np.zeros((8, 8, 4), dtype=np.uint8)
    img[0, 0], img[0, 2], img[0, 3], img[2:4, 0:2] = 1, 1, 1, 255
    levels = MM.chain(img)
    assert [l.shape[:2] for l in levels] == [(8, 8), (4, 4), (2, 2), (1, 1)] and MM.level_count(8, 8) == 4
    assert levels[1][0, 0, 0] == 0 and levels[1][0, 1, 0] == 1 and levels[1][1, 0, 0] == 255 and levels[2][0, 0, 0] == (0 + 1 + 255 + 0 + 2) >> 2 == 64 and levels[3][0, 0, 0] == 16
    assert MM.level_count(16384, 1) == 15 and MM.level_count(33, 17) == 6 and MM.level_count(64, 64) == 7
    # the one-texel checkerboard: every level below is uniformly code 128 (255 + 255 + 2) >> 2 = 128, alpha 255
    levels = MM.chain(MM.checkerboard(64))
    for l in levels[1:]:
        assert (l[..., :3] == 128).all() and (l[..., 3] == 255).all()
    # premultiplied stays premultiplied
    import image_paint_model as IM
    for l in MM.chain(IM.random_image(np.random.RandomState(1), 33, 17)):
        assert (l[..., :3] <= l[..., 3:4]).all()
    assert MM.level_scales(MM.chain(np.zeros((17, 33, 4), dtype=np.uint8)))[1] == (float(np.float32(16) / np.float32(33)), float(np.float32(8) / np.float32(17)))


def test_lod_and_the_blend_at_their_corners():
    import image_paint_model as IM
    import mip_model as MM
    image = IM.smooth_image(64)
    eye = lambda k: np.tile(np.eye(2) * k, (5, 1, 1))  # dp of an instance that maps a pixel to k path units
    spec = MM.MipSpec(image, IDENTITY, int(Filter.LinearMipmap), Spread.Repeat, Spread.Repeat, MM.chain(image))
    # rho <= 1: lod 0 — magnified and one to one
    for k in (0.0, 1e-3, 0.5, 1.0):
        assert (MM.lod_of(spec, eye(k))[0] == 0.0).all(), k
    assert np.allclose(MM.lod_of(spec, eye(2.0))[0], 1.0) and np.allclose(MM.lod_of(spec, eye(2.0 ** 2.5))[0], 2.5)
    # the clamp at L - 1 = 6, and NaN -> 0
    assert (MM.lod_of(spec, eye(64.0))[0] == 6.0).all() and (MM.lod_of(spec, eye(1e9))[0] == 6.0).all() and (MM.lod_of(spec, eye(1e30))[0] == 6.0).all()
    assert (MM.lod_of(spec, eye(np.nan))[0] == 0.0).all()
    # max of the two columns decides: 4 texels per pixel along x, 1.2 along y -> log2(4); and through the matrix, u = 3 x
    dp = np.tile(np.array([[4.0, 0.0], [0.0, 1.2]]), (3, 1, 1))
    assert np.allclose(MM.lod_of(spec, dp)[0], 2.0)
    assert np.allclose(MM.lod_of(spec._replace(matrix=(3.0, 0.0, 0.0, 0.0, 1.0, 0.0)), eye(1.0))[0], np.log2(3.0))
    # a rotation keeps rho; its sums are conditioned by kappa <= sqrt(2)
    c, s = np.cos(0.7), np.sin(0.7)
    lod, kappa = MM.lod_of(spec._replace(matrix=(c, -s, 0.0, s, c, 0.0)), eye(8.0))
    assert np.allclose(lod, 3.0) and (kappa >= 1.0).all() and (kappa < 1.5).all()
    # lod 0 and a one-level image: the base filter's value exactly
    p = np.random.RandomState(0).uniform(-90, 90, (300, 2))
    u, v = IM.uv_of(spec, p)
    base = IM.sample(MM.base_spec(spec), u, v)
    assert np.array_equal(MM.sample(spec, u, v, np.zeros(len(u)))[0], base)
    one_level = spec._replace(levels=[image])
    src, _, extra, lod = MM.mip_source(one_level, (1, 1, 1, 1), p, np.tile(np.eye(2) * 8.0, (len(p), 1, 1)), np.ones(len(p)), 208.0, 1.0 / 8.0, False)
    assert np.array_equal(src, np.clip(base, 0, 1)) and (lod == 0).all()
    # a whole lod reads one level: f = 0 at l0 = 3, and the top level's 1 x 1 texel beyond the clamp
    value, l0, l1, _ = MM.sample(spec, u, v, np.full(len(u), 3.0))
    assert np.array_equal(value, MM.sample_level(spec, 3, u, v)) and (l0 == 3).all() and (l1 == 4).all()
    value, l0, l1, _ = MM.sample(spec, u, v, np.full(len(u), 6.0))
    assert (l0 == 6).all() and (l1 == 6).all() and (value == spec.levels[6][0, 0] / 255.0).all()
    # halfway between two levels
    value = MM.sample(spec, u, v, np.full(len(u), 1.5))[0]
    assert np.allclose(value, 0.5 * (MM.sample_level(spec, 1, u, v) + MM.sample_level(spec, 2, u, v)), rtol=0, atol=1e-15)
    # equal levels give their value back exactly: a constant image, any lod, both filters, every spread
    same = np.full((17, 33, 4), 77, dtype=np.uint8)
    for f in (Filter.NearestMipmap, Filter.LinearMipmap):
        for sx, sy in IM.SPREADS:
            flat = MM.MipSpec(same, (0.7, 0.2, -1.0, -0.3, 0.9, 4.0), int(f), sx, sy, MM.chain(same))
            assert all((l == 77).all() for l in flat.levels)
            uu, vv = IM.uv_of(flat, p)
            assert (MM.sample(flat, uu, vv, np.random.RandomState(2).uniform(0, 5, len(uu)))[0] == 77.0 / 255.0).all()
    # the Jacobian of an affine instance is constant and the inverse of path -> pixels; of the identity homography the identity
    from test_ground_truth import place
    t = np.float32(place(128, 128, 50, 56, 40, rotate=0.3))
    pix = MM.G.samples(128, 128, 1).reshape(-1, 2)[::97]
    q, dp, kappa = MM.path_jacobian(pix, t, 128)
    assert np.allclose(q, MM.G.to_path(pix, t, 128, 128)) and np.allclose(dp, np.linalg.inv(MM.G.pixel_jacobian(t, 128, 128))[None]) and (kappa == 1.0).all()
    step = 1e-4
    from test_perspective_ground_truth import CASES, camera
    m = np.float32(camera(**CASES["tilted"])).reshape(16)
    pix = MM.G.pixel_centres(96)[2000:7000:131]
    q, dp, _ = MM.path_jacobian(pix, m, 96)
    for b in range(2):  # against a central difference of the model's own position
        d = np.zeros(2)
        d[b] = step
        numeric = (MM.M.to_path_h(pix + d, m, 96) - MM.M.to_path_h(pix - d, m, 96)) / (2 * step)
        assert np.allclose(dp[:, :, b], numeric, rtol=1e-5, atol=1e-9)


def _assert_caps(name, ok, extra, seams, expect):
    assert ok.mean() > 0.5, (name, ok.mean())
    assert seams <= 0.02, (name, seams)
    assert extra < 0.25 / 255.0, (name, extra * 255.0)
    assert np.isfinite(expect).all() and (expect >= 0).all() and (expect <= 1).all()


def test_the_model_alone_passes_its_caps_on_every_scene_of_the_grid():
    import image_paint_model as IM
    import mip_model as MM
    from test_gpu_blending import random_background
    background = random_background(MM.SIZE)
    for name, (shapes, transforms, colours, regions, paints), counts in MM.grid_cases():
        lods = []
        pix = MM.G.samples(MM.SIZE, MM.SIZE, 1).reshape(-1, 2)[:1]
        for t, p in zip(transforms, paints):
            dp = MM.path_jacobian(pix, t, MM.SIZE)[1]
            j = np.array([[p.matrix[0], p.matrix[1]], [p.matrix[3], p.matrix[4]]]) @ dp[0]  # texels per pixel
            assert abs(j[0, 1]) > 0.2 * abs(j[0, 0]) and abs(j[1, 0]) > 0.2 * abs(j[1, 1]), name  # turned off the frame's axes
            lods.append(float(MM.lod_of(p, dp)[0][0]))
        want = [np.log2(1.5), np.log2(3.3), 3.0, None, 2.0, 0.0]
        for i, (lod, w) in enumerate(zip(lods, want)):
            top = len(paints[i].levels) - 1.0
            assert lod == top if w is None else abs(lod - w) < 1e-3, (name, i, lod)
        for msaa in counts:
            expect, ok, extra, seams = MM.model(MM.SIZE, msaa, transforms, colours, regions, paints, IM.OVER, False, background)
            _assert_caps(f"{name} msaa {msaa}", ok, extra, seams, expect)


def test_the_model_alone_passes_its_caps_on_the_cases_with_their_own_expectation():
    import image_paint_model as IM
    import mip_model as MM
    for msaa in (1, 4):
        _, _, _, expect, sure, extra, seams, lod_range = MM.camera_case(msaa)
        assert lod_range > 1.5, lod_range
        assert sure.mean() > 0.9 and (expect[:, 3][sure] > 0).sum() > 400 and seams <= 0.02 and extra < 0.25 / 255.0, (msaa, sure.mean(), seams, extra * 255)
    _, _, src, extra = MM.stroke_case()
    assert extra < 0.25 / 255.0 and (src >= 0).all() and (src <= 1).all()
    # the checkerboard minified 8 x: the model's source is 128 / 255 x the premultiplied tint wherever the shape covers
    shapes, t, colour, region, spec = MM.checkerboard_case()
    expect, ok, extra, seams = MM.model(MM.SIZE, 1, [t], [colour], [region], [spec], IM.OVER, False, np.zeros((MM.SIZE, MM.SIZE, 4)))
    _assert_caps("checkerboard", ok, extra, seams, expect)
    pix = MM.G.samples(MM.SIZE, MM.SIZE, 1).reshape(-1, 2)
    inside = (region(MM.G.to_path(pix, t, MM.SIZE, MM.SIZE)) * MM.G.min_pixel_scale(t, MM.SIZE, MM.SIZE) > 1.0).reshape(MM.SIZE, MM.SIZE)
    tint = np.float64(colour)
    flat = (128.0 / 255.0) * np.array([tint[0] * tint[3], tint[1] * tint[3], tint[2] * tint[3], tint[3] * 255.0 / 128.0])
    assert inside.sum() > 3000 and np.abs(expect[inside] - flat).max() < 1e-12
    # ... while the one level aliases: the plain LINEAR model spans more than 64 codes there
    plain = IM.ImageSpec(spec.pixels, spec.matrix, Filter.Linear, spec.spread_x, spec.spread_y)
    aliased = IM.model(MM.SIZE, 1, [t], [colour], [region], [plain], IM.OVER, False, np.zeros((MM.SIZE, MM.SIZE, 4)))[0]
    assert (aliased[inside][:, 1].max() - aliased[inside][:, 1].min()) * 255.0 > 64.0
