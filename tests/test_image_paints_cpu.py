"""Image paints without a GPU: crh_image_paint_validate (host only), the Python / C++ / Rust mirrors of the new ABI, the remap of a mixed paint list,
and the float64 model of tests/test_gpu_image_paints.py run alone on the scenes those tests draw."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, Filter, ImagePaint, Paint, Spread, _ffi
from contrast_renderer_amd import renderer as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def raw(image=0x1000, filter=1, spread_x=0, spread_y=0, m=IDENTITY):
    c = _ffi.ImagePaintC()
    c.image, c.filter, c.spread_x, c.spread_y = image, filter, spread_x, spread_y  # (the handle is only compared with null)
    for i in range(6):
        c.m[i] = m[i]
    return c


INVALID = {"null image": raw(image=None), "unknown filter": raw(filter=2), "unknown spread_x": raw(spread_x=3), "unknown spread_y": raw(spread_y=7)}
NON_FINITE = {"nan": raw(m=(1.0, float("nan"), 0.0, 0.0, 1.0, 0.0)), "inf": raw(m=(1.0, 0.0, 0.0, 0.0, 1.0, float("inf")))}
VALID = {"nearest": raw(filter=0), "linear reflect / repeat": raw(spread_x=2, spread_y=1), "a singular map": raw(m=(0.0,) * 6)}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_validate_refuses_with_invalid_argument_and_a_text(lib, name):
    assert lib.crh_image_paint_validate(C.byref(INVALID[name])) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode().startswith("crh_image_paint: ")


@pytest.mark.parametrize("name", sorted(NON_FINITE))
def test_validate_refuses_a_non_finite_matrix(lib, name):
    assert lib.crh_image_paint_validate(C.byref(NON_FINITE[name])) == _ffi.ERR_NON_FINITE


@pytest.mark.parametrize("name", sorted(VALID))
def test_validate_accepts(lib, name):
    assert lib.crh_image_paint_validate(C.byref(VALID[name])) == _ffi.OK
    assert lib.crh_image_paint_validate(None) == _ffi.ERR_INVALID_ARGUMENT


def test_an_image_paint_is_not_a_paint_kind(lib):
    from test_paints_cpu import raw as gradient
    assert lib.crh_paint_validate(C.byref(gradient(kind=3))) == _ffi.ERR_INVALID_ARGUMENT
    assert C.sizeof(_ffi.PaintC) == 4 * (2 + 4 + 1 + 8 * 5) and C.sizeof(_ffi.ImagePaintC) == 8 + 4 * 3 + 4 * 6 + 4  # (padded to the pointer's alignment)


def test_the_library_exports_and_a_fresh_ffi_rs_declares_the_new_symbols(lib):
    names = ("crh_image_create", "crh_image_create_from_frame", "crh_image_size", "crh_image_destroy", "crh_image_paint_validate", "crh_scene_set_paints_with_images")
    for name in names:
        assert getattr(lib, name) is not None
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    for ffi in (committed, fresh):
        for name in names:
            assert re.search(r"pub fn %s\(" % name, ffi), name
        assert "pub struct crh_image_paint {" in ffi and "pub m: [f32; 6]," in ffi and "pub image: *const crh_image," in ffi
        assert "pub const CRH_FILTER_LINEAR: u32 = 1;" in ffi and "pub struct crh_image {" in ffi
        assert re.search(r"pub fn crh_scene_set_paints_with_images\(scene: \*mut crh_scene, paints: \*const crh_paint, n_paints: u32, image_paints: \*const crh_image_paint, "
                         r"n_image_paints: u32, instance_paint: \*const i32, n_instances: u32\) -> crh_status;", ffi)
    assert committed == fresh
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    assert "pub fn set_paints_with_images(&self, paints: &[Paint], image_paints: &[ImagePaint], instance_paint: &[i32]) -> Result<(), Error>" in shim
    assert "pub fn from_frame(frame: &Frame) -> Result<Image, Error>" in shim


def test_the_cpp_mirror_of_image_paints_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "image_paints_harness.cpp"),
               "-o", os.path.join(tmp, "image_paints_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


class _Handle:  # stands for an Image where no device is at hand: ImagePaint only carries it
    def __init__(self, handle, width=8, height=4):
        self.handle, self.width, self.height = handle, width, height


def test_python_image_paint_round_trips_and_is_hashable(lib):
    image = _Handle(0x2000)
    paint = ImagePaint(image, [0.5, -1.0, 2.0, 3.0, 0.25, -4.0], Filter.Nearest, Spread.Repeat, Spread.Reflect)
    c = paint.to_c()
    assert (c.image, c.filter, c.spread_x, c.spread_y, tuple(c.m)) == (0x2000, 0, 1, 2, (0.5, -1.0, 2.0, 3.0, 0.25, -4.0))
    paint.validate()
    default = ImagePaint(image, IDENTITY)
    assert (default.filter, default.spread_x, default.spread_y) == (Filter.Linear, Spread.Pad, Spread.Pad)
    assert hash(default) == hash(ImagePaint(image, IDENTITY)) and default == ImagePaint(image, list(IDENTITY)) and default != paint and len({default, paint, ImagePaint(image, IDENTITY)}) == 2
    with pytest.raises(Exception):
        default.filter = Filter.Nearest  # frozen
    with pytest.raises(ContrastError):
        ImagePaint(image, IDENTITY, filter=5).validate()
    with pytest.raises(ContrastError):
        ImagePaint(_Handle(None), IDENTITY).validate()  # a destroyed image
    with pytest.raises(ContrastError):
        ImagePaint(image, (1.0, 0.0, 0.0))
    # fit: the path rectangle onto the whole image, path y up = the image's row 0 at the upper edge
    m = ImagePaint.fit(image, (-1.0, -0.5), (3.0, 1.5)).matrix
    at = lambda x, y: (m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5])
    assert at(-1.0, 1.5) == (0.0, 0.0) and at(3.0, -0.5) == (8.0, 4.0) and at(1.0, 0.5) == (4.0, 2.0)


def test_a_mixed_list_puts_gradients_first_and_remaps_the_indices():
    red = (1.0, 0.0, 0.0, 1.0)
    g0, g1 = Paint.linear((0, 0), (1, 0), [(0.0, red)]), Paint.radial((0, 0), 1.0, [(0.5, red)])
    i0, i1 = ImagePaint(_Handle(1), IDENTITY), ImagePaint(_Handle(2), IDENTITY, Filter.Nearest)
    gradients, images, which = R.split_paints([i0, g0, i1, g1], [0, 1, 2, 3, -1, 2, 0])
    assert gradients == [g0, g1] and images == [i0, i1]
    assert which == [2, 0, 3, 1, -1, 3, 2]
    assert R.split_paints([g0, g1], [1, 0, -1]) == ([g0, g1], [], [1, 0, -1])
    assert R.split_paints([i0], [0, 5, -2])[2] == [0, 5, -2]  # what the C side refuses stays what it was
    # RenderPass numbers a pass's paints in the order they arrive, gradients and image paints mixed
    p = R.RenderPass.__new__(R.RenderPass)
    p.transforms, p.colors, p.paints, p.instance_paint = [], [], [], []
    for paint in (i0, None, g0, i0, i1):
        p.push_instance(np.eye(4), red, paint=paint)
    assert p.paints == [i0, g0, i1] and p.instance_paint == [0, -1, 1, 0, 2]
    assert R.split_paints(p.paints, p.instance_paint)[2] == [1, -1, 0, 1, 2]


# ---------------------------------------------------------------- the float64 model alone, on every scene the GPU tests draw

def test_the_model_follows_the_contract_at_its_corners():
    import image_paint_model as IM
    assert np.array_equal(IM.wrap(np.arange(-7, 8), 3, Spread.Pad), [0] * 8 + [1] + [2] * 6)
    assert np.array_equal(IM.wrap(np.arange(-7, 8), 3, Spread.Repeat), [2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1])
    assert np.array_equal(IM.wrap(np.arange(-7, 8), 3, Spread.Reflect), [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1])
    pixels = np.uint8([[[0, 0, 0, 255], [255, 0, 0, 255], [51, 0, 0, 255]]])  # 3 x 1
    spec = lambda f, s: IM.ImageSpec(pixels, IDENTITY, f, s, Spread.Pad)
    red = lambda f, s, u: IM.sample(spec(f, s), np.float64(u), np.zeros(len(u)))[:, 0]
    assert np.array_equal(red(Filter.Nearest, Spread.Pad, [-0.5, 0.0, 0.99, 1.0, 2.5, 9.0]), [0.0, 0.0, 0.0, 1.0, 0.2, 0.2])
    assert np.array_equal(red(Filter.Nearest, Spread.Repeat, [-0.5, -1.5, 3.5]), [0.2, 1.0, 0.0])  # floor, not truncation
    assert np.allclose(red(Filter.Linear, Spread.Pad, [0.5, 1.0, 1.5, 2.0, 0.0, 3.0]), [0.0, 0.5, 1.0, 0.6, 0.0, 0.2])  # texel centres give the texel
    assert np.allclose(red(Filter.Linear, Spread.Repeat, [0.0, 3.0]), [0.1, 0.1])  # halfway between the last and the first texel
    same = IM.ImageSpec(np.full((3, 5, 4), 77, dtype=np.uint8), (0.7, 0.2, -1.0, -0.3, 0.9, 4.0), Filter.Linear, Spread.Reflect, Spread.Repeat)
    p = np.random.RandomState(0).uniform(-9, 9, (200, 2))
    assert (IM.sample(same, *IM.uv_of(same, p)) == 77.0 / 255.0).all() and IM.neighbour_difference(same) == 0.0
    assert IM.neighbour_difference(spec(Filter.Linear, Spread.Pad)) == 1.0 and IM.neighbour_difference(IM.ImageSpec(pixels[:, :2], IDENTITY, 1, Spread.Repeat, 0)) == 1.0
    src, _ = IM.image_source(spec(Filter.Nearest, Spread.Pad), (0.5, 1.0, 1.0, 0.5), np.float64([[1.5, 0.0]]), 0.0)
    assert np.array_equal(src, [[0.25, 0.0, 0.0, 0.5]])  # value.rgb * (tint.rgb * tint.a), value.a * tint.a


def _assert_caps(name, ok, extra, seams, expect):
    assert ok.mean() > 0.5, (name, ok.mean())
    assert seams <= 0.02, (name, seams)
    assert extra < 0.25 / 255.0, (name, extra * 255.0)
    assert np.isfinite(expect).all() and (expect >= 0).all() and (expect <= 1).all()


def test_the_model_alone_passes_its_caps_on_every_scene_of_the_grid():
    import image_paint_model as IM
    from test_gpu_blending import random_background
    background = random_background(IM.SIZE)
    for name, (shapes, transforms, colours, regions, paints), counts in IM.grid_cases():
        specs = [(p, t) for p, t in zip(paints, transforms) if isinstance(p, IM.ImageSpec)]
        if name != "minified":
            assert all(IM.texel_px(p, t, IM.SIZE) >= 4.0 for p, t in specs), name
            assert all(abs(p.matrix[1]) > 0.2 * abs(p.matrix[0]) for p, _ in specs), name  # rotated off the axes
        for msaa in counts:
            expect, ok, extra, seams = IM.model(IM.SIZE, msaa, transforms, colours, regions, paints, IM.OVER, False, background)
            _assert_caps(f"{name} msaa {msaa}", ok, extra, seams, expect)
    # the placements reach below 0 and beyond the size on both axes
    _, transforms, _, regions, paints = IM.scene(Filter.Nearest, Spread.Pad, Spread.Pad)
    pix = IM.G.samples(IM.SIZE, IM.SIZE, 1).reshape(-1, 2)
    low, high = np.zeros(2, dtype=bool), np.zeros(2, dtype=bool)
    for t, region, p in zip(transforms, regions, paints):
        if isinstance(p, IM.ImageSpec):
            q = IM.G.to_path(pix, t, IM.SIZE, IM.SIZE)
            u, v = (a[region(q) > 0] for a in IM.uv_of(p, q))
            low |= [u.min() < -1.0, v.min() < -1.0]
            high |= [u.max() > p.pixels.shape[1] + 1.0, v.max() > p.pixels.shape[0] + 1.0]
    assert low.all() and high.all()


def test_the_model_alone_passes_its_caps_on_the_cases_with_their_own_expectation():
    import image_paint_model as IM
    _, expect, ok, extra, seams = IM.recorded_case()
    _assert_caps("recorded", ok, extra, seams, expect)
    for msaa, f in IM.CAMERA_CASES:
        _, _, _, expect, sure, extra, seams = IM.camera_case(msaa, f)
        assert sure.mean() > 0.9 and (expect[:, 3][sure] > 0).sum() > 400 and seams <= 0.02 and extra < 0.25 / 255.0, (msaa, f, sure.mean(), seams, extra * 255)
    for f in (Filter.Nearest, Filter.Linear):
        _, _, src, seam, extra = IM.stroke_case(f)
        assert seam.mean() <= 0.02 and extra < 0.25 / 255.0 and (src >= 0).all() and (src <= 1).all()


# ---------------------------------------------------------------- the coordinate rule at its ends (tests/test_gpu_image_paints.py, test_gpu_mipmaps.py)

def test_the_extreme_matrices_have_exact_and_stable_expectations():
    """What the GPU tests compare byte for byte must not hang on a rounding: every product-sum of the expectation is exact in float64 (fma32
    asserts it) and rounded to f32 once; every index and fraction stays what it is when X and Y move by a relative 2^-20 in any of the four
    directions; every fraction is 0, so a LINEAR value is one texel's codes; and the cases reach what they are named after."""
    import image_paint_model as IM
    names = [n for n, _ in IM.extreme_matrices()]
    assert len(names) == len(set(names)) == 21
    e = 2.0 ** -20
    size = IM.EXTREME_SIZE
    Y, X = np.meshgrid(np.arange(size) + 0.5, np.arange(size) + 0.5, indexing="ij")
    reached = {}
    for name, matrix in IM.extreme_matrices():
        u, v = IM.extreme_uv(matrix, X, Y)
        raw_u = IM.fma32(Y, np.float32(matrix[1]), IM.fma32(X, np.float32(matrix[0]), np.float32(matrix[2])))
        reached[name] = (float(np.abs(u).max()), float(np.abs(v).max()), bool(np.isinf(raw_u).any()))
        for filter in (Filter.Nearest, Filter.Linear):
            for spreads in IM.EXTREME_SPREADS:
                taps = IM.extreme_taps(matrix, filter, *spreads)
                assert not taps[4].any() and not taps[5].any(), (name, filter)
                for sx in (1.0 - e, 1.0 + e):
                    for sy in (1.0 - e, 1.0 + e):
                        moved = IM.extreme_taps(matrix, filter, *spreads, scale=(sx, sy), exact=False)
                        assert all(np.array_equal(a, b) for a, b in zip(taps, moved)), (name, filter, spreads, sx, sy)
    assert reached["u:2^23-32"][0] < 2.0 ** 23 and reached["u:2^23-32"][0] > 2.0 ** 23 - 33
    for name in ("2^24", "-2^24", "2^24+64", "-(2^24+64)", "3e38", "-3e38", "overflow", "inf-and-back"):
        assert reached["u:" + name][0] == 2.0 ** 24 and reached["v:" + name][1] == 2.0 ** 24, name
    assert reached["u:overflow"][2] and reached["u:inf-and-back"][2] and not reached["u:2^24+64"][2]
    # 2^23 and 2^24 differ modulo the height and twice the height: a clamp at another power of two shows
    assert (2 ** 23) % 5 != (2 ** 24) % 5 and (2 ** 23) % 10 != (2 ** 24) % 10
    # ... and the expectation shows more than one texel per case: the wrap is exercised, not a constant
    pixels = IM.random_image(np.random.RandomState(5), *IM.EXTREME_IMAGE)
    for name, matrix in IM.extreme_matrices():
        expect = IM.extreme_expectation(pixels, matrix, Filter.Linear, Spread.Repeat, Spread.Reflect)
        assert len(np.unique(expect.reshape(-1, 4), axis=0)) >= 5, name
