"""crh_image_blur without a GPU: crh_blur_taps (host only) against the tap rule and its float64 ideal, its errors, the integer model of
tests/blur_model.py alone — a known answer by hand, the constant image, premultiplication — and the Python / C++ / Rust mirrors."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, ContrastError, _ffi, blur_taps
from contrast_renderer_amd import renderer as R

import blur_model as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = [0.0, 0.01, 0.3, 1.0 / 3.0, 0.5, 1.0, 2.5, 7.0, 31.9, 64.0]
NAMES = ("crh_blur_taps", "crh_image_blur")
# Sigmas whose library taps need not equal the model's: where the C library's exp and Python's differ in the last place and a rounding of
# w[k] / S * 65536 + 0.5 flips. None does here — both are the platform's libm — so the equality is asserted for every sigma of the list.
EXP_DIFFERS = ()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def library_taps(lib, sigma):
    taps = (C.c_uint32 * 193)()
    radius = C.c_uint32(0xFFFF)
    assert lib.crh_blur_taps(sigma, taps, 193, C.byref(radius)) == _ffi.OK
    return [int(v) for v in taps[:radius.value + 1]], int(radius.value)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_the_taps_sum_to_65536_and_stay_within_one_and_a_half_of_the_ideal(lib, sigma):
    q, radius = library_taps(lib, sigma)
    s = float(np.float32(sigma))
    assert radius == math.ceil(3.0 * s) == len(q) - 1 and radius <= 192
    assert q[0] + 2 * sum(q[1:]) == 65536
    assert min(q) >= 0
    ideal, ideal_radius = BM.ideal_taps(sigma)
    assert ideal_radius == radius
    worst = max(abs(a - b) for a, b in zip(q, ideal))
    assert worst <= 1.5, worst
    if sigma not in EXP_DIFFERS:
        assert (q, radius) == BM.taps(sigma)
    mirrored, mirrored_radius = blur_taps(sigma)
    assert mirrored.dtype == np.uint32 and mirrored.tolist() == q and mirrored_radius == radius
    if sigma == 0.0:
        assert q == [65536]


def test_the_tap_rule_over_many_sigmas_in_the_model():
    """What the rule promises, on the model: |d| / 2 <= R (taps() asserts it), non-negative, monotone up to one unit, within 1.5 of the ideal."""
    for sigma in np.linspace(0.004, 64.0, 700):
        q, radius = BM.taps(sigma)
        ideal, _ = BM.ideal_taps(sigma)
        assert q[0] + 2 * sum(q[1:]) == 65536 and min(q) >= 0
        assert max(abs(a - b) for a, b in zip(q, ideal)) <= 1.5
        assert all(q[k + 1] <= q[k] + 1 for k in range(radius))


def test_the_errors_of_the_taps(lib):
    taps = (C.c_uint32 * 193)(*([7] * 193))
    radius = C.c_uint32(99)
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.crh_blur_taps(bad, taps, 193, C.byref(radius)) == _ffi.ERR_NON_FINITE
    assert lib.crh_blur_taps(-1.0, taps, 193, C.byref(radius)) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode() == "crh_blur_taps: sigma is negative"
    assert lib.crh_blur_taps(64.5, taps, 193, C.byref(radius)) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode() == "crh_blur_taps: sigma exceeds CRH_MAX_BLUR_SIGMA"
    assert lib.crh_blur_taps(2.0, taps, 6, C.byref(radius)) == _ffi.ERR_INVALID_ARGUMENT  # R = 6 wants 7 words
    assert lib.crh_last_error().decode() == "crh_blur_taps: capacity is below radius + 1"
    assert radius.value == 99 and list(taps) == [7] * 193  # a refused call writes nothing
    assert lib.crh_blur_taps(2.0, taps, 7, C.byref(radius)) == _ffi.OK and radius.value == 6 and taps[7] == 7
    # the NULL query: the radius alone, whatever the capacity; and no radius wanted
    radius = C.c_uint32(99)
    assert lib.crh_blur_taps(64.0, None, 0, C.byref(radius)) == _ffi.OK and radius.value == 192
    assert lib.crh_blur_taps(2.0, taps, 193, None) == _ffi.OK
    for bad in (float("nan"), -1.0, 64.5):
        with pytest.raises(ContrastError):
            blur_taps(bad)


def test_the_blur_refuses_null_arguments_and_bad_sigmas_without_a_device(lib):
    out = C.c_void_p(0x1234)
    assert lib.crh_image_blur(None, 1.0, 1.0, 0, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_blur(None, 1.0, 1.0, 0, None) == _ffi.ERR_INVALID_ARGUMENT


def test_a_known_answer_by_hand_one_white_texel():
    white = np.full((1, 1, 4), 255, dtype=np.uint8)
    for sigma_x, sigma_y in ((2.0, 2.0), (0.5, 1.0), (0.0, 3.0)):
        (qx, rx), (qy, ry) = BM.taps(sigma_x), BM.taps(sigma_y)
        got = BM.blur(white, qx, qy, BM.TRANSPARENT)
        assert got.shape == (1 + 2 * ry, 1 + 2 * rx, 4)
        for j in range(got.shape[0]):
            for i in range(got.shape[1]):
                expect = (qy[abs(j - ry)] * ((qx[abs(i - rx)] * 255 + 128) >> 8) + (1 << 23)) >> 24
                assert (got[j, i] == expect).all(), (i, j, got[j, i], expect)
        assert got[ry, rx, 0] == got.max() > 0
    assert BM.blur_sigma(white, 2.0, 2.0, BM.TRANSPARENT).shape == (13, 13, 4)


def test_the_wrap_helper_many_periods_out():
    i = np.arange(-400, 400)
    assert BM.wrap(i, 1, BM.PAD).tolist() == BM.wrap(i, 1, BM.REPEAT).tolist() == BM.wrap(i, 1, BM.REFLECT).tolist() == [0] * 800
    assert BM.wrap([-1, 0, 2, 3, 4, 5, 6, -4], 3, BM.REFLECT).tolist() == [0, 0, 2, 2, 1, 0, 0, 2]
    assert BM.wrap([-1, 3, -7, 7], 3, BM.REPEAT).tolist() == [2, 0, 2, 1]
    assert BM.wrap([-9, 1, 9], 3, BM.PAD).tolist() == [0, 1, 2]


def test_sigma_zero_is_a_copy_and_a_constant_image_is_a_fixed_point():
    rng = np.random.RandomState(4)
    pixels = BM.random_premultiplied(rng, 9, 5)
    for edge in BM.EDGES:
        assert np.array_equal(BM.blur_sigma(pixels, 0.0, 0.0, edge), pixels)
    for code in (1, 77, 254, 255):
        flat = np.full((5, 7, 4), code, dtype=np.uint8)
        for edge in (BM.PAD, BM.REPEAT, BM.REFLECT):
            for sigmas in ((0.3, 0.0), (1.0, 1.0), (2.5, 7.0), (64.0, 64.0)):
                assert (BM.blur_sigma(flat, *sigmas, edge) == code).all(), (code, edge, sigmas)
    # under TRANSPARENT: exactly the texels whose window lies wholly inside the source
    flat = np.full((40, 30, 4), 200, dtype=np.uint8)
    got = BM.blur_sigma(flat, 1.0, 2.0, BM.TRANSPARENT)  # R = (3, 6): the result is 36 x 52
    assert got.shape == (52, 36, 4) and (got[12:40, 6:30] == 200).all() and got[0, 0, 3] < 200


def test_premultiplied_stays_premultiplied():
    rng = np.random.RandomState(9)
    pixels = BM.random_premultiplied(rng, 33, 17)
    assert (pixels[..., :3] <= pixels[..., 3:4]).all()
    for edge in BM.EDGES:
        for sigmas in ((0.3, 0.5), (2.5, 7.0), (64.0, 1.0)):
            got = BM.blur_sigma(pixels, *sigmas, edge)
            assert (got[..., :3] <= got[..., 3:4]).all(), (edge, sigmas)


def test_the_two_forms_of_a_pass_agree():
    """The model folds the wrap into a matrix for short axes and walks shifted slices for long ones: the same integers."""
    rng = np.random.RandomState(2)
    values = rng.randint(0, 256, (23, 3, 4)).astype(np.uint64)
    for edge in BM.EDGES:
        for sigma in (0.0, 1.0, 20.0):
            q = BM.taps(sigma)[0]
            assert np.array_equal(np.matmul(BM._weights(q, 23, edge), values.reshape(23, -1)).reshape(-1, 3, 4), BM._slices(values, q, edge)), (edge, sigma)


def test_the_library_exports_and_a_fresh_ffi_rs_declares_the_new_symbols(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    assert "image_filter.hip" in b.SOURCES
    exports = open(b.write_export_map()).read()
    for name in NAMES:
        assert f"    {name};\n" in exports
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    for ffi in (committed, fresh):
        assert "pub const CRH_BLUR_EDGE_TRANSPARENT: u32 = 0;" in ffi and "pub const CRH_BLUR_EDGE_REFLECT: u32 = 3;" in ffi and "pub const CRH_MAX_BLUR_RADIUS: usize = 192;" in ffi
        assert re.search(r"pub fn crh_blur_taps\(sigma: f32, taps: \*mut u32, capacity: u32, radius: \*mut u32\) -> crh_status;", ffi)
        assert re.search(r"pub fn crh_image_blur\(src: \*const crh_image, sigma_x: f32, sigma_y: f32, edge: u32, out: \*mut \*mut crh_image\) -> crh_status;", ffi)
    assert committed == fresh
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub enum BlurEdge {", "pub fn blur_taps(sigma: f32) -> Result<Vec<u32>, Error>",
                 "pub fn blur(&self, sigma_x: f32, sigma_y: f32, edge: BlurEdge) -> Result<Image, Error>", "pub fn origin(&self) -> (u32, u32)"):
        assert text in shim, text


def test_the_cpp_mirror_of_blur_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "blur_harness.cpp"),
               "-o", os.path.join(tmp, "blur_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


def test_the_python_mirror_round_trips_the_edge(lib):
    assert [int(e) for e in (BlurEdge.Transparent, BlurEdge.Pad, BlurEdge.Repeat, BlurEdge.Reflect)] == [0, 1, 2, 3] == list(BM.EDGES)
    assert BlurEdge(2) is BlurEdge.Repeat and BlurEdge["Reflect"] is BlurEdge.Reflect
    with pytest.raises(ValueError):
        BlurEdge(4)
    assert R.MAX_BLUR_SIGMA == 64.0 and R.MAX_BLUR_RADIUS == 192
    assert hasattr(R.Image, "blur") and R.Image.origin == (0, 0)
    sig = lib._crh_signatures
    assert sig["crh_image_blur"][1][3] is C.c_uint32 and sig["crh_blur_taps"][1][0] is C.c_float
