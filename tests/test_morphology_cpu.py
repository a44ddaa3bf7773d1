"""crh_image_morphology without a GPU: crh_morphology_texels (host only, the rule of csrc/morphology.hpp that the kernels run) and crh_morphology_size
byte for byte against the numpy model of tests/morphology_model.py; every consequence the header states; the errors with their statuses and
texts; the Python / C++ / Rust mirrors; and one run of the rule as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, ContrastError, MorphologyOp, _ffi, morphology_size, morphology_texels
from contrast_renderer_amd import renderer as R

import blur_model as BM
import morphology_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_morphology_size", "crh_morphology_texels", "crh_image_morphology")
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17)]
RADII = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 5), (7, 3), (40, 40)]  # (40, 40) covers every axis of every size
SAME_SIZE = (MM.PAD, MM.REPEAT, MM.REFLECT)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


_pixels = {}


def pixels_of(w, h):
    """Random premultiplied texels of a size, made once and never written."""
    if (w, h) not in _pixels:
        _pixels[(w, h)] = BM.random_premultiplied(np.random.RandomState(5 * w + h), w, h)
        _pixels[(w, h)].setflags(write=False)
    return _pixels[(w, h)]


def library(lib, pixels, op, rx, ry, edge):
    h, w = pixels.shape[:2]
    ow, oh = C.c_uint32(), C.c_uint32()
    assert lib.crh_morphology_size(w, h, op, rx, ry, edge, C.byref(ow), C.byref(oh)) == _ffi.OK
    out = np.full((oh.value, ow.value, 4), 0xAB, dtype=np.uint8)
    assert lib.crh_morphology_texels(w, h, pixels.ctypes.data, op, rx, ry, edge, out.ctypes.data) == _ffi.OK
    return out


def same(got, expect, what):
    assert got.shape == expect.shape, (what, got.shape, expect.shape)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}"


def test_the_model_is_the_definition():
    """The numpy model against the definition taken one texel at a time, on sizes small enough for it."""
    for w, h in ((1, 1), (1, 7), (5, 3), (7, 4)):
        for rx, ry in ((0, 0), (1, 0), (0, 2), (2, 1), (9, 9)):
            for op in MM.OPS:
                for edge in MM.EDGES:
                    same(MM.morphology(pixels_of(w, h), op, rx, ry, edge), MM.brute(pixels_of(w, h), op, rx, ry, edge), (w, h, rx, ry, op, edge))


@pytest.mark.parametrize("edge", MM.EDGES, ids=[BlurEdge(e).name for e in MM.EDGES])
@pytest.mark.parametrize("op", MM.OPS, ids=["Erode", "Dilate"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_library_and_the_python_mirror_equal_the_model(lib, size, op, edge):
    pixels = pixels_of(*size)
    for rx, ry in RADII:
        expect = MM.morphology(pixels, op, rx, ry, edge)
        assert expect.shape[:2] == MM.size(*size, op, rx, ry, edge)[::-1]
        same(library(lib, pixels, op, rx, ry, edge), expect, (size, op, edge, rx, ry))
        same(morphology_texels(pixels, MorphologyOp(op), rx, ry, BlurEdge(edge)), expect, ("mirror", size, op, edge, rx, ry))
        assert morphology_size(size[0], size[1], MorphologyOp(op), rx, ry, BlurEdge(edge)) == MM.size(*size, op, rx, ry, edge)
    assert np.array_equal(morphology_texels(pixels, op, 2, edge=edge), MM.morphology(pixels, op, 2, 2, edge))  # radius_y=None means radius_x


def test_the_size_and_its_refusal_above_16384(lib):
    w, h = C.c_uint32(7), C.c_uint32(9)
    size = lambda *a: lib.crh_morphology_size(*a, C.byref(w), C.byref(h))  # noqa: E731
    assert size(16384, 16384, 0, 192, 192, 0) == _ffi.OK and (w.value, h.value) == (16384, 16384)  # ERODE keeps the size
    assert size(16384, 16384, 1, 192, 192, 3) == _ffi.OK and (w.value, h.value) == (16384, 16384)
    assert size(16000, 1, 1, 192, 192, 0) == _ffi.OK and (w.value, h.value) == (16384, 385)
    w.value, h.value = 7, 9
    for args in ((16001, 1, 1, 192, 0, 0), (1, 16384, 1, 0, 1, 0), (16384, 16384, 1, 1, 1, 0)):
        assert size(*args) == _ffi.ERR_UNSUPPORTED and (w.value, h.value) == (7, 9)
        assert lib.crh_last_error().decode() == "crh_morphology_size: a side of the grown result exceeds 16384"
    assert size(16384, 1, 1, 0, 192, 0) == _ffi.OK and (w.value, h.value) == (16384, 385)  # the other axis grows freely


def test_the_stated_consequences(lib):
    for w, h in SIZES:
        pixels = pixels_of(w, h)
        assert (pixels[..., :3] <= pixels[..., 3:]).all()
        for edge in MM.EDGES:
            for op in MM.OPS:
                assert np.array_equal(library(lib, pixels, op, 0, 0, edge), pixels)  # radius (0, 0) is a copy
                for rx, ry in RADII[1:]:
                    got = library(lib, pixels, op, rx, ry, edge)
                    assert (got[..., :3] <= got[..., 3:]).all(), (w, h, op, edge, rx, ry)  # rgb <= a survives
        for edge in SAME_SIZE:
            for rx, ry in RADII[1:]:
                grown, choked = library(lib, pixels, MM.DILATE, rx, ry, edge), library(lib, pixels, MM.ERODE, rx, ry, edge)
                assert (grown >= pixels).all() and (pixels >= choked).all()
                inverse = np.ascontiguousarray(255 - pixels)
                assert np.array_equal(choked, 255 - library(lib, inverse, MM.DILATE, rx, ry, edge))  # erode(x) == 255 - dilate(255 - x)
            # a window that covers a whole axis gives that row's or column's extreme
            rows = library(lib, pixels, MM.DILATE, 40, 0, edge)
            assert np.array_equal(rows, np.broadcast_to(pixels.max(axis=1, keepdims=True), pixels.shape))
            columns = library(lib, pixels, MM.ERODE, 0, 40, edge)
            assert np.array_equal(columns, np.broadcast_to(pixels.min(axis=0, keepdims=True), pixels.shape))
        # r1 then r2 equals r1 + r2 under each edge; for TRANSPARENT dilate the sizes (and so the origins) add
        for edge in MM.EDGES:
            for op in MM.OPS:
                twice = library(lib, library(lib, pixels, op, 2, 1, edge), op, 3, 4, edge)
                once = library(lib, pixels, op, 5, 5, edge)
                same(twice, once, ("r1 then r2", w, h, op, edge))
                if MM.grows(op, edge):
                    assert once.shape[:2] == (h + 10, w + 10)


def test_known_answers_by_hand(lib):
    image = np.zeros((7, 9, 4), dtype=np.uint8)
    image[3, 4] = (200, 100, 50, 255)
    got = library(lib, image, MM.DILATE, 2, 1, MM.TRANSPARENT)
    assert got.shape == (7 + 2, 9 + 4, 4)
    expect = np.zeros_like(got)
    expect[3 + 1 - 1:3 + 1 + 2, 4 + 2 - 2:4 + 2 + 3] = (200, 100, 50, 255)  # a 5 x 3 rectangle round the texel's grown position (4 + 2, 3 + 1)
    assert np.array_equal(got, expect) and int((got[..., 3] > 0).sum()) == 15
    opaque = np.full((7, 9, 4), 255, dtype=np.uint8)
    opaque[3, 4] = 0
    for edge in SAME_SIZE:
        got = library(lib, opaque, MM.ERODE, 2, 1, edge)
        expect = np.full_like(opaque, 255)
        expect[2:5, 2:7] = 0
        assert np.array_equal(got, expect), edge
    got = library(lib, opaque, MM.ERODE, 2, 1, MM.TRANSPARENT)  # the same rectangle, and the border the transparent outside eats
    expect = np.zeros_like(opaque)
    expect[1:-1, 2:-2] = 255
    expect[2:5, 2:7] = 0
    assert np.array_equal(got, expect)


def test_errors_statuses_texts_and_untouched_outputs(lib):
    pixels = pixels_of(5, 3)
    w, h = C.c_uint32(7), C.c_uint32(9)
    out = np.full((3 + 8, 5 + 8, 4), 0xAB, dtype=np.uint8)
    bad = [((5, 3, 2, 1, 1, 1), "op is above CRH_MORPHOLOGY_DILATE"), ((5, 3, 1, 1, 1, 4), "edge is above CRH_BLUR_EDGE_REFLECT"),
           ((5, 3, 1, 193, 1, 1), "a radius exceeds CRH_MAX_MORPHOLOGY_RADIUS"), ((5, 3, 0, 1, 193, 0), "a radius exceeds CRH_MAX_MORPHOLOGY_RADIUS"),
           ((5, 3, 1, 0xFFFFFFFF, 0, 0), "a radius exceeds CRH_MAX_MORPHOLOGY_RADIUS"), ((0, 3, 1, 1, 1, 1), "width and height lie in [1, 16384]"),
           ((5, 0, 1, 1, 1, 1), "width and height lie in [1, 16384]"), ((16385, 3, 1, 1, 1, 1), "width and height lie in [1, 16384]"),
           ((5, 16385, 0, 1, 1, 1), "width and height lie in [1, 16384]")]
    for (iw, ih, op, rx, ry, edge), text in bad:
        assert lib.crh_morphology_size(iw, ih, op, rx, ry, edge, C.byref(w), C.byref(h)) == _ffi.ERR_INVALID_ARGUMENT, text
        assert lib.crh_last_error().decode() == "crh_morphology_size: " + text
        assert (w.value, h.value) == (7, 9)
        assert lib.crh_morphology_texels(iw, ih, pixels.ctypes.data, op, rx, ry, edge, out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT, text
        assert lib.crh_last_error().decode() == "crh_morphology_size: " + text
        assert (out == 0xAB).all()
    assert lib.crh_morphology_size(5, 3, 1, 192, 192, 3, C.byref(w), C.byref(h)) == _ffi.OK and (w.value, h.value) == (5, 3)  # the limits themselves
    w.value, h.value = 7, 9
    for args in ((None, C.byref(h)), (C.byref(w), None)):
        assert lib.crh_morphology_size(5, 3, 1, 1, 1, 1, *args) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.crh_last_error().decode() == "crh_morphology_size: a null argument" and (w.value, h.value) == (7, 9)
    assert lib.crh_morphology_texels(5, 3, None, 1, 1, 1, 1, out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_last_error().decode() == "crh_morphology_size: a null argument"
    assert lib.crh_morphology_texels(5, 3, pixels.ctypes.data, 1, 1, 1, 1, None) == _ffi.ERR_INVALID_ARGUMENT
    assert (out == 0xAB).all()
    same_buffer = pixels.copy()
    assert lib.crh_morphology_texels(5, 3, same_buffer.ctypes.data, 1, 1, 1, 1, same_buffer.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT  # out_rgba8 == rgba8
    assert lib.crh_last_error().decode() == "crh_morphology_size: out_rgba8 is rgba8" and np.array_equal(same_buffer, pixels)
    tall = pixels_of(1, 7)
    assert lib.crh_morphology_texels(1, 16384, tall.ctypes.data, 1, 0, 1, 0, out.ctypes.data) == _ffi.ERR_UNSUPPORTED and (out == 0xAB).all()  # (refused before a byte is read)
    # the device entry point validates before it touches a device
    image = C.c_void_p(0x1234)
    assert lib.crh_image_morphology(None, 1, 1, 1, 0, C.byref(image)) == _ffi.ERR_INVALID_ARGUMENT and image.value == 0x1234
    assert lib.crh_last_error().decode() == "crh_morphology_size: a null argument"


def test_unaligned_bytes(lib):
    pixels = pixels_of(33, 17)
    expect = MM.morphology(pixels, MM.DILATE, 7, 3, MM.TRANSPARENT)
    for shift_in, shift_out in ((1, 0), (0, 3), (3, 1)):
        raw_in, raw_out = np.zeros(pixels.size + 8, dtype=np.uint8), np.full(expect.size + 8, 0xCD, dtype=np.uint8)
        raw_in[shift_in:shift_in + pixels.size] = pixels.ravel()
        assert lib.crh_morphology_texels(33, 17, raw_in.ctypes.data + shift_in, 1, 7, 3, 0, raw_out.ctypes.data + shift_out) == _ffi.OK
        assert np.array_equal(raw_out[shift_out:shift_out + expect.size].reshape(expect.shape), expect)
        assert (raw_out[:shift_out] == 0xCD).all() and (raw_out[shift_out + expect.size:] == 0xCD).all()


def test_the_python_mirror(lib):
    assert [int(MorphologyOp.Erode), int(MorphologyOp.Dilate)] == [0, 1] == list(MM.OPS)
    assert MorphologyOp(1) is MorphologyOp.Dilate and MorphologyOp["Erode"] is MorphologyOp.Erode
    with pytest.raises(ValueError):
        MorphologyOp(2)
    assert R.MAX_MORPHOLOGY_RADIUS == 192 == MM.MAX_RADIUS
    for name in ("morphology", "dilate", "erode"):
        assert callable(getattr(R.Image, name))
    for bad in (dict(op=2, radius_x=1), dict(op=1, radius_x=193), dict(op=1, radius_x=1, edge=4)):
        with pytest.raises(ContrastError) as refused:
            morphology_texels(pixels_of(5, 3), **bad)
        assert refused.value.status == _ffi.ERR_INVALID_ARGUMENT
    with pytest.raises(ContrastError):
        morphology_texels(pixels_of(5, 3)[..., :3], 1, 1)
    with pytest.raises(ContrastError) as refused:
        morphology_size(16384, 1, MorphologyOp.Dilate, 1)
    assert refused.value.status == _ffi.ERR_UNSUPPORTED
    sig = lib._crh_signatures
    assert len(sig["crh_morphology_size"][1]) == 8 and len(sig["crh_morphology_texels"][1]) == 8 and len(sig["crh_image_morphology"][1]) == 6


def test_the_library_exports_and_the_mirrors_agree_across_header_python_and_ffi_rs(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    exports = open(b.write_export_map()).read()
    for name in NAMES:
        assert f"    {name};\n" in exports
    assert any(os.path.basename(h) == "morphology.hpp" for h in b.header_deps())
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    assert re.search(r"#define CRH_MAX_MORPHOLOGY_RADIUS 192u\b", header)
    assert re.search(r"CRH_MORPHOLOGY_ERODE = 0,\s+CRH_MORPHOLOGY_DILATE = 1\s+\} crh_morphology_op;", header)
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    assert committed == fresh
    for text in ("pub fn crh_morphology_size(width: u32, height: u32, op: u32, radius_x: u32, radius_y: u32, edge: u32, out_width: *mut u32, out_height: *mut u32) -> crh_status;",
                 "pub fn crh_morphology_texels(width: u32, height: u32, rgba8: *const c_void, op: u32, radius_x: u32, radius_y: u32, edge: u32, out_rgba8: *mut c_void) -> crh_status;",
                 "pub fn crh_image_morphology(src: *const crh_image, op: u32, radius_x: u32, radius_y: u32, edge: u32, out: *mut *mut crh_image) -> crh_status;",
                 "pub const CRH_MAX_MORPHOLOGY_RADIUS: usize = 192;", "pub const CRH_MORPHOLOGY_ERODE: u32 = 0;", "pub const CRH_MORPHOLOGY_DILATE: u32 = 1;"):
        assert text in committed, text
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub enum MorphologyOp {", "    Erode = 0,", "    Dilate = 1,",
                 "pub fn morphology_size(width: u32, height: u32, op: MorphologyOp, radius_x: u32, radius_y: u32, edge: BlurEdge) -> Result<(u32, u32), Error>",
                 "pub fn morphology_texels(width: u32, height: u32, texels: &[u8], op: MorphologyOp, radius_x: u32, radius_y: u32, edge: BlurEdge) -> Result<(u32, u32, Vec<u8>), Error>",
                 "pub fn morphology(&self, op: MorphologyOp, radius_x: u32, radius_y: u32, edge: BlurEdge) -> Result<Image, Error>",
                 "pub fn dilate(&self, radius_x: u32, radius_y: u32, edge: BlurEdge) -> Result<Image, Error>",
                 "pub fn erode(&self, radius_x: u32, radius_y: u32, edge: BlurEdge) -> Result<Image, Error>"):
        assert text in shim, text
    mirror = open(os.path.join(ROOT, "include", "contrast_renderer.hpp")).read()
    for text in ("enum class MorphologyOp : uint32_t { Erode = CRH_MORPHOLOGY_ERODE, Dilate = CRH_MORPHOLOGY_DILATE };", "Image morphology(MorphologyOp op, uint32_t radius_x, uint32_t radius_y,",
                 "Image dilate(uint32_t radius_x, uint32_t radius_y,", "Image erode(uint32_t radius_x, uint32_t radius_y,"):
        assert text in mirror, text


def test_the_cpp_mirror_of_morphology_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "morphology_harness.cpp"),
               "-o", os.path.join(tmp, "morphology_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """A stand-alone program (its own main, no library, nothing loaded into python) around csrc/morphology.hpp, the rule that
    crh_morphology_texels runs: compiled as host code with the two sanitizers (the flag goes to the host compilation alone) and run once."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        binary = os.path.join(tmp, "morphology_sanitize")
        # -x c++ and -Xarch_host: plain host C++, the sanitizers on the host alone (no device pass; clang links the sanitizers' runtime statically, so the program needs nothing preloaded)
        cmd = [hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
               "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), "-I", os.path.join(ROOT, "contrast_renderer_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "morphology_sanitize.cpp"), "-o", binary]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert done.stdout.strip().endswith("168660 texels, 0 failures")
