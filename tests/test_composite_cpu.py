"""crh_image_composite without a GPU: crh_composite_texels (host only, the rule of csrc/composite.hpp that the kernel runs) byte for byte against
the integer model of tests/composite_model.py; that model within half a code of the W3C definitions in float64; the alpha exhaustively; the
consequences the header states; crh_composite_validate's errors; and the Python / C++ / Rust mirrors."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import BlendMode, CompositeOp, ContrastError, _ffi, composite_texels
from contrast_renderer_amd import renderer as R

import composite_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_composite_validate", "crh_composite_texels", "crh_image_composite", "crh_frame_load_image")
OPACITY_CODES = (255, 128, 1, 0)
N_RANDOM = 1 << 20


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


@pytest.fixture(scope="module")
def inputs():
    """(name, source, backdrop): all valid pairs over the edge codes, one code for the three colours, and 2^20 random pairs of which every
    fifth is not premultiplied. Made once, never written."""
    made = [("grid",) + CM.grid_pairs(), ("random",) + CM.random_pairs(N_RANDOM, seed=11)]
    for _, s, b in made:
        s.setflags(write=False), b.setflags(write=False)
    assert made[0][1].shape == (66 * 66, 4) and made[1][1].shape == (N_RANDOM, 4)
    loose = (made[1][1][:, :3] > made[1][1][:, 3:4]).any(axis=1)
    assert loose.any() and not loose[np.arange(N_RANDOM) % 5 != 0].any()
    return made


def library_texels(lib, source, backdrop, op, mode, opacity):
    how = _ffi.CompositeC(op, mode, opacity, 12345, -6789)  # (x, y are ignored)
    out = np.full(source.shape, 0xAB, dtype=np.uint8)
    assert lib.crh_composite_texels(C.byref(how), source.ctypes.data, backdrop.ctypes.data, len(source), out.ctypes.data) == _ffi.OK
    return out


@pytest.mark.parametrize("o", OPACITY_CODES)
def test_the_library_equals_the_integer_model_for_every_operator_and_mode(lib, inputs, o):
    opacity = float(np.float32(o / 255.0))
    assert CM.opacity_code(opacity) == o
    for name, source, backdrop in inputs:
        s, b = CM.fade(CM.load(source), o), CM.load(backdrop)
        for mode in range(len(CM.MODES)):
            x = CM.blend(s, b, mode)
            for op in range(len(CM.OPS)):
                expect = CM.finish(s, b, x, op)
                got = library_texels(lib, source, backdrop, op, mode, opacity)
                if not np.array_equal(got, expect):
                    k = int(np.argwhere((got != expect).any(axis=1))[0][0])
                    pytest.fail(f"{name} {CM.OPS[op]} {CM.MODES[mode]} o={o}: pair {k} source {source[k]} backdrop {backdrop[k]} -> {got[k]}, the model {expect[k]}")


def test_the_staged_model_is_the_plain_one():
    source, backdrop = CM.grid_pairs()
    for op, mode, o in ((CM.SRC_ATOP, CM.HARD_LIGHT, 128), (CM.XOR, CM.DIFFERENCE, 255), (CM.PLUS, CM.OVERLAY, 1)):
        s, b = CM.fade(CM.load(source), o), CM.load(backdrop)
        assert np.array_equal(CM.texels(source, backdrop, op, mode, o), CM.finish(s, b, CM.blend(s, b, mode), op))


@pytest.mark.parametrize("o", OPACITY_CODES)
def test_the_integer_model_is_within_half_a_code_of_the_w3c_formula(inputs, o):
    """One rounding of the exact rational value: |integer - real| <= 0.5, and 1e-9 for the float64 evaluation of the real value."""
    worst = 0.0
    for name, source, backdrop in inputs:
        source, backdrop = source[:1 << 16], backdrop[:1 << 16]
        s, b = CM.fade(CM.load(source), o), CM.load(backdrop)
        for mode in range(len(CM.MODES)):
            x = CM.blend(s, b, mode)
            assert (x <= 65025).all()
            for op in range(len(CM.OPS)):
                got = CM.finish(s, b, x, op).astype(np.float64)
                error = np.abs(got - CM.w3c(s, b, op, mode))
                assert error.max() <= 0.5 + 1e-9, (name, CM.OPS[op], CM.MODES[mode], o, error.max(), source[int(error.max(axis=1).argmax())], backdrop[int(error.max(axis=1).argmax())])
                worst = max(worst, float(error.max()))
    print(f"o={o}: worst error {worst:.6f} code")


def test_the_alpha_exhaustively(lib):
    """ao over all 65 536 (sa, ba) for every operator: the library, the model and the rounded real value"""
    sa, ba = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    source, backdrop = np.zeros((65536, 4), dtype=np.uint8), np.zeros((65536, 4), dtype=np.uint8)
    source[:, 3], backdrop[:, 3] = sa.ravel(), ba.ravel()
    source[:, :3], backdrop[:, :3] = source[:, 3:4] // 2, backdrop[:, 3:4]
    for op in range(len(CM.OPS)):
        (a0, a1), (b0, b1) = CM.FACTORS[op]
        a, b = source[:, 3].astype(np.int64), backdrop[:, 3].astype(np.int64)
        exact = np.minimum(255, ((a0 + a1 * b) * a + (b0 + b1 * a) * b + 127) // 255)  # in Python-wide integers
        for mode in (CM.NORMAL, CM.HARD_LIGHT, CM.DIFFERENCE):  # the mode does not enter ao
            got = library_texels(lib, source, backdrop, op, mode, 1.0)
            assert np.array_equal(got[:, 3], exact), (CM.OPS[op], CM.MODES[mode])
            assert np.array_equal(CM.texels(source, backdrop, op, mode, 255)[:, 3], exact)
            assert (got[:, :3] <= got[:, 3:4]).all()


def test_the_stated_consequences(lib, inputs):
    for name, source, backdrop in inputs:
        source, backdrop = source[:1 << 17], backdrop[:1 << 17]
        s255, b = CM.load(source), CM.load(backdrop)
        for o in OPACITY_CODES:
            opacity = float(np.float32(o / 255.0))
            for op in range(len(CM.OPS)):
                for mode in range(len(CM.MODES)):
                    got = library_texels(lib, source, backdrop, op, mode, opacity)
                    assert (got[:, :3] <= got[:, 3:4]).all(), ("co <= ao", name, CM.OPS[op], CM.MODES[mode], o)  # premultiplied stays premultiplied
                    if op == CM.DST:
                        assert np.array_equal(got, b.astype(np.uint8)), ("DST is the (loaded) backdrop", CM.MODES[mode], o)
                    if op == CM.CLEAR:
                        assert not got.any()
                    if op == CM.COPY and mode == CM.NORMAL:
                        assert np.array_equal(got, CM.fade(s255, o).astype(np.uint8)), ("COPY is the placed source", o)
        # NORMAL + SRC_OVER at o = 255: sc + round(bc (255 - sa) / 255), the over of every 8-bit compositor
        got = library_texels(lib, source, backdrop, CM.SRC_OVER, CM.NORMAL, 1.0).astype(np.uint32)
        assert np.array_equal(got, np.minimum(255, s255 + (b * (255 - s255[:, 3:4]) + 127) // 255))
    # a transparent source leaves the backdrop unchanged — whatever its colour bytes are (the load clamps them to 0)
    backdrop = inputs[1][2][:1 << 16]
    clear = np.zeros_like(backdrop)
    clear[:, :3] = inputs[1][1][:1 << 16, :3]
    for op in CM.KEEP_BACKDROP:
        for mode in range(len(CM.MODES)):
            for opacity in (1.0, 0.5):
                assert np.array_equal(library_texels(lib, clear, backdrop, op, mode, opacity), CM.load(backdrop).astype(np.uint8)), (CM.OPS[op], CM.MODES[mode])
    # opacity 0 makes every source transparent
    for op in CM.KEEP_BACKDROP:
        assert np.array_equal(library_texels(lib, inputs[1][1][:1 << 16], backdrop, op, CM.SCREEN, 0.0), CM.load(backdrop).astype(np.uint8))


def test_the_geometry_of_the_model():
    rng = np.random.RandomState(3)
    backdrop, source = CM.random_image(rng, 7, 5), CM.random_image(rng, 4, 6)
    for x, y in ((0, 0), (-3, -2), (5, 1), (7, 0), (0, -6), (-(1 << 31), (1 << 31) - 1), (6, 4)):
        placed = CM.place(source, 7, 5, x, y)
        for j in range(5):
            for i in range(7):
                inside = 0 <= i - x < 4 and 0 <= j - y < 6
                assert np.array_equal(placed[j, i], source[j - y, i - x] if inside else np.zeros(4, dtype=np.uint8)), (x, y, i, j)
        assert np.array_equal(CM.composite(backdrop, source, CM.SRC_IN, CM.NORMAL, 255, x, y), CM.texels(placed, backdrop, CM.SRC_IN, CM.NORMAL, 255))
    assert not CM.composite(backdrop, source, CM.SRC_IN, CM.NORMAL, 255, 7, 0).any()  # SRC_IN clears outside the source


def test_validation_statuses_and_texts(lib):
    def how(op=3, mode=0, opacity=1.0):
        return _ffi.CompositeC(op, mode, opacity, 0, 0)
    assert lib.crh_composite_validate(None) == _ffi.ERR_INVALID_ARGUMENT
    for ok in (how(), how(12, 8, 0.0), how(0, 0, 0.5)):
        assert lib.crh_composite_validate(C.byref(ok)) == _ffi.OK
    for bad, text in ((how(op=13), "crh_composite_validate: op is above CRH_COMPOSITE_PLUS"), (how(mode=9), "crh_composite_validate: mode is above CRH_BLEND_EXCLUSION"),
                      (how(opacity=1.0001), "crh_composite_validate: opacity is outside [0, 1]"), (how(opacity=-0.25), "crh_composite_validate: opacity is outside [0, 1]"),
                      (how(op=0xFFFFFFFF), "crh_composite_validate: op is above CRH_COMPOSITE_PLUS")):
        assert lib.crh_composite_validate(C.byref(bad)) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.crh_last_error().decode() == text
    for opacity in (float("nan"), float("inf"), -float("inf")):
        assert lib.crh_composite_validate(C.byref(how(opacity=opacity))) == _ffi.ERR_NON_FINITE
    # a refused call writes nothing
    source, backdrop = CM.grid_pairs()
    out = np.full(source.shape, 0xAB, dtype=np.uint8)
    for bad, status in ((how(op=13), _ffi.ERR_INVALID_ARGUMENT), (how(mode=9), _ffi.ERR_INVALID_ARGUMENT), (how(opacity=2.0), _ffi.ERR_INVALID_ARGUMENT), (how(opacity=float("nan")), _ffi.ERR_NON_FINITE)):
        assert lib.crh_composite_texels(C.byref(bad), source.ctypes.data, backdrop.ctypes.data, len(source), out.ctypes.data) == status
        assert (out == 0xAB).all()
    assert lib.crh_composite_texels(None, source.ctypes.data, backdrop.ctypes.data, len(source), out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_composite_texels(C.byref(how()), None, backdrop.ctypes.data, len(source), out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_composite_texels(C.byref(how()), source.ctypes.data, backdrop.ctypes.data, len(source), None) == _ffi.ERR_INVALID_ARGUMENT
    assert (out == 0xAB).all()
    # the device entry points validate before they touch a device
    image = C.c_void_p(0x1234)
    assert lib.crh_image_composite(None, None, C.byref(how()), C.byref(image)) == _ffi.ERR_INVALID_ARGUMENT and image.value == 0x1234
    assert lib.crh_frame_load_image(None, None) == _ffi.ERR_INVALID_ARGUMENT


def test_the_python_mirror(lib):
    assert [int(v) for v in CompositeOp] == list(range(13)) and [int(v) for v in BlendMode] == list(range(9))
    assert [v.name.upper() for v in CompositeOp] == [n.replace("_", "") for n in CM.OPS]
    assert [v.name.upper() for v in BlendMode] == [n.replace("_", "") for n in CM.MODES]
    source, backdrop = CM.grid_pairs()
    got = composite_texels(source, backdrop, CompositeOp.SrcAtop, BlendMode.HardLight, 0.6)
    assert got.dtype == np.uint8 and np.array_equal(got, CM.texels(source, backdrop, CM.SRC_ATOP, CM.HARD_LIGHT, CM.opacity_code(0.6)))
    assert np.array_equal(composite_texels(source, backdrop), CM.texels(source, backdrop, CM.SRC_OVER, CM.NORMAL, 255))
    for bad in (dict(op=13), dict(mode=9), dict(opacity=1.5), dict(opacity=float("nan"))):
        with pytest.raises(ContrastError):
            composite_texels(source, backdrop, **bad)
    with pytest.raises(ContrastError):
        composite_texels(source, backdrop[:-1])
    assert hasattr(R.Image, "composite") and hasattr(R.Frame, "load_image")
    assert "offset = (dx - source.origin[0], dy - source.origin[1])" in R.Image.composite.__doc__
    sig = lib._crh_signatures
    assert sig["crh_composite_texels"][1][3] is C.c_uint64 and sig["crh_image_composite"][1][2] is C.POINTER(_ffi.CompositeC)
    assert C.sizeof(_ffi.CompositeC) == 20


def test_the_library_exports_and_the_enums_agree_across_header_python_and_ffi_rs(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    exports = open(b.write_export_map()).read()
    for name in NAMES:
        assert f"    {name};\n" in exports
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    assert committed == fresh
    for prefix, names, mirror in (("CRH_COMPOSITE_", CM.OPS, CompositeOp), ("CRH_BLEND_", CM.MODES, BlendMode)):
        for value, name in enumerate(names):
            assert re.search(rf"\b{prefix}{name} = {value}[,\s]", header), (prefix, name)
            assert f"pub const {prefix}{name}: u32 = {value};" in committed
            assert int(mirror[name.title().replace("_", "")]) == value
    assert re.search(r"pub struct crh_composite \{\s*pub op: u32,\s*pub mode: u32,\s*pub opacity: f32,\s*pub x: i32,\s*pub y: i32,\s*\}", committed)
    assert "pub fn crh_composite_validate(how: *const crh_composite) -> crh_status;" in committed
    assert "pub fn crh_composite_texels(how: *const crh_composite, source_rgba8: *const c_void, backdrop_rgba8: *const c_void, n: u64, out_rgba8: *mut c_void) -> crh_status;" in committed
    assert "pub fn crh_image_composite(backdrop: *const crh_image, source: *const crh_image, how: *const crh_composite, out: *mut *mut crh_image) -> crh_status;" in committed
    assert "pub fn crh_frame_load_image(frame: *mut crh_frame, image: *const crh_image) -> crh_status;" in committed
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub enum CompositeOp {", "pub enum BlendMode {", "pub fn composite_texels(source: &[u8], backdrop: &[u8], op: CompositeOp, mode: BlendMode, opacity: f32) -> Result<Vec<u8>, Error>",
                 "pub fn composite(&self, source: &Image, op: CompositeOp, mode: BlendMode, opacity: f32, offset: (i32, i32)) -> Result<Image, Error>",
                 "pub fn load_image(&mut self, image: &Image) -> Result<(), Error>"):
        assert text in shim, text
    for enum, names in (("CompositeOp", CM.OPS), ("BlendMode", CM.MODES)):
        body = shim[shim.index(f"pub enum {enum} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"(\w+) = (\d+),", body) == [(n.title().replace("_", ""), str(v)) for v, n in enumerate(names)]


def test_the_cpp_mirror_computes_the_models_bytes(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    source, backdrop = CM.grid_pairs()
    with tempfile.TemporaryDirectory() as tmp:
        binary, pairs = os.path.join(tmp, "composite_harness"), os.path.join(tmp, "pairs.bin")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "composite_harness.cpp"),
               "-o", binary, "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        with open(pairs, "wb") as f:
            f.write(source.tobytes() + backdrop.tobytes())
        done = subprocess.run([binary, pairs, "0.6"], capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr)
    lines = done.stdout.splitlines()
    assert len(lines) == 13 * 9
    o = CM.opacity_code(0.6)
    assert o == 153
    for line in lines:
        op, mode, payload = line.split()
        expect = CM.texels(source, backdrop, int(op), int(mode), o)
        assert bytes.fromhex(payload) == expect.tobytes(), (CM.OPS[int(op)], CM.MODES[int(mode)])
