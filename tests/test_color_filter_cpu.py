"""crh_image_color_filter without a GPU: crh_color_filter_texels (host only, the rule of csrc/color_filter.hpp that the kernel runs) byte for byte
against the integer model of tests/color_filter_model.py; the unpremultiply exhaustively; that model within its derived bound of the
real-valued formula in float64; the consequences the header states; crh_color_filter_validate's errors; the Python / C++ / Rust mirrors; and
one run of the rule as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import ColorMatrix, ContrastError, _ffi, color_filter_texels
from contrast_renderer_amd import renderer as R

import color_filter_model as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_color_filter_validate", "crh_color_filter_texels", "crh_image_color_filter")
N_RANDOM = 1 << 20
MATRICES = FM.matrices()
F, B = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


@pytest.fixture(scope="module")
def inputs():
    """(name, texels): all 32 896 pairs c <= a with the three colours varied from c, and 2^20 random texels of which every fifth is not
    premultiplied. Made once, never written."""
    made = [("pairs", FM.all_pairs()), ("random", FM.random_texels(N_RANDOM, seed=12))]
    for _, t in made:
        t.setflags(write=False)
    loose = (made[1][1][:, :3] > made[1][1][:, 3:4]).any(axis=1)
    assert loose.any() and not loose[np.arange(N_RANDOM) % 5 != 0].any()
    return made


def library_texels(lib, texels, matrix, tables):
    m = None if matrix is None else (C.c_float * 20)(*matrix)
    t = None if tables is None else np.ascontiguousarray(tables).ctypes.data_as(B)
    out = np.full(texels.shape, 0xAB, dtype=np.uint8)
    assert lib.crh_color_filter_texels(m, t, texels.ctypes.data, len(texels), out.ctypes.data) == _ffi.OK
    return out


@pytest.mark.parametrize("name,matrix", MATRICES, ids=[n for n, _ in MATRICES])
def test_the_library_equals_the_integer_model(lib, inputs, name, matrix):
    for what, texels in inputs:
        v = FM.apply_matrix(FM.unpremultiply(FM.load(texels)), FM.coefficients(matrix))
        for tables_name, tables in FM.table_sets():
            expect = FM.premultiply(FM.apply_tables(v, tables))
            got = library_texels(lib, texels, matrix, tables)
            if not np.array_equal(got, expect):
                k = int(np.argwhere((got != expect).any(axis=1))[0][0])
                pytest.fail(f"{name} tables={tables_name} {what}: texel {k} {texels[k]} -> {got[k]}, the model {expect[k]}")
            assert (got[:, :3] <= got[:, 3:4]).all()  # c' <= a'


def test_the_extremes_reach_the_bound_of_the_sums():
    u = np.array([[255, 255, 255, 255]], dtype=np.int64)
    for sign in (1, -1):
        k = FM.coefficients([sign * 16.0] * 20)
        assert (np.abs(k) == 1 << 20).all()
        n = u @ k[:, :4].T + 255 * k[:, 4] + 32768
        assert (np.abs(n) == 5 * 255 * (1 << 20) + sign * 32768).all() and 5 * 255 * (1 << 20) + 32768 == 1336967168 < 1 << 31
    assert np.array_equal(FM.coefficients(None), 65536 * np.eye(4, 5, dtype=np.int64))


def test_the_identity_returns_every_premultiplied_texel(lib, inputs):
    for what, texels in inputs:
        loaded = FM.load(texels).astype(np.uint8)
        for matrix in (None, FM.identity(), FM.opacity(1)):
            for tables in (None, FM.identity_tables()):
                assert np.array_equal(library_texels(lib, texels, matrix, tables), loaded), (what, matrix is None, tables is None)
        assert np.array_equal(FM.texels(texels), loaded)
    pairs = inputs[0][1]
    assert np.array_equal(library_texels(lib, pairs, None, None), pairs)  # (premultiplied: the load changes nothing)
    # a = 0 goes in as (0, 0, 0, 0) whatever its colour bytes are
    clear = inputs[1][1][:4096].copy()
    clear[:, 3] = 0
    assert clear[:, :3].any() and not library_texels(lib, clear, FM.saturate(2), None).any()
    bias = library_texels(lib, clear, FM.flood(1, 0.5, 0, 0)[:19] + [1.0], None)  # alpha from the bias alone: the colour is the flood's, not the bytes'
    assert (bias == np.array([255, 128, 0, 255], dtype=np.uint8)).all()


def test_the_unpremultiply_exhaustively_through_the_library(lib):
    """With every a' table entry 255 the premultiply is the identity, so the output colour is u itself: all 32 896 pairs c <= a against
    (255 c + a / 2) / a in Python-wide integers."""
    pairs = FM.all_pairs()
    tables = FM.identity_tables()
    tables[768:] = 255
    got = library_texels(lib, pairs, FM.identity(), tables).astype(np.int64)
    c, a = pairs[:, :3].astype(np.int64), pairs[:, 3:4].astype(np.int64)
    u = np.where(a > 0, (255 * c + a // 2) // np.maximum(a, 1), 0)
    assert np.array_equal(got[:, :3], u) and (got[:, 3] == 255).all()
    # every c for every a in the red channel (the varied colours of all_pairs do not cover every pair in g and b)
    assert len({(int(x), int(y)) for x, y in zip(pairs[:, 0], pairs[:, 3])}) == 32896
    for channel in (1, 2):
        moved = pairs.copy()
        moved[:, [0, channel]] = moved[:, [channel, 0]]
        got = library_texels(lib, moved, FM.identity(), tables).astype(np.int64)
        assert np.array_equal(got[:, channel], u[:, 0])
    assert np.array_equal(library_texels(lib, pairs, FM.opacity(1), FM.identity_tables()), pairs)


def test_the_stated_consequences(lib, inputs):
    for what, texels in inputs:
        texels = texels[:1 << 17]
        loaded = FM.load(texels)
        a = loaded[:, 3]
        # the flood: round(colour * round(alpha a)), with the colour's code round(255 colour)
        r, g, b, alpha = 0.2, 0.4, 0.9, 0.6
        got = library_texels(lib, texels, FM.flood(r, g, b, alpha), None).astype(np.int64)
        k = FM.coefficients(FM.flood(r, g, b, alpha))
        a_out = (k[3, 3] * a + 32768) >> 16
        assert np.array_equal(a_out, np.floor(float(np.float32(alpha)) * a + 0.5).astype(np.int64))  # round(alpha a)
        codes = [int(np.floor(255.0 * float(np.float32(v)) + 0.5)) for v in (r, g, b)]
        assert codes == [51, 102, 229]  # (the f32 nearest 0.9 lies below it: 229.4999)
        assert np.array_equal(got[:, 3], a_out)
        for c in range(3):
            assert np.array_equal(got[:, c], (codes[c] * a_out + 127) // 255)
        # the shadow's colour: black at an opacity
        shadow = library_texels(lib, texels, FM.flood(0, 0, 0, 0.5), None)
        assert not shadow[:, :3].any() and np.array_equal(shadow[:, 3], (a + 1) >> 1)
        # luminanceToAlpha: colour (0, 0, 0), alpha from the straight colour
        mask = library_texels(lib, texels, FM.luminance_to_alpha(), None)
        assert not mask[:, :3].any()
        u = FM.unpremultiply(loaded)
        k = FM.coefficients(FM.luminance_to_alpha())
        assert np.array_equal(mask[:, 3], np.clip((u[:, :3] @ k[3, :3] + 32768) >> 16, 0, 255))
        # invert tables on the identity matrix: straight codes 255 - u, alpha 255 - a
        inverted = library_texels(lib, texels, None, FM.invert_tables()).astype(np.int64)
        assert np.array_equal(inverted[:, 3], 255 - a) and np.array_equal(inverted[:, :3], ((255 - u[:, :3]) * (255 - a[:, None]) + 127) // 255)


@pytest.mark.parametrize("name,matrix", MATRICES, ids=[n for n, _ in MATRICES])
def test_the_integer_model_is_within_its_bound_of_the_real_formula(inputs, name, matrix):
    """The bound is FM.bounds' derivation (the header states it): per matrix, e_c + e_a + e_c e_a / 255 + 1/2 on a colour and e_a on alpha.
    Measured worst cases over these inputs (the 32 896 pairs and 2^18 random texels), colour / alpha, against the bounds (also in DESIGN.md):
      identity 0 / 0 (2.0215 / 0.5097); saturate0 1.3520 / 0 (2.0215 / 0.5097); saturate2 2.1150 / 0 (2.9513 / 0.5097);
      hue90 1.8960 / 0 (2.5966 / 0.5097); luminanceToAlpha 0 / 0.9875 (2.0215 / 1.0097); flood(0.2, 0.4, 0.9, 0.6) 1.0600 / 0.4000
      (1.5205 / 0.5097); random 0.3225 / 0.3225 (34.16 / 18.08) and all +16, all -16 0 / 0 (51.88 / 24.51): these three clamp nearly every value."""
    worst_c = worst_a = 0.0
    bound_c, bound_a = FM.bounds(matrix)
    for what, texels in inputs:
        texels = texels[:1 << 18]
        error = np.abs(FM.texels(texels, matrix).astype(np.float64) - FM.real(texels, matrix))
        worst_c, worst_a = max(worst_c, float(error[:, :3].max())), max(worst_a, float(error[:, 3].max()))
    print(f"{name}: worst colour error {worst_c:.4f} (bound {bound_c:.4f}), alpha {worst_a:.4f} (bound {bound_a:.4f})")
    assert worst_c <= bound_c + 1e-9 and worst_a <= bound_a + 1e-9


def test_validation_statuses_and_texts(lib):
    def m(**at):
        values = FM.identity()
        for k, v in at.items():
            values[int(k[1:])] = v
        return (C.c_float * 20)(*values)
    text = "crh_color_filter_validate: a coefficient is outside [-CRH_COLOR_MATRIX_MAX, CRH_COLOR_MATRIX_MAX]"
    tables = FM.invert_tables()
    assert lib.crh_color_filter_validate(None, None) == _ffi.OK
    assert lib.crh_color_filter_validate(m(), tables.ctypes.data_as(B)) == _ffi.OK
    for ok in (m(_7=16.0), m(_19=-16.0), (C.c_float * 20)(*[16.0] * 20), (C.c_float * 20)(*[-16.0] * 20)):
        assert lib.crh_color_filter_validate(ok, None) == _ffi.OK
    above = float(np.nextafter(np.float32(16.0), np.float32(17.0)))
    assert np.float32(above) == np.float32(16.000002)
    for bad in (m(_7=above), m(_0=-above), m(_19=17.0), m(_4=-1e30)):
        assert lib.crh_color_filter_validate(bad, None) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.crh_last_error().decode() == text
    for value in (float("nan"), float("inf"), -float("inf")):
        assert lib.crh_color_filter_validate(m(_13=value), None) == _ffi.ERR_NON_FINITE
    assert lib.crh_color_filter_validate(m(_0=17.0, _13=float("nan")), None) == _ffi.ERR_NON_FINITE
    # a refused call writes nothing
    texels = FM.all_pairs()
    out = np.full(texels.shape, 0xAB, dtype=np.uint8)
    for bad, status in ((m(_7=above), _ffi.ERR_INVALID_ARGUMENT), (m(_13=float("nan")), _ffi.ERR_NON_FINITE)):
        assert lib.crh_color_filter_texels(bad, None, texels.ctypes.data, len(texels), out.ctypes.data) == status
        assert (out == 0xAB).all()
    assert lib.crh_color_filter_texels(None, None, None, len(texels), out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.crh_color_filter_texels(None, None, texels.ctypes.data, len(texels), None) == _ffi.ERR_INVALID_ARGUMENT
    assert (out == 0xAB).all()
    assert lib.crh_color_filter_texels(None, None, None, 0, None) == _ffi.OK
    # the device entry point validates before it touches a device
    image = C.c_void_p(0x1234)
    assert lib.crh_image_color_filter(None, None, None, C.byref(image)) == _ffi.ERR_INVALID_ARGUMENT and image.value == 0x1234


def test_in_place_and_unaligned_bytes(lib):
    texels = FM.random_texels(4099, seed=3)
    matrix, tables = FM.hue_rotate(90), FM.random_tables(9)
    expect = FM.texels(texels, matrix, tables)
    m, t = (C.c_float * 20)(*matrix), tables.ctypes.data_as(B)
    same = texels.copy()
    assert lib.crh_color_filter_texels(m, t, same.ctypes.data, len(same), same.ctypes.data) == _ffi.OK
    assert np.array_equal(same, expect)
    for shift_in, shift_out in ((1, 0), (0, 3), (3, 1), (2, 2)):
        raw_in, raw_out = np.zeros(texels.size + 8, dtype=np.uint8), np.full(texels.size + 8, 0xCD, dtype=np.uint8)
        raw_in[shift_in:shift_in + texels.size] = texels.ravel()
        assert lib.crh_color_filter_texels(m, t, raw_in.ctypes.data + shift_in, len(texels), raw_out.ctypes.data + shift_out) == _ffi.OK
        assert np.array_equal(raw_out[shift_out:shift_out + texels.size].reshape(-1, 4), expect)
        assert (raw_out[:shift_out] == 0xCD).all() and (raw_out[shift_out + texels.size:] == 0xCD).all()


def test_the_python_mirror(lib):
    # the SVG filter-effects coefficients, float64, rounded to f32 once
    f32 = lambda rows: [float(np.float32(v)) for v in np.asarray(rows, dtype=np.float64).ravel()]  # noqa: E731
    assert ColorMatrix.identity() == f32(np.eye(4, 5))
    assert ColorMatrix.saturate(1) == pytest.approx(f32(np.eye(4, 5)), abs=1e-7)
    assert ColorMatrix.saturate(0)[:15] == f32([[0.213, 0.715, 0.072, 0, 0]] * 3)
    s = 2.0
    assert ColorMatrix.saturate(s) == f32([[0.213 + 0.787 * s, 0.715 - 0.715 * s, 0.072 - 0.072 * s, 0, 0], [0.213 - 0.213 * s, 0.715 + 0.285 * s, 0.072 - 0.072 * s, 0, 0],
                                           [0.213 - 0.213 * s, 0.715 - 0.715 * s, 0.072 + 0.928 * s, 0, 0], [0, 0, 0, 1, 0]])
    assert ColorMatrix.hue_rotate(0) == pytest.approx(f32(np.eye(4, 5)), abs=1e-7)
    # hueRotate(90): cos = 0, sin = 1 (to 6e-17) in the specification's matrix
    assert ColorMatrix.hue_rotate(90) == pytest.approx(f32([[0.213 - 0.213, 0.715 - 0.715, 0.072 + 0.928, 0, 0], [0.213 + 0.143, 0.715 + 0.140, 0.072 - 0.283, 0, 0],
                                                            [0.213 - 0.787, 0.715 + 0.715, 0.072 + 0.072, 0, 0], [0, 0, 0, 1, 0]]), abs=1e-7)
    assert ColorMatrix.luminance_to_alpha() == f32([[0] * 5] * 3 + [[0.2125, 0.7154, 0.0721, 0, 0]])
    assert ColorMatrix.flood(0.2, 0.4, 0.9, 0.6) == f32([[0, 0, 0, 0, 0.2], [0, 0, 0, 0, 0.4], [0, 0, 0, 0, 0.9], [0, 0, 0, 0.6, 0]])
    assert ColorMatrix.opacity(0.25) == f32([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0.25, 0]])
    for ours, models in ((ColorMatrix.saturate(2), FM.saturate(2)), (ColorMatrix.hue_rotate(90), FM.hue_rotate(90)), (ColorMatrix.flood(0.2, 0.4, 0.9, 0.6), FM.flood(0.2, 0.4, 0.9, 0.6))):
        assert ours == models and len(ours) == 20 and all(type(v) is float for v in ours)
    texels = FM.all_pairs()
    got = color_filter_texels(texels, ColorMatrix.hue_rotate(90), FM.random_tables(9))
    assert got.dtype == np.uint8 and np.array_equal(got, FM.texels(texels, FM.hue_rotate(90), FM.random_tables(9)))
    assert np.array_equal(color_filter_texels(texels), texels)
    assert np.array_equal(color_filter_texels(texels, tables=FM.invert_tables().reshape(4, 256)), FM.texels(texels, None, FM.invert_tables()))
    assert np.array_equal(color_filter_texels(texels, np.float32(ColorMatrix.saturate(0)).reshape(4, 5)), FM.texels(texels, FM.saturate(0)))
    for bad in (dict(matrix=[1.0] * 19), dict(matrix=[17.0] * 20), dict(matrix=[float("nan")] * 20), dict(tables=np.zeros(1023, dtype=np.uint8)), dict(tables=np.zeros(1024, dtype=np.int32))):
        with pytest.raises(ContrastError):
            color_filter_texels(texels, **bad)
    with pytest.raises(ContrastError):
        color_filter_texels(texels[:, :3])
    assert hasattr(R.Image, "color_filter") and R.COLOR_MATRIX_MAX == 16.0
    sig = lib._crh_signatures
    assert sig["crh_color_filter_texels"][1][3] is C.c_uint64 and sig["crh_image_color_filter"][1][1] is F and sig["crh_image_color_filter"][1][2] is B


def test_the_library_exports_and_the_mirrors_agree_across_header_python_and_ffi_rs(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    exports = open(b.write_export_map()).read()
    for name in NAMES:
        assert f"    {name};\n" in exports
    assert any(os.path.basename(h) == "color_filter.hpp" for h in b.header_deps())
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    assert re.search(r"#define CRH_COLOR_MATRIX_MAX 16\.0f\b", header)
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    assert committed == fresh
    assert "pub fn crh_color_filter_validate(matrix: *const f32, tables: *const u8) -> crh_status;" in committed
    assert "pub fn crh_color_filter_texels(matrix: *const f32, tables: *const u8, rgba8: *const c_void, n: u64, out: *mut c_void) -> crh_status;" in committed
    assert "pub fn crh_image_color_filter(src: *const crh_image, matrix: *const f32, tables: *const u8, out: *mut *mut crh_image) -> crh_status;" in committed
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub struct ColorMatrix;", "pub fn identity() -> [f32; 20]", "pub fn saturate(s: f64) -> [f32; 20]", "pub fn hue_rotate(degrees: f64) -> [f32; 20]",
                 "pub fn luminance_to_alpha() -> [f32; 20]", "pub fn flood(r: f64, g: f64, b: f64, a: f64) -> [f32; 20]", "pub fn opacity(a: f64) -> [f32; 20]",
                 "pub fn color_filter_texels(texels: &[u8], matrix: Option<&[f32; 20]>, tables: Option<&[u8; 1024]>) -> Result<Vec<u8>, Error>",
                 "pub fn color_filter(&self, matrix: Option<&[f32; 20]>, tables: Option<&[u8; 1024]>) -> Result<Image, Error>"):
        assert text in shim, text
    # the shim's coefficients are the specification's: every literal of the Python constructors' rows appears in its rows
    body = shim[shim.index("pub struct ColorMatrix;"):shim.index("pub fn color_filter_texels")]
    for literal in ("0.213", "0.787", "0.715", "0.285", "0.072", "0.928", "0.143", "0.140", "0.283", "0.2125", "0.7154", "0.0721"):
        assert literal in body, literal


def test_the_cpp_mirror_computes_the_models_bytes(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    texels = np.concatenate([FM.all_pairs()[::7], FM.random_texels(1024, seed=4)])
    with tempfile.TemporaryDirectory() as tmp:
        binary, data = os.path.join(tmp, "color_filter_harness"), os.path.join(tmp, "texels.bin")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "color_filter_harness.cpp"),
               "-o", binary, "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        with open(data, "wb") as f:
            f.write(texels.tobytes())
        done = subprocess.run([binary, data], capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr)
    lines = done.stdout.splitlines()
    assert len(lines) == 6 * 3
    ours = {"identity": ColorMatrix.identity(), "saturate": ColorMatrix.saturate(2), "hue_rotate": ColorMatrix.hue_rotate(90), "luminance_to_alpha": ColorMatrix.luminance_to_alpha(),
            "flood": ColorMatrix.flood(0.2, 0.4, 0.9, 0.6), "opacity": ColorMatrix.opacity(0.25)}
    seen = 0
    for line in lines:
        fields = line.split()
        if fields[0] == "matrix":
            # (libm's cos(pi / 2) and numpy's may differ in the last bit of a double: one f32 step at the most)
            assert [float(v) for v in fields[2:]] == pytest.approx(ours[fields[1]], abs=1e-7), fields[1]
            matrix = [float(v) for v in fields[2:]]
            continue
        name, with_tables, payload = fields
        expect = FM.texels(texels, matrix, FM.invert_tables() if int(with_tables) else None)
        assert bytes.fromhex(payload) == expect.tobytes(), (name, with_tables)
        seen += 1
    assert seen == 12


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """A stand-alone program (its own main, no library, nothing loaded into python) around csrc/color_filter.hpp, the rule that
    crh_color_filter_texels runs: compiled as host code with the two sanitizers (the flag goes to the host compilation alone) and run once."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        binary = os.path.join(tmp, "color_filter_sanitize")
        # -x c++ and -Xarch_host: plain host C++, the sanitizers on the host alone (no device pass; clang links the sanitizers' runtime statically, so the program needs nothing preloaded)
        cmd = [hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
               "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), "-I", os.path.join(ROOT, "contrast_renderer_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "color_filter_sanitize.cpp"), "-o", binary]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert done.stdout.strip().endswith("36992 texels, 0 failures")
