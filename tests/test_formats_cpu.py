"""The BGRA / sRGB frame formats on the CPU: the committed sRGB codec tables against their float64 definition (include/contrast_hip.h at
CRH_FORMAT_RGBA8_SRGB), the generator's drift, and the format constants of the C header, the Python, C++ and Rust mirrors."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = os.path.join(ROOT, "contrast_renderer_amd", "csrc", "srgb_tables.h")
FORMATS = {"CRH_FORMAT_RGBA8": 0, "CRH_FORMAT_RGBA16F": 1, "CRH_FORMAT_RGBA8_ATTACHMENT": 2, "CRH_FORMAT_BGRA8": 3, "CRH_FORMAT_BGRA8_ATTACHMENT": 4,
           "CRH_FORMAT_RGBA8_SRGB": 5, "CRH_FORMAT_RGBA8_SRGB_ATTACHMENT": 6, "CRH_FORMAT_BGRA8_SRGB": 7, "CRH_FORMAT_BGRA8_SRGB_ATTACHMENT": 8}


def linear64(s):
    return s / 12.92 if s <= 0.04045 else ((s + 0.055) / 1.055) ** 2.4


def committed_tables():
    """-> (D[256], T[257]) as float32 arrays, parsed from csrc/srgb_tables.h (T[0] = -inf, T[256] = +inf)."""
    text = open(TABLES).read()

    def table(name):
        body = text.split(f"#define {name}")[1].split("}")[0]
        out = []
        for tok in re.findall(r"-?__builtin_huge_valf\(\)|-?0x[0-9a-fA-F.]+p[+-]?\d+f", body):
            out.append(float("-inf") if tok.startswith("-__builtin") else float("inf") if tok.startswith("__builtin") else float.fromhex(tok[:-1]))
        return np.array(out, dtype=np.float64).astype(np.float32)
    return table("CRH_SRGB_DECODE_INIT"), table("CRH_SRGB_THRESHOLD_INIT")


def encode(x):
    """The codec's encode of float32 values: #{k in 1..255 : x >= T[k]}, NaN -> 0 (numpy, vectorised)."""
    _, t = committed_tables()
    x = np.asarray(x, dtype=np.float32)
    codes = np.searchsorted(t[1:256], x, side="right").astype(np.int64)
    return np.where(np.isnan(x), 0, codes).astype(np.uint8)


def decode(codes):
    d, _ = committed_tables()
    return d[np.asarray(codes, dtype=np.int64)]


def encode64(x):
    """The sRGB curve in float64, the exact inverse of linear64 (breakpoint linear64(0.04045))."""
    x = np.asarray(x, dtype=np.float64)
    knee = 0.04045 / 12.92
    with np.errstate(invalid="ignore"):
        s = np.where(x <= knee, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0), 1.0 / 2.4) - 0.055)
    return np.clip(s, 0.0, 1.0)


def test_committed_tables_are_what_the_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_srgb_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_tables_equal_the_float64_definition_bit_for_bit():
    d, t = committed_tables()
    assert d.shape == (256,) and t.shape == (257,)
    want_d = np.array([linear64(c / 255.0) for c in range(256)], dtype=np.float64).astype(np.float32)  # round to nearest
    assert np.array_equal(d.view(np.uint32), want_d.view(np.uint32))
    assert d[0] == 0.0 and d[255] == 1.0
    for k in range(1, 256):
        v = linear64((k - 0.5) / 255.0)
        tk = t[k]
        below = np.nextafter(tk, np.float32(-np.inf))
        assert float(tk) >= v and float(below) < v, k  # the smallest float32 not below v
    assert t[0] == -np.inf and t[256] == np.inf
    assert np.array_equal(encode(d), np.arange(256, dtype=np.uint8))


def test_thresholds_increase_and_encode_is_the_rounded_curve():
    _, t = committed_tables()
    assert np.all(np.diff(t[1:256].astype(np.float64)) > 0)
    near = []
    for k in range(1, 256):
        bits = int(t[k].view(np.uint32))
        near.append(np.arange(bits - 4, bits + 5, dtype=np.uint32).view(np.float32))
    near = np.concatenate(near)
    rng = np.random.RandomState(1)
    rand = np.concatenate([rng.uniform(-0.05, 1.05, 500_000), np.exp(rng.uniform(np.log(1e-9), 0.0, 500_000))]).astype(np.float32)
    for x in (near, rand):
        want = np.floor(255.0 * encode64(x) + 0.5).astype(np.int64)
        got = encode(x).astype(np.int64)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:5]]
    special = np.array([0.0, -0.0, -1.0, -np.inf, 1.0, 2.0, np.inf, np.nan], dtype=np.float32)
    assert encode(special).tolist() == [0, 0, 0, 0, 255, 255, 255, 0]


def test_the_reference_f32_helpers_agree_within_one_code():
    from contrast_renderer_amd import utils
    d, _ = committed_tables()
    for c in range(256):
        lin = utils.srgb_to_linear([c / 255.0, 0.0, 0.0, 1.0])[0]
        assert abs(int(encode(lin)) - c) <= 1, c
        back = utils.linear_to_srgb([d[c], 0.0, 0.0, 1.0])[0]
        assert abs(int(np.floor(np.float32(back) * 255.0 + 0.5)) - c) <= 1, c


def test_the_header_and_the_mirrors_agree_on_the_formats():
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    for name, value in FORMATS.items():
        assert re.search(rf"\b{name}\s*=\s*{value}\b", header), name
    from contrast_renderer_amd import renderer as R
    for name, value in FORMATS.items():
        assert getattr(R, name[len("CRH_"):]) == value, name
    tf = R.TextureFormat
    assert [int(tf.Rgba8Unorm), int(tf.Bgra8Unorm), int(tf.Rgba8UnormSrgb), int(tf.Bgra8UnormSrgb)] == [0, 3, 5, 7]
    assert [f.attachment for f in tf] == [2, 4, 6, 8]
    assert R.ColorTargetState().format == tf.Rgba8Unorm
    ffi = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    for name, value in FORMATS.items():
        assert f"pub const {name}: u32 = {value};" in ffi, name
    lib = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for wgpu, c in (("Rgba8Unorm", "RGBA8"), ("Bgra8Unorm", "BGRA8"), ("Rgba8UnormSrgb", "RGBA8_SRGB"), ("Bgra8UnormSrgb", "BGRA8_SRGB")):
        assert f"{wgpu} = ffi::CRH_FORMAT_{c}," in lib
        assert re.search(rf"\b{wgpu} = CRH_FORMAT_{c}\b", open(os.path.join(ROOT, "include", "contrast_renderer.hpp")).read()), wgpu
    assert "pub format: TextureFormat" in lib


def test_the_cpp_mirror_compiles_with_the_new_formats(tmp_path):
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    src = tmp_path / "formats.cpp"
    src.write_text('#include "contrast_renderer.hpp"\n'
                   "using namespace contrast_renderer;\n"
                   "static_assert((uint32_t)TextureFormat::Bgra8UnormSrgb == CRH_FORMAT_BGRA8_SRGB, \"\");\n"
                   "int check(Renderer& r) {\n"
                   "    Configuration c;\n"
                   "    ColorTargetState s;\n"
                   "    s.format = TextureFormat::Bgra8Unorm;\n"
                   "    c.blending = s;\n"
                   "    Frame f(r, 16, 16);\n"
                   "    Frame g(r, 16, 16, attachment_format(TextureFormat::Rgba8UnormSrgb));\n"
                   "    return (int)r.format() + (int)r.get_blending().format;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
