"""crh_image_variable_blur without a GPU (include/contrast_hip.h states the rule): crh_variable_blur_sigma against the numpy model of
tests/variable_blur_model.py for every code, crh_variable_blur_texels and the Python mirror byte for byte against the model on the
cases of the device test, the rule's five consequences with the host rule, the refused calls with their statuses, texts and order, a
C++ harness, and the rule as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, Channel, ContrastError, _ffi, variable_blur_sigma, variable_blur_texels

import blur_model as B
import variable_blur_model as M
from test_image_api_contract_cpu import ImageHead

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_variable_blur_validate", "crh_variable_blur_sigma", "crh_variable_blur_texels", "crh_image_variable_blur")
PREFIX = "crh_variable_blur_validate: "
OK, INVALID, NON_FINITE = _ffi.OK, _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_NON_FINITE


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def how_of(sigma_x=(0.0, 3.0), sigma_y=(0.0, 3.0), channel=3, edge=1):
    return _ffi.VariableBlurC((C.c_float * 2)(*sigma_x), (C.c_float * 2)(*sigma_y), channel, edge)


def bits(value):
    return struct.pack("<f", value)


def host(case):
    kind, w, h, pair, edge, channel = case
    sx, sy = M.PAIRS[pair]
    return variable_blur_texels(M.source(w, h), M.mask(kind, w, h), (sx[1], sy[1]), (sx[0], sy[0]), Channel(channel), BlurEdge(edge))


def test_the_symbols_are_exported(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None


# ascending, descending, equal, the whole range either way, and a pair whose difference is not a float (2^-20 beside 64)
SIGMA_PAIRS = ((0.0, 64.0), (64.0, 0.0), (3.0, 3.0), (0.0, 0.0), (1.5, 40.0), (40.0, 1.5), (2.0 ** -20, 64.0), (0.1, 0.7), (63.999996, 0.3))


@pytest.mark.parametrize("pair", SIGMA_PAIRS, ids=[f"{a!r}-{b!r}" for a, b in SIGMA_PAIRS])
def test_the_sigma_of_every_code_is_the_models(lib, pair):
    s0, s1 = np.float32(pair[0]), np.float32(pair[1])
    other = (np.float32(pair[1]), np.float32(pair[0]))
    how = how_of((float(s0), float(s1)), (float(other[0]), float(other[1])))
    sx, sy = C.c_float(), C.c_float()
    for u in range(256):
        assert lib.crh_variable_blur_sigma(C.byref(how), u, C.byref(sx), C.byref(sy)) == OK
        assert bits(sx.value) == bits(M.sigma_of(s0, s1, u)) and bits(sy.value) == bits(M.sigma_of(other[0], other[1], u)), u
        assert variable_blur_sigma(u, (float(s1), float(other[1])), (float(s0), float(other[0]))) == (sx.value, sy.value)
    assert lib.crh_variable_blur_sigma(C.byref(how), 0, C.byref(sx), C.byref(sy)) == OK and bits(sx.value) == bits(s0) and bits(sy.value) == bits(s1)
    assert lib.crh_variable_blur_sigma(C.byref(how), 255, C.byref(sx), C.byref(sy)) == OK and bits(sx.value) == bits(s1) and bits(sy.value) == bits(s0)


@pytest.mark.parametrize("size", M.SIZES, ids=[f"{w}x{h}" for w, h in M.SIZES])
def test_the_host_rule_equals_the_model_at_every_size_and_edge(lib, size):
    for case in M.size_cases(*size):
        text = M.first_mismatch(host(case), M.expected(*case), M.mask(case[0], *size)[..., case[5]])
        assert text is None, (case, text)


@pytest.mark.parametrize("kind", M.MASKS)
@pytest.mark.parametrize("size", M.LARGE, ids=[f"{w}x{h}" for w, h in M.LARGE])
def test_the_host_rule_equals_the_model_for_every_mask_and_sigma_pair(lib, size, kind):
    for case in M.mask_cases(kind, *size):
        text = M.first_mismatch(host(case), M.expected(*case), M.mask(kind, *size)[..., case[5]])
        assert text is None, (case, text)


def test_the_c_call_writes_the_same_bytes_at_any_alignment(lib):
    w, h = 40, 1
    src, mask = M.source(w, h), M.mask("noise", w, h)
    raw = [(C.c_uint8 * (w * h * 4 + 1))() for _ in range(3)]
    for buffer, pixels in zip(raw, (src, mask)):
        C.memmove(C.addressof(buffer) + 1, pixels.ctypes.data, w * h * 4)
    how = how_of((0.0, 64.0), (64.0, 0.0), 0, 3)
    assert lib.crh_variable_blur_texels(w, h, C.addressof(raw[0]) + 1, C.addressof(raw[1]) + 1, C.byref(how), C.addressof(raw[2]) + 1) == OK
    assert bytes(raw[2])[1:] == M.variable_blur(src, mask, (0.0, 64.0), (64.0, 0.0), 0, M.REFLECT).tobytes()


def test_consequence_1_a_mask_of_one_value_gives_the_blur(lib):
    w, h = 37, 21
    src = M.source(w, h)
    for u in (0, 1, 128, 255):
        mask = np.random.RandomState(u).randint(0, 256, (h, w, 4)).astype(np.uint8)
        mask[..., 2] = u
        sx, sy = M.sigma_of(1.5, 40.0, u), M.sigma_of(40.0, 1.5, u)
        for edge in B.EDGES:
            want = B.blur_sigma(src, sx, sy, edge)
            if edge == B.TRANSPARENT:
                rx, ry = B.radius_of(sx), B.radius_of(sy)
                want = want[ry:ry + h, rx:rx + w]
            assert np.array_equal(variable_blur_texels(src, mask, (40.0, 1.5), (1.5, 40.0), Channel.B, BlurEdge(edge)), want), (u, edge)


def test_consequence_2_a_level_of_sigma_0_comes_back_exactly(lib):
    w, h = 37, 21
    src, checker = M.source(w, h), M.mask("checker", w, h)
    sharp = checker[..., 3] == 0
    for edge in BlurEdge:
        got = variable_blur_texels(src, checker, 64.0, 0.0, Channel.A, edge)
        assert np.array_equal(got[sharp], src[sharp]) and not np.array_equal(got[~sharp], src[~sharp]), edge
        got = variable_blur_texels(src, checker, 0.0, 64.0, Channel.A, edge)  # the descending ramp: code 255 is the sharp one
        assert np.array_equal(got[~sharp], src[~sharp]), edge


def test_consequence_3_a_constant_image_comes_back_exactly(lib):
    w, h = 37, 21
    flat = np.empty((h, w, 4), dtype=np.uint8)
    flat[:] = (30, 200, 7, 201)
    for edge in (BlurEdge.Pad, BlurEdge.Repeat, BlurEdge.Reflect):
        assert np.array_equal(variable_blur_texels(flat, M.mask("noise", w, h), (64.0, 9.0), (0.3, 64.0), Channel.R, edge), flat), edge
    assert not np.array_equal(variable_blur_texels(flat, M.mask("noise", w, h), 9.0, 0.3, Channel.R, BlurEdge.Transparent), flat)  # (it fades at the rim)


def test_consequence_4_premultiplied_stays_premultiplied(lib):
    w, h = 37, 21
    src = M.source(w, h)
    assert (src[..., :3] <= src[..., 3:]).all()
    for edge in BlurEdge:
        for kind in ("noise", "checker", "ramp_x"):
            got = variable_blur_texels(src, M.mask(kind, w, h), (13.0, 64.0), (2.0, 0.0), Channel.R, edge)
            assert (got[..., :3] <= got[..., 3:]).all(), (edge, kind)


def test_consequence_5_the_order_of_the_two_sigmas_is_only_the_formulas(lib):
    """A descending ramp over the inverted mask is the ascending one wherever the two formulas give one float: at the codes 0 and 255
    always, and at every code of a pair whose levels the test has compared first."""
    w, h = 37, 21
    src, checker = M.source(w, h), M.mask("checker", w, h)
    for edge in BlurEdge:
        assert np.array_equal(variable_blur_texels(src, checker, (7.0, 0.4), (0.0, 20.0), Channel.A, edge),
                              variable_blur_texels(src, 255 - checker, (0.0, 20.0), (7.0, 0.4), Channel.A, edge)), edge
    same = np.array([u for u in range(256) if bits(M.sigma_of(0.0, 8.0, u)) == bits(M.sigma_of(8.0, 0.0, 255 - u))], dtype=np.uint8)
    assert len(same) > 16
    noise = np.repeat(same[np.random.RandomState(5).randint(0, len(same), (h, w))][..., None], 4, axis=2)
    assert np.array_equal(variable_blur_texels(src, noise, 8.0, 0.0, Channel.R), variable_blur_texels(src, 255 - noise, 0.0, 8.0, Channel.R))


def test_the_refusals(lib):
    out = C.c_void_p(0x1234)
    texels, mask, result = (C.c_uint8 * 64)(), (C.c_uint8 * 64)(), (C.c_uint8 * 64)(*([0xAB] * 64))
    IN, MASK, TO = C.addressof(texels), C.addressof(mask), C.addressof(result)
    sx, sy = C.c_float(-1.0), C.c_float(-2.0)
    good = how_of()
    # fake image heads, never followed: every call below returns before it looks at the texels or at the renderer behind 0x10 and 0x20
    heads = [ImageHead(0x10, 5, 3), ImageHead(0x10, 5, 3), ImageHead(0x10, 5, 4), ImageHead(0x20, 5, 3), ImageHead(0x20, 4, 3), ImageHead(0, 5, 3)]
    src, same, small, foreign, foreign_small, no_renderer = (C.addressof(head) for head in heads)

    def refused(status, code, text):
        assert status == code, (status, text)
        if text is not None:
            assert lib.crh_last_error().decode() == PREFIX + text
        assert out.value == 0x1234 and bytes(result) == b"\xAB" * 64 and (sx.value, sy.value) == (-1.0, -2.0)

    # 1: a null argument
    refused(lib.crh_variable_blur_validate(None), INVALID, "a null argument")
    for arguments in ((None, 3, C.byref(sx), C.byref(sy)), (C.byref(good), 3, None, C.byref(sy)), (C.byref(good), 3, C.byref(sx), None)):
        refused(lib.crh_variable_blur_sigma(*arguments), INVALID, "a null argument")
    for arguments in ((2, 2, None, MASK, C.byref(good), TO), (2, 2, IN, None, C.byref(good), TO), (2, 2, IN, MASK, None, TO), (2, 2, IN, MASK, C.byref(good), None)):
        refused(lib.crh_variable_blur_texels(*arguments), INVALID, "a null argument")
    for arguments in ((None, same, C.byref(good), C.byref(out)), (src, None, C.byref(good), C.byref(out)), (src, same, None, C.byref(out)), (src, same, C.byref(good), None),
                      (no_renderer, same, C.byref(good), C.byref(out))):
        refused(lib.crh_image_variable_blur(*arguments), INVALID, "a null argument")
    # 2 to 5: the fields, by all four entry points
    nan, inf = float("nan"), float("inf")
    fields = [(how_of(sigma_x=(nan, 1.0)), NON_FINITE, "a sigma is not finite"), (how_of(sigma_y=(1.0, inf)), NON_FINITE, "a sigma is not finite"),
              (how_of(sigma_x=(-0.5, 1.0)), INVALID, "a sigma is outside [0, CRH_MAX_BLUR_SIGMA]"), (how_of(sigma_y=(1.0, 64.001)), INVALID, "a sigma is outside [0, CRH_MAX_BLUR_SIGMA]"),
              (how_of(channel=4), INVALID, "channel is above CRH_CHANNEL_A"), (how_of(edge=4), INVALID, "edge is above CRH_BLUR_EDGE_REFLECT"),
              # the order when two faults are present
              (how_of(sigma_x=(65.0, 1.0), sigma_y=(nan, 1.0)), NON_FINITE, "a sigma is not finite"), (how_of(sigma_x=(65.0, 1.0), channel=9, edge=9), INVALID, "a sigma is outside [0, CRH_MAX_BLUR_SIGMA]"),
              (how_of(channel=9, edge=9), INVALID, "channel is above CRH_CHANNEL_A")]
    for how, code, text in fields:
        refused(lib.crh_variable_blur_validate(C.byref(how)), code, text)
        refused(lib.crh_variable_blur_sigma(C.byref(how), 300, C.byref(sx), C.byref(sy)), code, text)
        refused(lib.crh_variable_blur_texels(0, 2, IN, MASK, C.byref(how), IN), code, text)
        refused(lib.crh_image_variable_blur(src, foreign_small, C.byref(how), C.byref(out)), code, text)
    assert lib.crh_variable_blur_validate(C.byref(good)) == OK
    for legal in (how_of((64.0, 0.0), (0.0, 64.0), 0, 0), how_of((0.0, 0.0), (0.0, 0.0), 3, 3)):
        assert lib.crh_variable_blur_validate(C.byref(legal)) == OK
    refused(lib.crh_variable_blur_sigma(C.byref(good), 256, C.byref(sx), C.byref(sy)), INVALID, "a code is above 255")
    # the sizes, then an output that is an input
    for w, h in ((0, 2), (2, 0), (16385, 1), (1, 16385)):
        refused(lib.crh_variable_blur_texels(w, h, IN, MASK, C.byref(good), IN), INVALID, "width and height lie in [1, 16384]")
    refused(lib.crh_variable_blur_texels(2, 2, TO, MASK, C.byref(good), TO), INVALID, "out_rgba8 is rgba8 or mask_rgba8")
    refused(lib.crh_variable_blur_texels(2, 2, IN, TO, C.byref(good), TO), INVALID, "out_rgba8 is rgba8 or mask_rgba8")
    assert lib.crh_variable_blur_texels(2, 2, IN, IN, C.byref(good), MASK) == OK  # (the mask may be the source)
    # 6: the images, the size before the renderer
    refused(lib.crh_image_variable_blur(src, small, C.byref(good), C.byref(out)), INVALID, "the mask is of another size")
    refused(lib.crh_image_variable_blur(src, foreign_small, C.byref(good), C.byref(out)), INVALID, "the mask is of another size")
    refused(lib.crh_image_variable_blur(src, foreign, C.byref(good), C.byref(out)), INVALID, "the images belong to different renderers")
    # the Python mirror
    pixels = np.zeros((2, 2, 4), dtype=np.uint8)
    for bad in (dict(sigma=65.0), dict(sigma=1.0, sigma_at_zero=-1.0), dict(sigma=(1.0, nan)), dict(sigma=1.0, channel=4), dict(sigma=1.0, edge=7)):
        with pytest.raises(ContrastError):
            variable_blur_texels(pixels, pixels, **bad)
    with pytest.raises(ContrastError):
        variable_blur_texels(pixels, np.zeros((2, 3, 4), dtype=np.uint8), 1.0)
    with pytest.raises(ContrastError):
        variable_blur_sigma(256, 1.0)


def test_the_cpp_mirror_compiles_links_and_agrees():
    """tests/cpp/variable_blur_harness.cpp against the C ABI: variable_blur_texels and variable_blur_sigma of the C++ mirror on images
    this test writes, compared with the model; its device side is only compiled."""
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    w, h = 19, 7
    src, mask = M.source(w, h), M.mask("noise", w, h)
    with tempfile.TemporaryDirectory() as tmp:
        binary, texels = os.path.join(tmp, "variable_blur_harness"), os.path.join(tmp, "texels.bin")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "variable_blur_harness.cpp"),
               "-o", binary, "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        with open(texels, "wb") as f:
            f.write(src.tobytes() + mask.tobytes())
        done = subprocess.run([binary, texels, str(w), str(h)], capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr)
    lines = done.stdout.splitlines()
    assert len(lines) == 5
    for line, edge in zip(lines, B.EDGES):
        assert line == M.variable_blur(src, mask, (0.0, 2.5), (4.0, 0.0), 0, edge).tobytes().hex(), edge
    assert [np.float32(v) for v in lines[4].split()] == [M.sigma_of(0.0, 2.5, 100), M.sigma_of(4.0, 0.0, 100)]


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """A stand-alone program (its own main, no library, nothing loaded into python) around csrc/variable_blur.hpp, the rule that
    crh_variable_blur_texels runs: compiled as host code with the two sanitizers (the flag goes to the host compilation alone) and run
    once. It runs one-texel axes under each edge at radius 192 and noise masks in heap buffers sized exactly."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        binary = os.path.join(tmp, "variable_blur_sanitize")
        # -x c++ and -Xarch_host: plain host C++, the sanitizers on the host alone (no device pass; clang links the sanitizers' runtime statically, so the program needs nothing preloaded)
        cmd = [hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
               "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), "-I", os.path.join(ROOT, "contrast_renderer_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "variable_blur_sanitize.cpp"), "-o", binary]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert re.search(r"\d+ texels, 0 failures$", done.stdout.strip())
