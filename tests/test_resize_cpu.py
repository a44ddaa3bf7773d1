"""crh_image_resize without a GPU (include/contrast_hip.h states the rule): crh_resize_taps against the taps of tests/resize_model.py,
integer for integer; crh_resize_texels and the Python mirror byte for byte against the model, on inputs the model's counters show to
reach both clamps of both passes and the min(v, alpha) stage; every stated consequence and refusal; the mirrors; and the rule as a
stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import ContrastError, ResizeFilter, _ffi, resize_taps, resize_texels

import resize_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_resize_taps", "crh_resize_texels", "crh_image_resize")
PREFIX = "crh_resize_taps: "
INVALID, UNSUPPORTED = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED
EDGE_PAIRS = ((16384, 33), (33, 16384), (16384, 16384), (1, 16384), (16384, 1))
# 16384 texels go to no fewer outputs than these (the window of the output in the middle just holds 512 texels), and to one fewer not
LEAST = {M.BOX: 33, M.TRIANGLE: 65, M.CATMULL_ROM: 129, M.MITCHELL: 129, M.LANCZOS3: 193}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def check_axis(n, m, filter):
    """crh_resize_taps against the model, and what the rule promises of the taps; -> the largest window, or None where both refuse"""
    try:
        first, count, taps = M.axis_taps(n, m, filter)
    except M.Unsupported:
        with pytest.raises(ContrastError) as refused:
            resize_taps(n, m, ResizeFilter(filter))
        assert refused.value.status == UNSUPPORTED, (n, m, filter)
        return None
    got_first, got_count, got_taps = resize_taps(n, m, ResizeFilter(filter))
    assert got_first.dtype == np.int32 and got_count.dtype == np.uint16 and got_taps.dtype == np.int16
    assert got_first.tolist() == first and got_count.tolist() == count and got_taps.tolist() == [q for window in taps for q in window], (n, m, M.NAMES[filter])
    for lo, k, q in zip(first, count, taps):
        assert sum(q) == M.ONE and sum(abs(v) for v in q) <= M.MAX_GAIN and 0 <= lo and 1 <= k <= M.MAX_TAPS and lo + k <= n, (n, m, M.NAMES[filter])
    return max(count)


@pytest.mark.parametrize("filter", M.FILTERS, ids=list(M.NAMES.values()))
def test_taps_of_every_small_pair(filter, lib):
    for n, m in itertools.product(range(1, 25), range(1, 25)):
        assert check_axis(n, m, filter) is not None


@pytest.mark.parametrize("filter", M.FILTERS, ids=list(M.NAMES.values()))
def test_taps_of_the_longest_axes_and_round_the_cap(filter, lib):
    served = {pair: check_axis(pair[0], pair[1], filter) for pair in EDGE_PAIRS}
    assert served[(33, 16384)] and served[(16384, 16384)] and served[(1, 16384)] == 1
    assert served[(16384, 1)] is None and (served[(16384, 33)] is not None) == (filter == M.BOX)
    # just under and just over 512 taps: 16384 / 33 = 496.5 (box) .. 16384 / 193 = 84.9 (Lanczos3) are the largest ratios of a call
    least = LEAST[filter]
    assert M.max_count(16384, least, filter) <= 512 < M.max_count(16384, least - 1, filter)
    assert check_axis(16384, least, filter) >= 498 and check_axis(16384, least - 1, filter) is None
    total = C.c_uint64(77)
    assert lib.crh_resize_taps(16384, least - 1, filter, None, None, None, 0, C.byref(total)) == UNSUPPORTED and total.value == 77
    assert lib.crh_last_error().decode() == PREFIX + "an output's window exceeds CRH_MAX_RESIZE_TAPS texels: chain two calls"
    # a window of exactly 512 texels: 512 source texels into one output, the whole source
    assert check_axis(512, 1, filter) == 512 and check_axis(513, 1, filter) is None


def test_the_worst_gain_the_issue_names(lib):
    first, count, taps = M.axis_taps(4, 5, M.LANCZOS3)
    assert sum(abs(q) for q in taps[2]) == 25748
    assert max(sum(abs(q) for q in window) for f in M.FILTERS for n in range(1, 25) for m in range(1, 25) for window in M.axis_taps(n, m, f)[2]) == 25748


SIZES = [((1, 1), (1, 1)), ((1, 1), (9, 7)), ((9, 7), (1, 1)), ((24, 5), (7, 24)), ((7, 23), (23, 3)), ((64, 3), (63, 5)), ((129, 2), (31, 2)), ((33, 2), (300, 1))]


@pytest.mark.parametrize("filter", M.FILTERS, ids=list(M.NAMES.values()))
def test_texels_byte_for_byte(filter, lib):
    rng = np.random.default_rng(filter)
    for (w, h), (out_w, out_h) in SIZES:
        for make in (M.premultiplied, M.saturated):
            src = make(rng, h, w)
            expect = M.resize(src, out_w, out_h, filter)
            got = resize_texels(src, out_w, out_h, ResizeFilter(filter))
            assert got.shape == expect.shape and np.array_equal(got, expect), ((w, h), (out_w, out_h), make.__name__)
            assert (got[..., :3] <= got[..., 3:]).all()  # rgb <= a always holds
    wide = M.premultiplied(rng, 1, 16384)
    least = LEAST[filter]
    assert np.array_equal(resize_texels(wide, least, 1, ResizeFilter(filter)), M.resize(wide, least, 1, filter))
    tall = np.ascontiguousarray(wide.transpose(1, 0, 2))
    assert np.array_equal(resize_texels(tall, 1, least, ResizeFilter(filter)), M.resize(tall, 1, least, filter))
    assert np.array_equal(resize_texels(src, 5, 3), M.resize(src, 5, 3, M.LANCZOS3))  # the default filter


def test_the_checker_binds_every_clamp_and_min_alpha_has_work(lib):
    """8 x 5 to 21 x 13: the model's counters show both clamps of both passes binding under the three filters with negative lobes, and
    none under BOX and TRIANGLE; a random 11 x 6 image to 5 x 4 has colours that only min(v, alpha) keeps below their alpha."""
    src = M.checker(5, 8)
    for filter in M.FILTERS:
        counters = {}
        expect = M.resize(src, 21, 13, filter, counters)
        clamps = [counters[k] for k in ("h_low", "h_high", "v_low", "v_high")]
        assert all(clamps) if filter in (M.CATMULL_ROM, M.MITCHELL, M.LANCZOS3) else not any(clamps), (M.NAMES[filter], counters)
        assert np.array_equal(resize_texels(src, 21, 13, ResizeFilter(filter)), expect)
    src = M.premultiplied(np.random.default_rng(2), 6, 11)
    for filter in (M.CATMULL_ROM, M.LANCZOS3):
        counters = {}
        expect = M.resize(src, 5, 4, filter, counters)
        assert counters["min_alpha"] > 0, (M.NAMES[filter], counters)
        assert np.array_equal(resize_texels(src, 5, 4, ResizeFilter(filter)), expect)


def test_no_clamp_binds_under_box_and_triangle(lib):
    rng = np.random.default_rng(5)
    for filter, ((w, h), (out_w, out_h)) in itertools.product((M.BOX, M.TRIANGLE), SIZES):
        counters = {}
        M.resize(rng.integers(0, 256, (h, w, 4), dtype=np.uint8) | np.uint8(0xF0), out_w, out_h, filter, counters)
        assert not any(counters[k] for k in ("h_low", "h_high", "v_low", "v_high")), (M.NAMES[filter], counters)
        for window in M.axis_taps(w, out_w, filter)[2]:
            assert min(window) >= 0


@pytest.mark.parametrize("filter", M.FILTERS, ids=list(M.NAMES.values()))
def test_constants_come_back_exactly(filter, lib):
    for texel, ((w, h), (out_w, out_h)) in itertools.product(((0, 0, 0, 0), (255, 255, 255, 255), (1, 0, 77, 78), (200, 13, 254, 254)), SIZES):
        flat = np.full((h, w, 4), texel, dtype=np.uint8)
        assert (resize_texels(flat, out_w, out_h, ResizeFilter(filter)) == np.array(texel, dtype=np.uint8)).all(), (texel, (w, h), (out_w, out_h))


def test_the_same_size_is_a_copy_except_under_mitchell(lib):
    rng = np.random.default_rng(6)
    for w, h in ((1, 1), (2, 7), (31, 9), (64, 3)):
        src = M.premultiplied(rng, h, w)
        for filter in M.FILTERS:
            same = np.array_equal(resize_texels(src, w, h, ResizeFilter(filter)), src)
            assert same == (filter != M.MITCHELL or (w, h) == (1, 1)), (w, h, M.NAMES[filter])
    # Mitchell is not interpolating: 1/18, 8/9, 1/18 inside the image, renormalised over what is left at its ends
    first, count, taps = resize_taps(9, 9, ResizeFilter.Mitchell)
    assert count.tolist() == [3, 4, 5, 5, 5, 5, 5, 4, 3] and first.tolist() == [0, 0, 0, 1, 2, 3, 4, 5, 6]
    assert taps[7:12].tolist() == [0, 910, 14564, 910, 0] and taps[:3].tolist() == M.axis_taps(9, 9, M.MITCHELL)[2][0] and taps[1] > 0
    for filter in (M.BOX, M.TRIANGLE, M.CATMULL_ROM, M.LANCZOS3):
        first, count, taps = M.axis_taps(9, 9, filter)
        assert all(window[o - lo] == M.ONE and sum(abs(q) for q in window) == M.ONE for o, (lo, window) in enumerate(zip(first, taps))), M.NAMES[filter]


def test_box_at_an_integer_ratio_is_the_area_mean(lib):
    rng = np.random.default_rng(8)
    for (kx, ky), (out_w, out_h) in (((2, 2), (9, 5)), ((3, 1), (7, 4)), ((5, 7), (3, 3)), ((16, 16), (2, 2)), ((255, 1), (2, 1))):
        src = rng.integers(0, 256, (out_h * ky, out_w * kx, 4), dtype=np.uint8)
        src[..., 3] = 255  # (opaque: min(v, alpha) is out of the way)
        got = resize_texels(src, out_w, out_h, ResizeFilter.Box).astype(np.float64)
        mean = src.astype(np.float64).reshape(out_h, ky, out_w, kx, 4).mean(axis=(1, 3))
        assert np.abs(got - mean).max() <= 0.51, ((kx, ky), np.abs(got - mean).max())


class ImageHead(C.Structure):
    """What a crh_image starts with: its renderer and its size. Enough for the calls below, which refuse before they look at the texels or
    at the renderer behind the pointer (0x10 is never followed)."""
    _fields_ = [("renderer", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("pixels", C.c_void_p * 2)]


def test_refusals_statuses_texts_and_untouched_outputs(lib):
    a_size, a_side, a_filter = "width and height lie in [1, 16384]", "a side lies outside [1, 16384]", "filter is above CRH_RESIZE_LANCZOS3"
    null, capacity, taps_cap = "a null argument", "capacity is below the total", "an output's window exceeds CRH_MAX_RESIZE_TAPS texels: chain two calls"
    src = M.premultiplied(np.random.default_rng(9), 3, 5)
    out = np.full((16, 16, 4), 0xA5, dtype=np.uint8)
    first, count, taps = np.full(8, 77, dtype=np.int32), np.full(8, 77, dtype=np.uint16), np.full(64, 77, dtype=np.int16)
    total, handle = C.c_uint64(77), C.c_void_p(0x1234)
    heads = [ImageHead(0x10, 5, 3), ImageHead(0x10, 16384, 2), ImageHead(None, 5, 3), ImageHead(0x10, 0, 3)]
    fake, wide, unowned, flat = (C.addressof(head) for head in heads)
    pf, pc, pt = first.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_uint16)), taps.ctypes.data_as(C.POINTER(C.c_int16))

    def untouched():
        return (out == 0xA5).all() and (first == 77).all() and (count == 77).all() and (taps == 77).all() and (total.value, handle.value) == (77, 0x1234)

    def refused(call, status, text):
        assert lib.crh_blur_taps(-1.0, None, 0, None) == INVALID  # some other text first
        assert call() == status and lib.crh_last_error().decode() == PREFIX + text and untouched(), text

    for call in (lambda: lib.crh_resize_taps(5, 8, 4, None, None, None, 0, None), lambda: lib.crh_resize_taps(5, 8, 4, pf, None, pt, 64, C.byref(total)),
                 lambda: lib.crh_resize_taps(5, 8, 4, None, pc, None, 64, C.byref(total)), lambda: lib.crh_resize_taps(0, 8, 9, pf, pc, None, 64, C.byref(total)),
                 lambda: lib.crh_resize_texels(5, 3, None, 4, 4, 4, out.ctypes.data), lambda: lib.crh_resize_texels(5, 3, src.ctypes.data, 4, 4, 4, None),
                 lambda: lib.crh_resize_texels(0, 3, None, 4, 4, 9, out.ctypes.data),  # a null beside a bad size and filter: the null is named
                 lambda: lib.crh_image_resize(None, 4, 4, 4, C.byref(handle)), lambda: lib.crh_image_resize(fake, 4, 4, 4, None),
                 lambda: lib.crh_image_resize(unowned, 4, 4, 4, C.byref(handle)), lambda: lib.crh_image_resize(None, 0, 0, 9, None)):
        refused(call, INVALID, null)
    for n, m in ((0, 8), (5, 0), (16385, 8), (5, 16385)):
        refused(lambda: lib.crh_resize_taps(n, m, 4, pf, pc, pt, 64, C.byref(total)), INVALID, a_side)
        refused(lambda: lib.crh_resize_taps(n, m, 9, None, None, None, 0, C.byref(total)), INVALID, a_side)  # the side before the filter
    for width, height in ((0, 3), (5, 0), (16385, 3), (5, 16385)):
        refused(lambda: lib.crh_resize_texels(width, height, src.ctypes.data, 4, 4, 4, out.ctypes.data), INVALID, a_size)
        refused(lambda: lib.crh_resize_texels(5, 3, src.ctypes.data, width, height, 9, out.ctypes.data), INVALID, a_size)
        refused(lambda: lib.crh_image_resize(fake, width, height, 9, C.byref(handle)), INVALID, a_size)
    refused(lambda: lib.crh_image_resize(flat, 4, 4, 4, C.byref(handle)), INVALID, a_size)
    for filter in (5, 6, 0xFFFFFFFF):
        refused(lambda: lib.crh_resize_taps(5, 8, filter, pf, pc, pt, 64, C.byref(total)), INVALID, a_filter)
        refused(lambda: lib.crh_resize_texels(5, 3, src.ctypes.data, 4, 4, filter, out.ctypes.data), INVALID, a_filter)
        refused(lambda: lib.crh_image_resize(fake, 4, 4, filter, C.byref(handle)), INVALID, a_filter)
        refused(lambda: lib.crh_image_resize(wide, 1, 1, filter, C.byref(handle)), INVALID, a_filter)  # the filter before the cap
    before = src.copy()
    assert lib.crh_resize_texels(5, 3, src.ctypes.data, 5, 3, 4, src.ctypes.data) == INVALID and lib.crh_last_error().decode() == PREFIX + "out_rgba8 is rgba8"
    assert np.array_equal(src, before)
    # the capacity: the total of 5 -> 8 under Lanczos3 is what the model says, one less is refused, and the arrays stay as they were
    needed = sum(M.axis_taps(5, 8, M.LANCZOS3)[1])
    refused(lambda: lib.crh_resize_taps(5, 8, 4, pf, pc, pt, needed - 1, C.byref(total)), INVALID, capacity)
    assert lib.crh_resize_taps(5, 8, 4, None, None, None, 0, C.byref(total)) == 0 and total.value == needed and (first == 77).all()
    total.value = 77
    assert lib.crh_resize_taps(5, 8, 4, pf, pc, pt, needed, None) == 0 and (taps[needed:] == 77).all() and first[0] == 0
    first[:], count[:], taps[:] = 77, 77, 77
    # the cap: CRH_ERR_UNSUPPORTED, on either axis, from every entry point
    refused(lambda: lib.crh_resize_taps(16384, 2, 4, pf, pc, pt, 64, C.byref(total)), UNSUPPORTED, taps_cap)
    refused(lambda: lib.crh_image_resize(wide, 2, 2, 4, C.byref(handle)), UNSUPPORTED, taps_cap)
    refused(lambda: lib.crh_image_resize(wide, 32, 2, 0, C.byref(handle)), UNSUPPORTED, taps_cap)
    long_row, long_column = np.zeros((1, 700, 4), dtype=np.uint8), np.zeros((700, 1, 4), dtype=np.uint8)
    refused(lambda: lib.crh_resize_texels(700, 1, long_row.ctypes.data, 1, 1, 0, out.ctypes.data), UNSUPPORTED, taps_cap)
    refused(lambda: lib.crh_resize_texels(1, 700, long_column.ctypes.data, 1, 1, 1, out.ctypes.data), UNSUPPORTED, taps_cap)
    for call in (lambda: resize_taps(16384, 2), lambda: resize_texels(long_row, 1, 1), lambda: resize_texels(src, 0, 4), lambda: resize_texels(src, 4, 16385),
                 lambda: resize_taps(5, 8, 7), lambda: resize_texels(src[..., :3], 4, 4), lambda: resize_texels(src.astype(np.float32), 4, 4)):
        with pytest.raises(ContrastError):
            call()


def test_unaligned_bytes(lib):
    src = M.saturated(np.random.default_rng(10), 3, 7)
    raw_in = np.full(7 * 3 * 4 + 3, 0xA5, dtype=np.uint8)
    raw_in[1:-2] = src.reshape(-1)
    for filter in M.FILTERS:
        expect = M.resize(src, 5, 4, filter)
        raw_out = np.full(expect.size + 3, 0xA5, dtype=np.uint8)
        assert lib.crh_resize_texels(7, 3, raw_in.ctypes.data + 1, 5, 4, filter, raw_out.ctypes.data + 2) == 0
        assert np.array_equal(raw_out[2:-1].reshape(expect.shape), expect) and (raw_out[:2] == 0xA5).all() and raw_out[-1] == 0xA5


def test_the_library_exports_and_the_mirrors_agree_across_header_python_and_ffi_rs(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    from contrast_renderer_amd import build as b
    assert set(NAMES) <= set(b.declared_entry_points())
    exports = open(b.write_export_map()).read()
    for name in NAMES:
        assert f"    {name};\n" in exports
    assert any(os.path.basename(h) == "resize.hpp" for h in b.header_deps())
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    assert "CRH_RESIZE_BOX = 0, CRH_RESIZE_TRIANGLE = 1, CRH_RESIZE_CATMULL_ROM = 2, CRH_RESIZE_MITCHELL = 3, CRH_RESIZE_LANCZOS3 = 4" in header and "#define CRH_MAX_RESIZE_TAPS 512u" in header
    committed = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_ffi
        fresh = gen_rust_ffi.generate()
    finally:
        sys.path.pop(0)
    assert committed == fresh
    for text in ("pub fn crh_resize_taps(n: u32, m: u32, filter: u32, first: *mut i32, count: *mut u16, taps: *mut i16, capacity: u64, total: *mut u64) -> crh_status;",
                 "pub fn crh_resize_texels(width: u32, height: u32, rgba8: *const c_void, out_width: u32, out_height: u32, filter: u32, out_rgba8: *mut c_void) -> crh_status;",
                 "pub fn crh_image_resize(src: *const crh_image, width: u32, height: u32, filter: u32, out: *mut *mut crh_image) -> crh_status;",
                 "pub const CRH_RESIZE_LANCZOS3: u32 = 4;", "pub const CRH_MAX_RESIZE_TAPS: usize = 512;"):
        assert text in committed, text
    shim = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    for text in ("pub enum ResizeFilter {", "pub fn resize_taps(n: u32, m: u32, filter: ResizeFilter) -> Result<(Vec<i32>, Vec<u16>, Vec<i16>), Error>",
                 "pub fn resize_texels(width: u32, height: u32, texels: &[u8], out_width: u32, out_height: u32, filter: ResizeFilter) -> Result<Vec<u8>, Error>",
                 "pub fn resize(&self, width: u32, height: u32, filter: ResizeFilter) -> Result<Image, Error>"):
        assert text in shim, text
    for name in NAMES:
        assert f"ffi::{name}(" in shim, name
    mirror = open(os.path.join(ROOT, "include", "contrast_renderer.hpp")).read()
    for text in ("enum class ResizeFilter : uint32_t {", "struct ResizeTaps {", "Image resize(uint32_t width, uint32_t height, ResizeFilter filter = ResizeFilter::Lanczos3) const",
                 "inline std::vector<uint8_t> resize_texels(uint32_t width, uint32_t height,", "inline ResizeTaps resize_taps(uint32_t n, uint32_t m, ResizeFilter filter = ResizeFilter::Lanczos3)"):
        assert text in mirror, text
    import contrast_renderer_amd
    for name in ("ResizeFilter", "resize_taps", "resize_texels"):
        assert name in contrast_renderer_amd.__all__ and hasattr(contrast_renderer_amd, name)
    assert hasattr(contrast_renderer_amd.Image, "resize")
    assert [f.value for f in ResizeFilter] == list(M.FILTERS)


def test_the_cpp_mirror_of_resize_compiles_against_the_c_abi(lib):
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "resize_harness.cpp"),
               "-o", os.path.join(tmp, "resize_harness"), "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """A stand-alone program (its own main, no library, nothing loaded into python) around csrc/resize.hpp, the rule that crh_resize_taps
    and crh_resize_texels run: compiled as host code with the two sanitizers (the flag goes to the host compilation alone) and run once.
    It builds the taps over the edge sizes and round the cap and resizes images in heap buffers sized exactly."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        binary = os.path.join(tmp, "resize_sanitize")
        # -x c++ and -Xarch_host: plain host C++, the sanitizers on the host alone (no device pass; clang links the sanitizers' runtime statically, so the program needs nothing preloaded)
        cmd = [hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
               "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), "-I", os.path.join(ROOT, "contrast_renderer_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "resize_sanitize.cpp"), "-o", binary]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert re.search(r"\d+ texels, 0 failures$", done.stdout.strip())
