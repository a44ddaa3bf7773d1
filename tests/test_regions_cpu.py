"""crh_crop_texels and crh_statistics_texels (include/contrast_hip.h, "Regions and statistics") without a device: every byte and every
counter against the numpy model of tests/regions_model.py, the properties the header states, the refusals as a literal table — status,
exact crh_last_error text, which of two faults is named, nothing written — and the mirrors: struct and enum layouts, the exported
symbols, the Python wrappers, a C++ harness."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import Channel, ContrastError, ImageStatistics, _ffi, crop_texels, statistics_texels
from contrast_renderer_amd import renderer as R

import regions_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, INVALID = _ffi.OK, _ffi.ERR_UNSUPPORTED, _ffi.ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def check_statistics(src, channel, threshold, what=None):
    got = statistics_texels(src, channel, threshold)
    histogram, bounds, count = M.statistics(src, channel, threshold)
    assert isinstance(got, ImageStatistics) and got.histogram.shape == (4, 256) and got.histogram.dtype == np.uint32
    assert (got.histogram == histogram).all() and got.bounds == bounds and got.count == count, (what, channel, threshold, got.bounds, bounds, got.count, count)
    return got


# ---- crop

@pytest.mark.parametrize("premultiplied", (True, False))
@pytest.mark.parametrize("size", ((13, 7), (1, 1), (4, 9), (32, 2)))
def test_crop_rectangles_of_every_class_against_the_model(lib, size, premultiplied):
    """Inside, over each side and corner, containing the source, missing it on each side, x and y at INT32_MIN and INT32_MAX; the bytes
    as stored, so colours above their alpha come through as they are."""
    w, h = size
    src = M.random_texels(w, h, 11 * w + h, premultiplied)
    for name, x, y, width, height in M.rectangles(w, h):
        got = crop_texels(src, x, y, width, height)
        assert got.shape == (height, width, 4) and (got == M.crop(src, x, y, width, height)).all(), (name, x, y, width, height)


def test_a_crop_that_misses_the_source_is_transparent_and_one_that_contains_it_is_a_backdrop(lib):
    src = M.random_texels(5, 4, 3)
    assert not crop_texels(src, 5, 0, 6, 6).any() and not crop_texels(src, -3, -3, 3, 3).any()
    big = crop_texels(src, -2, -1, 9, 7)
    assert (big[1:5, 2:7] == src).all() and int(big.astype(np.int64).sum()) == int(src.astype(np.int64).sum())


def test_crop_of_a_crop_composes(lib):
    src = M.random_texels(23, 17, 5)
    first = crop_texels(src, -4, 3, 30, 12)
    for a, b, w, h in ((0, 0, 30, 12), (5, 2, 11, 7), (29, 11, 1, 1), (2, 0, 28, 3)):  # rectangles inside the first result
        assert (crop_texels(first, a, b, w, h) == crop_texels(src, -4 + a, 3 + b, w, h)).all(), (a, b, w, h)


def test_crop_takes_the_largest_sizes(lib):
    src = np.zeros((1, 16384, 4), dtype=np.uint8)
    src[0, 16383] = (1, 2, 3, 4)
    assert tuple(crop_texels(src, 16383, 0, 1, 1)[0, 0]) == (1, 2, 3, 4)
    tall = crop_texels(src, 16380, -16383, 4, 16384)
    assert tuple(tall[16383, 3]) == (1, 2, 3, 4) and int(tall.astype(np.int64).sum()) == 10


# ---- statistics

@pytest.mark.parametrize("premultiplied", (True, False))
def test_statistics_of_random_images_in_every_channel_and_threshold(lib, premultiplied):
    for (w, h) in ((13, 7), (1, 1), (64, 3), (5, 40)):
        src = M.random_texels(w, h, w * 31 + h, premultiplied)
        for channel in range(4):
            for threshold in (1, 128, 255):
                check_statistics(src, channel, threshold, (w, h))


@pytest.mark.parametrize("threshold", (1, 128, 255))
def test_a_code_at_the_threshold_is_inside_and_one_below_is_not(lib, threshold):
    for channel in range(4):
        src = np.zeros((3, 4, 4), dtype=np.uint8)
        src[1, 2, channel] = threshold
        src[2, 0, channel] = threshold - 1
        got = check_statistics(src, channel, threshold)
        assert got.bounds == (2, 1, 3, 2) and got.count == 1
        other = check_statistics(src, (channel + 1) % 4, threshold)  # the other channels hold zeros: nothing is inside
        assert other.bounds == (0, 0, 0, 0) and other.count == 0


def test_single_texels_in_the_corners(lib):
    w, h = 9, 6
    corners = ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))
    for x, y in corners:
        src = np.zeros((h, w, 4), dtype=np.uint8)
        src[y, x] = (0, 0, 0, 200)
        assert check_statistics(src, M.A, 1).bounds == (x, y, x + 1, y + 1)
    for (ax, ay), (bx, by) in ((corners[0], corners[3]), (corners[1], corners[2])):  # two in opposite corners: the whole image
        src = np.zeros((h, w, 4), dtype=np.uint8)
        src[ay, ax] = src[by, bx] = (9, 9, 9, 9)
        got = check_statistics(src, M.A, 9)
        assert got.bounds == (0, 0, w, h) and got.count == 2


def test_none_inside_gives_zeros_and_all_inside_gives_the_image(lib):
    src = np.full((5, 7, 4), 100, dtype=np.uint8)
    none = check_statistics(src, M.G, 101)
    assert none.bounds == (0, 0, 0, 0) and none.count == 0 and int(none.histogram[1, 100]) == 35
    everything = check_statistics(src, M.G, 100)
    assert everything.bounds == (0, 0, 7, 5) and everything.count == 35
    empty = check_statistics(np.zeros((5, 7, 4), dtype=np.uint8), M.A, 1)
    assert empty.count == 0 and (empty.histogram[:, 0] == 35).all() and int(empty.histogram.sum()) == 4 * 35


def test_properties_of_the_histogram_the_count_and_the_bounds(lib):
    src = M.random_texels(37, 21, 8)
    src[:4] = 0
    src[:, 30:] = 0
    src[15:, :6] = 0
    for channel in range(4):
        for threshold in (1, 77, 255):
            got = check_statistics(src, channel, threshold)
            assert (got.histogram.sum(axis=1) == 37 * 21).all()
            assert got.count == int(got.histogram[channel, threshold:].sum())
            if got.count:
                x0, y0, x1, y1 = got.bounds
                cut = statistics_texels(crop_texels(src, x0, y0, x1 - x0, y1 - y0), channel, threshold)
                assert cut.bounds == (0, 0, x1 - x0, y1 - y0) and cut.count == got.count
    miss = statistics_texels(crop_texels(src, 40, 0, 6, 5), M.A, 1)  # a crop that misses the source: width * height in bin 0, no bounds
    assert (miss.histogram[:, 0] == 30).all() and miss.bounds == (0, 0, 0, 0) and miss.count == 0


# ---- refusals: the call, its arguments, the status, the exact text of crh_last_error()

class ImageHead(C.Structure):
    """What a crh_image starts with (tests/test_image_api_contract_cpu.py): the calls below refuse before they follow the renderer"""
    _fields_ = [("renderer", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("pixels", C.c_void_p * 2)]


_kept = []


def _keep(value):
    _kept.append(value)
    return value


def image(width=5, height=3, renderer=0x10):
    return C.addressof(_keep(ImageHead(renderer, width, height)))


OUT = C.pointer(_keep(C.c_void_p(0x1234)))  # a refused call leaves it as it is
TEXELS, RESULT = _keep((C.c_uint8 * 64)()), _keep((C.c_uint8 * 64)())
IN, TO = C.addressof(TEXELS), C.addressof(RESULT)
STATS = _keep(_ffi.ImageStatsC())
C.memset(C.addressof(STATS), 0xAB, C.sizeof(STATS))
TO_STATS = C.pointer(STATS)
FRAME = 0x40  # never followed: every row with it refuses before
CROP, STATISTICS = "crh_crop_texels: ", "crh_statistics_texels: "
NULL, A_SIZE, SAME = "a null argument", "width and height lie in [1, 16384]", "out_rgba8 is rgba8"
CHANNEL, THRESHOLD = "channel is above CRH_CHANNEL_A", "threshold is outside [1, 255]"

CONTRACT = [
    # ---- crh_crop_texels: null arguments, then the source's size, then the result's, then out == in
    ("crh_crop_texels", (4, 4, None, 0, 0, 2, 2, TO), INVALID, CROP + NULL),
    ("crh_crop_texels", (4, 4, IN, 0, 0, 2, 2, None), INVALID, CROP + NULL),
    ("crh_crop_texels", (0, 4, None, 0, 0, 2, 2, TO), INVALID, CROP + NULL),  # null before the size
    ("crh_crop_texels", (0, 4, IN, 0, 0, 2, 2, TO), INVALID, CROP + A_SIZE),
    ("crh_crop_texels", (4, 16385, IN, 0, 0, 2, 2, TO), INVALID, CROP + A_SIZE),
    ("crh_crop_texels", (4, 4, IN, 0, 0, 0, 2, TO), INVALID, CROP + A_SIZE),
    ("crh_crop_texels", (4, 4, IN, 0, 0, 2, 16385, TO), INVALID, CROP + A_SIZE),
    ("crh_crop_texels", (4, 4, IN, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, TO), INVALID, CROP + A_SIZE),
    ("crh_crop_texels", (4, 4, IN, 0, 0, 2, 2, IN), INVALID, CROP + SAME),
    ("crh_crop_texels", (4, 4, IN, 0, 0, 0, 2, IN), INVALID, CROP + A_SIZE),  # the size before out == in
    # ---- crh_statistics_texels: null arguments, the channel, the threshold, the size
    ("crh_statistics_texels", (4, 4, None, 3, 1, TO_STATS), INVALID, STATISTICS + NULL),
    ("crh_statistics_texels", (4, 4, IN, 3, 1, None), INVALID, STATISTICS + NULL),
    ("crh_statistics_texels", (4, 4, None, 4, 0, TO_STATS), INVALID, STATISTICS + NULL),  # null before the channel
    ("crh_statistics_texels", (4, 4, IN, 4, 1, TO_STATS), INVALID, STATISTICS + CHANNEL),
    ("crh_statistics_texels", (4, 4, IN, 0xFFFFFFFF, 1, TO_STATS), INVALID, STATISTICS + CHANNEL),
    ("crh_statistics_texels", (0, 4, IN, 4, 0, TO_STATS), INVALID, STATISTICS + CHANNEL),  # the channel before the threshold and the size
    ("crh_statistics_texels", (4, 4, IN, 3, 0, TO_STATS), INVALID, STATISTICS + THRESHOLD),
    ("crh_statistics_texels", (4, 4, IN, 3, 256, TO_STATS), INVALID, STATISTICS + THRESHOLD),
    ("crh_statistics_texels", (0, 4, IN, 3, 0, TO_STATS), INVALID, STATISTICS + THRESHOLD),  # the threshold before the size
    ("crh_statistics_texels", (0, 4, IN, 3, 1, TO_STATS), INVALID, STATISTICS + A_SIZE),
    ("crh_statistics_texels", (4, 16385, IN, 3, 1, TO_STATS), INVALID, STATISTICS + A_SIZE),
    # ---- the three device entry points: a null source, renderer, frame or out, and the checks behind them, before any HIP call
    ("crh_image_crop", (None, 0, 0, 2, 2, OUT), INVALID, CROP + NULL),
    ("crh_image_crop", (image(renderer=None), 0, 0, 2, 2, OUT), INVALID, CROP + NULL),
    ("crh_image_crop", (image(), 0, 0, 2, 2, None), INVALID, CROP + NULL),
    ("crh_image_crop", (None, 0, 0, 0, 2, OUT), INVALID, CROP + NULL),  # null before the size
    ("crh_image_crop", (image(), 0, 0, 0, 2, OUT), INVALID, CROP + A_SIZE),
    ("crh_image_crop", (image(), -5, 7, 2, 16385, OUT), INVALID, CROP + A_SIZE),
    ("crh_image_create_from_frame_region", (None, 0, 0, 2, 2, OUT), INVALID, CROP + NULL),
    ("crh_image_create_from_frame_region", (FRAME, 0, 0, 2, 2, None), INVALID, CROP + NULL),
    ("crh_image_create_from_frame_region", (None, 0, 0, 0, 2, OUT), INVALID, CROP + NULL),  # null before the size
    ("crh_image_statistics", (None, 3, 1, TO_STATS), INVALID, STATISTICS + NULL),
    ("crh_image_statistics", (image(renderer=None), 3, 1, TO_STATS), INVALID, STATISTICS + NULL),
    ("crh_image_statistics", (image(), 3, 1, None), INVALID, STATISTICS + NULL),
    ("crh_image_statistics", (None, 4, 0, TO_STATS), INVALID, STATISTICS + NULL),  # null before the channel
    ("crh_image_statistics", (image(), 4, 0, TO_STATS), INVALID, STATISTICS + CHANNEL),
    ("crh_image_statistics", (image(), 3, 0, TO_STATS), INVALID, STATISTICS + THRESHOLD),
    ("crh_image_statistics", (image(0, 3), 3, 256, TO_STATS), INVALID, STATISTICS + THRESHOLD),  # the threshold before the size
    ("crh_image_statistics", (image(0, 3), 3, 255, TO_STATS), INVALID, STATISTICS + A_SIZE),
]


@pytest.mark.parametrize("row", range(len(CONTRACT)), ids=[f"{i}-{row[0]}" for i, row in enumerate(CONTRACT)])
def test_the_call_returns_the_status_and_sets_the_text(lib, row):
    name, args, status, text = CONTRACT[row]
    assert lib.crh_turbulence_validate(None) == INVALID  # some other text first, so that the one asserted below is this call's
    before = lib.crh_last_error().decode()
    assert getattr(lib, name)(*args) == status
    assert before != text and lib.crh_last_error().decode() == text
    assert OUT.contents.value == 0x1234 and not any(RESULT) and not any(TEXELS)
    assert bytes(STATS) == b"\xAB" * 4116  # a refused call writes nothing to *out


def test_the_rows_are_valid_but_for_the_fault_they_name(lib):
    assert lib.crh_crop_texels(4, 4, IN, 0, 0, 2, 2, TO) == OK
    stats = _ffi.ImageStatsC()
    assert lib.crh_statistics_texels(4, 4, IN, 3, 1, C.byref(stats)) == OK and stats.histogram[0] == 16 and stats.count == 0


# ---- mirrors

def test_the_struct_and_the_enum_are_the_headers(lib):
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    body = re.search(r"typedef struct crh_image_stats \{(.*?)\} crh_image_stats;", header, flags=re.S).group(1)
    fields = [" ".join(field.split()) for field in re.sub(r"/\*.*?\*/", " ", body, flags=re.S).split(";")]
    assert fields[:3] == ["uint32_t histogram[1024]", "uint32_t x0, y0, x1, y1", "uint32_t count"]
    assert C.sizeof(_ffi.ImageStatsC) == 4116 and _ffi.ImageStatsC.x0.offset == 4096 and _ffi.ImageStatsC.count.offset == 4112
    assert [int(c) for c in Channel] == [int(v) for v in re.search(r"CRH_CHANNEL_R = (\d), CRH_CHANNEL_G = (\d), CRH_CHANNEL_B = (\d), CRH_CHANNEL_A = (\d)", header).groups()]
    ffi_rs = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "ffi.rs")).read()
    assert "pub histogram: [u32; 1024]," in ffi_rs
    sig = lib._crh_signatures if hasattr(lib, "_crh_signatures") else None
    if sig is not None:
        assert sig["crh_image_crop"][1][1] is C.c_int32 and sig["crh_image_statistics"][1][3] is C.POINTER(_ffi.ImageStatsC)


def test_the_library_exports_the_headers_entry_points(lib):
    from contrast_renderer_amd import build
    declared = set(build.declared_entry_points())
    new = {"crh_crop_texels", "crh_statistics_texels", "crh_image_crop", "crh_image_create_from_frame_region", "crh_image_statistics"}
    assert new <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", build.OUT], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("crh_")} == declared | set(build.DEBUG_TAPS)
    for name in new:
        assert hasattr(lib, name)


def test_the_python_wrappers_refuse_what_they_must():
    src = M.random_texels(4, 4, 2)
    for call in (lambda: crop_texels(src, 0, 0, 0, 1), lambda: crop_texels(src, 0, 0, 1, 16385), lambda: crop_texels(src, 2 ** 31, 0, 1, 1), lambda: crop_texels(src[..., :3], 0, 0, 1, 1),
                 lambda: statistics_texels(src, 4, 1), lambda: statistics_texels(src, Channel.A, 0), lambda: statistics_texels(src, Channel.A, 256), lambda: statistics_texels(src.astype(np.float32))):
        with pytest.raises(ContrastError):
            call()
    assert "can be negative" in R.Image.__doc__ and "origin[0] - x" in R.Image.crop.__doc__
    assert R.Image.trim.__doc__ and R.Image.bounds.__doc__ and R.Image.statistics.__doc__ and "region" in R.Image.from_frame.__doc__


def test_the_cpp_mirror_reproduces_recorded_cases(lib):
    """tests/cpp/regions_harness.cpp against the C ABI: crop_texels and statistics_texels of the C++ mirror on an image this test writes,
    compared with the model; its device side is only compiled."""
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    w, h = 11, 6
    src = M.random_texels(w, h, 21)
    src[:2] = 0
    src[:, 8:] = 0
    cases = [(2, 1, 5, 4), (-3, -2, 17, 9), (20, 0, 3, 3), (M.INT32_MIN, M.INT32_MAX, 2, 2)]
    with tempfile.TemporaryDirectory() as tmp:
        binary, texels = os.path.join(tmp, "regions_harness"), os.path.join(tmp, "texels.bin")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "regions_harness.cpp"),
               "-o", binary, "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        with open(texels, "wb") as f:
            f.write(src.tobytes())
        args = [binary, texels, str(w), str(h)] + [str(v) for case in cases for v in case]
        done = subprocess.run(args, capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr)
    lines = done.stdout.splitlines()
    assert len(lines) == len(cases) + 2
    for line, (x, y, cw, ch) in zip(lines, cases):
        assert line == "crop " + M.crop(src, x, y, cw, ch).tobytes().hex(), (x, y, cw, ch)
    for line, (channel, threshold) in zip(lines[len(cases):], ((M.A, 1), (M.R, 128))):
        histogram, bounds, count = M.statistics(src, channel, threshold)
        assert line == "statistics %d %d %d %d %d %s" % (*bounds, count, histogram.astype("<u4").tobytes().hex()), (channel, threshold)
