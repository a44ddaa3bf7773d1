"""The sample patterns of msaa 1, 2, 4 and 8 as the header states them (include/contrast_hip.h) and as the raster kernels pack them
(csrc/raster_common.hpp sample_pattern_x / sample_pattern_y, sample_lo / sample_hi): the standard locations, in sample-index order."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STANDARD = {1: [(8, 8)], 2: [(12, 12), (4, 4)], 4: [(6, 2), (14, 6), (2, 10), (10, 14)],
            8: [(9, 5), (7, 11), (13, 9), (5, 3), (3, 13), (1, 7), (11, 15), (15, 1)]}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_header_states_the_standard_patterns():
    text = _read("include", "contrast_hip.h")
    for n, pattern in STANDARD.items():
        m = re.search(rf"^ \*   {n}: (.*)$", text, re.M)
        assert m, n
        stated = [tuple(int(v) for v in p) for p in re.findall(r"\((\d+), (\d+)\)", m.group(1))]
        assert stated == pattern, n
    assert "1, 2, 4 or 8" in text


def _packed(name, text):
    m = re.search(rf"constexpr uint32_t {name}\(int samples\) {{ return (.*?); }}", text)
    assert m, name
    words = dict(re.findall(r"samples == (\d+) \? (0x[0-9A-F]+)u", m.group(1)))
    words["1"] = re.search(r": (0x[0-9A-F]+)u\)+$", m.group(1)).group(1)
    return {int(k): int(v, 16) for k, v in words.items()}


def test_the_kernels_pack_the_standard_patterns():
    text = _read("contrast_renderer_amd", "csrc", "raster_common.hpp")
    px, py = _packed("sample_pattern_x", text), _packed("sample_pattern_y", text)
    for n, pattern in STANDARD.items():
        assert [((px[n] >> (4 * k)) & 15, (py[n] >> (4 * k)) & 15) for k in range(n)] == pattern, n
    # the tile tests' corners: the extremes of the pattern, both axes alike
    for fn, pick in (("sample_lo", min), ("sample_hi", max)):
        body = re.search(rf"constexpr float {fn}\(int samples\) {{ return (.*?); }}", text).group(1)
        vals = dict(re.findall(r"samples == (\d+) \? ([0-9.]+)f", body))
        vals["1"] = re.search(r": ([0-9.]+)f\)+$", body).group(1)
        for n, pattern in STANDARD.items():
            assert float(vals[str(n)]) == pick(v for p in pattern for v in p) / 16.0, (fn, n)
