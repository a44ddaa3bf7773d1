// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_morphology_cpu.py: a stand-alone host
// program around the rule of csrc/morphology.hpp, the code crh_morphology_texels runs (no library, no device). It puts images through both
// operators and all four edges — radius 192 on 1-texel axes among them — in buffers that end exactly where the image does, at odd addresses,
// and compares with a plain double loop over the window that wraps by its own arithmetic; and it walks csrc/edge.hpp's stepped wrap, the one
// the vertical kernel uses, its direct one and its branching one against that arithmetic. Exit status 0 = all equal.
#include <morphology.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

long long wrap_plain(long long i, long long n, unsigned edge) { // PAD, REPEAT, REFLECT by floor division
    if (edge == 1) return i < 0 ? 0 : i >= n ? n - 1 : i;
    const long long p = edge == 2 ? n : 2 * n;
    long long k = i % p;
    if (k < 0) k += p;
    return k < n ? k : p - 1 - k;
}

void plain(const uint8_t* in, int w, int h, bool dilate, int rx, int ry, unsigned edge, std::vector<uint8_t>& out, int& ow, int& oh) {
    const bool grows = dilate && edge == 0;
    ow = w + (grows ? 2 * rx : 0), oh = h + (grows ? 2 * ry : 0);
    out.assign((size_t)ow * oh * 4, 0);
    for (int j = 0; j < oh; ++j)
        for (int i = 0; i < ow; ++i)
            for (int c = 0; c < 4; ++c) {
                int best = dilate ? 0 : 255;
                // under TRANSPARENT the texels of the window outside the source are all zero: one zero stands for them, and the loops run over
                // the part of the window inside the source (a grown 385 x 385 result of a single texel would otherwise take 2 * 10^10 steps)
                int x0 = i - (grows ? rx : 0) - rx, x1 = x0 + 2 * rx, y0 = j - (grows ? ry : 0) - ry, y1 = y0 + 2 * ry;
                if (edge == 0) {
                    if (x0 < 0 || x1 >= w || y0 < 0 || y1 >= h) best = dilate ? best : 0;
                    x0 = x0 < 0 ? 0 : x0, x1 = x1 >= w ? w - 1 : x1, y0 = y0 < 0 ? 0 : y0, y1 = y1 >= h ? h - 1 : y1;
                }
                for (long long y = y0; y <= y1; ++y)
                    for (long long x = x0; x <= x1; ++x) {
                        const int v = edge != 0 ? in[((size_t)wrap_plain(y, h, edge) * w + (size_t)wrap_plain(x, w, edge)) * 4 + c] : in[((size_t)y * w + (size_t)x) * 4 + c];
                        best = dilate ? (v > best ? v : best) : (v < best ? v : best);
                    }
                out[((size_t)j * ow + i) * 4 + c] = (uint8_t)best;
            }
}

} // namespace

int main() {
    using namespace crh;
    struct Case {
        int w, h, rx, ry;
    };
    const Case cases[] = {{1, 1, 192, 192}, {1, 7, 192, 3}, {7, 1, 2, 192}, {5, 3, 0, 0}, {5, 3, 1, 0}, {5, 3, 0, 1}, {9, 7, 2, 1}, {13, 11, 7, 3}, {6, 5, 40, 40}, {1, 3, 192, 0}};
    size_t texels = 0;
    int failures = 0;
    uint32_t seed = 12345u;
    for (const Case& c : cases)
        for (unsigned edge = 0; edge < 4; ++edge)
            for (int dilate = 0; dilate < 2; ++dilate) {
                const size_t n = (size_t)c.w * c.h * 4;
                // exact-size heap buffers at an odd address: a read or write past either end is the sanitizer's to see
                uint8_t* in = (uint8_t*)std::malloc(n + 1);
                for (size_t k = 0; k < n; ++k) seed = seed * 1664525u + 1013904223u, in[1 + k] = (uint8_t)(seed >> 24);
                std::vector<uint8_t> expect;
                int ow = 0, oh = 0;
                plain(in + 1, c.w, c.h, dilate != 0, c.rx, c.ry, edge, expect, ow, oh);
                const bool grows = morphology_grows(dilate ? kMorphologyDilate : kMorphologyErode, edge);
                if (ow != c.w + (grows ? 2 * c.rx : 0) || oh != c.h + (grows ? 2 * c.ry : 0)) ++failures;
                uint8_t* out = (uint8_t*)std::malloc(expect.size() + 3);
                if (dilate) morphology_run<true>(in + 1, (uint32_t)c.w, (uint32_t)c.h, (uint32_t)c.rx, (uint32_t)c.ry, edge, out + 3);
                else morphology_run<false>(in + 1, (uint32_t)c.w, (uint32_t)c.h, (uint32_t)c.rx, (uint32_t)c.ry, edge, out + 3);
                if (std::memcmp(out + 3, expect.data(), expect.size())) ++failures, std::printf("%d x %d radius (%d, %d) edge %u dilate %d: differs\n", c.w, c.h, c.rx, c.ry, edge, dilate);
                texels += expect.size() / 4;
                std::free(in), std::free(out);
            }
    // the wrap directly and by steps of one from a pivot, up and down, against the plain arithmetic: sizes 1 .. 9 and 16384, 400 steps either way
    const int sizes[] = {1, 2, 3, 4, 5, 7, 9, 16384};
    for (int n : sizes)
        for (unsigned edge = 1; edge < 4; ++edge)
            for (int pivot : {-385, -1, 0, n - 1, n, 3 * n + 1}) {
                const int period = edge_period(n, edge);
                int up = edge_phase(pivot, n, edge), down = up;
                for (int k = 0; k <= 400; ++k) {
                    if (k) up = edge_phase_before(up, period), down = edge_phase_next(down, period);
                    for (int side = 0; side < 2; ++side) {
                        const int i = side ? pivot + k : pivot - k, expect = (int)wrap_plain(i, n, edge);
                        if (edge_wrap_at(i, side ? down : up, n, edge) != expect || edge_wrap(i, n, edge) != expect || edge_wrap_branching(i, n, edge) != expect) ++failures;
                    }
                }
            }
    // the packed min / max: every pair of codes in every field
    for (uint32_t a = 0; a < 256u; ++a)
        for (uint32_t b = 0; b < 256u; ++b) {
            const uint32_t x = a | (255u - a) << 8 | b << 16 | a << 24, y = b | (255u - b) << 8 | a << 16 | (255u - b) << 24;
            const uint32_t hi = morphology_merge(morphology_extreme<true>(morphology_split(x), morphology_split(y)));
            const uint32_t lo = morphology_merge(morphology_extreme<false>(morphology_split(x), morphology_split(y)));
            for (int c = 0; c < 4; ++c) {
                const uint32_t p = (x >> (8 * c)) & 255u, q = (y >> (8 * c)) & 255u;
                if (((hi >> (8 * c)) & 255u) != (p > q ? p : q) || ((lo >> (8 * c)) & 255u) != (p < q ? p : q)) ++failures;
            }
        }
    std::printf("%zu texels, %d failures\n", texels, failures);
    return failures ? 1 : 0;
}
