// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_distance_cpu.py: a stand-alone host
// program around the rule of csrc/distance.hpp, the code crh_distance_texels runs (no library, no device). It makes distance fields of
// images of every size the tests use, in both modes, under every edge, from and into heap buffers that end exactly where the image and the
// result do, at odd addresses, and compares with a plain loop that writes the header's rule out again: a double loop over every q within
// the spread, 64-bit integers, the % operator and no tables. Among the cases is the rule's edge: spread 255 on a 1 x 1 and a 3 x 2 image
// (an index 255 periods out under every wrapping edge, and a result of 511 x 511 from one texel): an index that left the source or the
// column distances, or a product that overflows, would be the sanitizer's to see. Exit status 0 = all equal.
#include <distance.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

long long wrap_plain(long long i, long long n, unsigned edge) {
    if (edge == 1u) return i < 0 ? 0 : i >= n ? n - 1 : i;
    const long long p = edge == 2u ? n : 2 * n;
    long long k = i % p;
    if (k < 0) k += p;
    return k < n ? k : 2 * n - 1 - k;
}

bool inside_plain(const uint8_t* in, long long w, long long h, unsigned channel, unsigned threshold, unsigned edge, long long x, long long y) {
    if (edge == 0u) {
        if (x < 0 || x >= w || y < 0 || y >= h) return false;
    } else {
        x = wrap_plain(x, w, edge), y = wrap_plain(y, h, edge);
    }
    return in[(y * w + x) * 4 + channel] >= threshold;
}

unsigned code_plain(long long d2, long long spread) { // d2 < 0: none
    if (d2 == 0) return 0u;
    if (d2 < 0 || d2 >= spread * spread) return 255u;
    unsigned c = 0u;
    for (long long k = 1; k < 256; ++k)
        if ((2 * k - 1) * (2 * k - 1) * spread * spread <= 260100 * d2) c = (unsigned)k;
    return c;
}

void plain(const uint8_t* in, int w, int h, unsigned mode, unsigned channel, unsigned threshold, int spread, unsigned edge, std::vector<uint8_t>& out) {
    const int o = mode == 0u && edge == 0u ? spread : 0;
    const int out_w = w + 2 * o, out_h = h + 2 * o;
    out.assign((size_t)out_w * out_h * 4, 0);
    const bool wanted = mode == 0u;
    if (o != 0) { // OUTSIDE under TRANSPARENT: every inside q is a texel of the source, so the least |p - q|^2 is over those, whatever the spread
        for (int j = 0; j < out_h; ++j)
            for (int i = 0; i < out_w; ++i) {
                long long d2 = -1;
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) {
                        const long long dx = x - (i - o), dy = y - (j - o);
                        if (inside_plain(in, w, h, channel, threshold, edge, x, y) && (d2 < 0 || dx * dx + dy * dy < d2)) d2 = dx * dx + dy * dy;
                    }
                uint8_t* d = out.data() + ((size_t)j * out_w + i) * 4;
                d[0] = d[1] = d[2] = d[3] = (uint8_t)(255u - code_plain(d2, spread));
            }
        return;
    }
    // the inside map over every position a window reaches, once
    const int reach = o + spread, map_w = w + 2 * reach, map_h = h + 2 * reach;
    std::vector<uint8_t> map((size_t)map_w * map_h);
    for (int y = 0; y < map_h; ++y)
        for (int x = 0; x < map_w; ++x) map[(size_t)y * map_w + x] = inside_plain(in, w, h, channel, threshold, edge, x - reach, y - reach) == wanted;
    for (int j = 0; j < out_h; ++j)
        for (int i = 0; i < out_w; ++i) {
            long long d2 = -1;
            for (int dy = -spread; dy <= spread; ++dy)
                for (int dx = -spread; dx <= spread; ++dx)
                    if (map[(size_t)(j + spread + dy) * map_w + (i + spread + dx)] && (d2 < 0 || (long long)dx * dx + (long long)dy * dy < d2)) d2 = (long long)dx * dx + (long long)dy * dy;
            const unsigned c = code_plain(d2, spread), v = mode == 1u ? c : 255u - c;
            uint8_t* d = out.data() + ((size_t)j * out_w + i) * 4;
            d[0] = d[1] = d[2] = d[3] = (uint8_t)v;
        }
}

uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

} // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {3, 2}, {1, 40}, {40, 1}, {7, 5}, {64, 9}, {67, 33}};
    const int spreads[] = {1, 2, 4, 17, 255};
    size_t texels = 0, failures = 0;
    uint32_t seed = 12345u;
    unsigned turn = 0;
    std::vector<uint8_t> expect;
    for (const auto& size : sizes)
        for (const int spread : spreads)
            for (unsigned edge = 0; edge < 4; ++edge)
                for (unsigned mode = 0; mode < 2; ++mode) {
                    const int w = size[0], h = size[1];
                    if (spread == 255 && w * h > 6) continue; // the plain loop is quadratic in the spread: the largest is for the two smallest images, whose wraps lie many periods out
                    const unsigned thresholds[] = {1u, 128u, 255u, 77u};
                    const unsigned channel = turn % 4u, threshold = thresholds[(turn / 4u) % 4u];
                    ++turn;
                    const int o = mode == 0u && edge == 0u ? spread : 0;
                    const size_t bytes = (size_t)w * h * 4, out_bytes = (size_t)(w + 2 * o) * (h + 2 * o) * 4;
                    // buffers that end with the image and with the result, at odd addresses: a byte too many read or written is the sanitizer's to see
                    std::vector<uint8_t> in(bytes + 1), raw(out_bytes + 1);
                    for (size_t n = 1; n <= bytes; ++n) in[n] = (rnd(seed) >> 24) % 5u == 0u ? (uint8_t)(rnd(seed) >> 24) : (uint8_t)0;
                    if (turn % 5u == 0u) memset(in.data() + 1, 255, bytes); // a full image: no outside under a wrapping edge
                    if (turn % 7u == 0u) memset(in.data() + 1, 0, bytes);   // an empty one
                    const crh::DistanceConstants f = {mode, 8u * channel, threshold, (uint32_t)spread, edge};
                    crh::distance_run(in.data() + 1, (uint32_t)w, (uint32_t)h, f, raw.data() + 1);
                    plain(in.data() + 1, w, h, mode, channel, threshold, spread, edge, expect);
                    texels += expect.size() / 4;
                    if (expect.size() != out_bytes || memcmp(raw.data() + 1, expect.data(), expect.size()) != 0) {
                        ++failures;
                        printf("differs: %d x %d spread %d mode %u channel %u threshold %u edge %u\n", w, h, spread, mode, channel, threshold, edge);
                    }
                }
    // the thresholds against the integer statement, every spread and every D2 up to spread^2 + 2
    for (int spread = 1; spread <= 255; ++spread) {
        crh::DistanceThresholds t;
        crh::distance_thresholds((uint32_t)spread, &t);
        for (long long d2 = 0; d2 <= (long long)spread * spread + 2; d2 += spread < 32 ? 1 : 1 + d2 % 7) {
            const long long capped = d2 < (long long)spread * spread ? d2 : (long long)spread * spread;
            if (crh::distance_code(t.t, (uint32_t)capped) != code_plain(d2, spread)) {
                ++failures;
                printf("differs: c(%lld) at spread %d\n", d2, spread);
            }
        }
    }
    printf("%zu texels, %zu failures\n", texels, failures);
    return failures == 0 ? 0 : 1;
}
