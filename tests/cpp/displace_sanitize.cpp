// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_displace_cpu.py: a stand-alone host
// program around the rule of csrc/displace.hpp, the code crh_displace_texels runs (no library, no device). It displaces images of every
// size the tests use under both filters, every edge and several channel pairs, from and into heap buffers that end exactly where the
// image does, at odd addresses, and compares with a plain loop that writes the header's rule out again in 64-bit integers with a floor
// division, the % operator and no tables. Among the cases are the rule's edges: scales of +-1024 on axes of 1 and 3 texels (an index
// many periods out under every wrapping edge) and on axes of 16384 texels (the largest positions and addresses): an index that left the
// source, a shift of a negative value taken wrongly or a product that overflows would be the sanitizer's to see. Exit status 0 = all equal.
#include <displace.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

long long floor_div(long long a, long long b) { // b > 0
    long long q = a / b;
    if (a % b < 0) --q;
    return q;
}

long long wrap_plain(long long i, long long n, unsigned edge) {
    if (edge == 1u) return i < 0 ? 0 : i >= n ? n - 1 : i;
    const long long p = edge == 2u ? n : 2 * n;
    long long k = i % p;
    if (k < 0) k += p;
    return k < n ? k : 2 * n - 1 - k;
}

long long code_plain(const uint8_t* texel, unsigned channel) {
    const long long a = texel[3];
    if (channel == 3u) return a;
    const long long c = texel[channel] < a ? texel[channel] : a;
    return a == 0 ? 0 : (255 * c + a / 2) / a;
}

void fetch_plain(const uint8_t* in, long long w, long long h, unsigned edge, long long i, long long j, long long s[4]) {
    if (edge == 0u) {
        if (i < 0 || i >= w || j < 0 || j >= h) {
            s[0] = s[1] = s[2] = s[3] = 0;
            return;
        }
    } else {
        i = wrap_plain(i, w, edge), j = wrap_plain(j, h, edge);
    }
    for (int c = 0; c < 4; ++c) s[c] = in[(j * w + i) * 4 + c];
}

void plain(const uint8_t* in, const uint8_t* map, int w, int h, const float scale[2], const unsigned channel[2], unsigned filter, unsigned edge, std::vector<uint8_t>& out) {
    out.assign((size_t)w * h * 4, 0);
    const long long kx = (long long)floor((double)scale[0] * 256.0 + 0.5), ky = (long long)floor((double)scale[1] * 256.0 + 0.5);
    for (long long j = 0; j < h; ++j)
        for (long long i = 0; i < w; ++i) {
            const uint8_t* m = map + (j * w + i) * 4;
            const long long X = 256 * i + 128 + floor_div(kx * (2 * code_plain(m, channel[0]) - 255) + 255, 510);
            const long long Y = 256 * j + 128 + floor_div(ky * (2 * code_plain(m, channel[1]) - 255) + 255, 510);
            uint8_t* d = out.data() + (j * w + i) * 4;
            long long s00[4], s10[4], s01[4], s11[4];
            if (filter == 0u) {
                fetch_plain(in, w, h, edge, floor_div(X, 256), floor_div(Y, 256), s00);
                for (int c = 0; c < 4; ++c) d[c] = (uint8_t)s00[c];
                continue;
            }
            const long long i0 = floor_div(X - 128, 256), j0 = floor_div(Y - 128, 256), fx = X - 128 - 256 * i0, fy = Y - 128 - 256 * j0;
            fetch_plain(in, w, h, edge, i0, j0, s00), fetch_plain(in, w, h, edge, i0 + 1, j0, s10);
            fetch_plain(in, w, h, edge, i0, j0 + 1, s01), fetch_plain(in, w, h, edge, i0 + 1, j0 + 1, s11);
            for (int c = 0; c < 4; ++c) {
                const long long top = s00[c] * (256 - fx) + s10[c] * fx, bottom = s01[c] * (256 - fx) + s11[c] * fx;
                d[c] = (uint8_t)floor_div(top * (256 - fy) + bottom * fy + 32768, 65536);
            }
        }
}

uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

} // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {3, 3}, {33, 15}, {64, 17}, {16384, 2}, {2, 16384}};
    const float scales[][2] = {{0.0f, 0.0f}, {0.0f, 37.5f}, {-20.0f, 20.0f}, {7.77f, -0.3f}, {510.0f, 510.0f}, {1024.0f, -1024.0f}, {-1024.0f, 1024.0f}};
    const unsigned pairs[][2] = {{0, 1}, {3, 3}, {2, 0}};
    size_t texels = 0, failures = 0;
    uint32_t seed = 12345u;
    unsigned turn = 0;
    std::vector<uint8_t> expect;
    for (const auto& size : sizes)
        for (const auto& scale : scales)
            for (unsigned edge = 0; edge < 4; ++edge)
                for (unsigned filter = 0; filter < 2; ++filter) {
                    const int w = size[0], h = size[1];
                    if (w * h > 4096 && !(scale[0] == 1024.0f || scale[0] == -1024.0f)) continue; // the long axes are for the largest positions alone
                    const unsigned* pair = pairs[turn++ % 3];
                    const size_t bytes = (size_t)w * h * 4;
                    // buffers that end with the image, at odd addresses: a byte too many read or written is the sanitizer's to see
                    std::vector<uint8_t> in(bytes + 1), map(bytes + 1), raw(bytes + 1);
                    for (size_t n = 1; n <= bytes; ++n) in[n] = (uint8_t)(rnd(seed) >> 24), map[n] = (uint8_t)(rnd(seed) >> 24);
                    if (turn % 4 == 0)
                        for (size_t n = 4; n <= bytes; n += 8) map[n] = 0; // transparent map texels among the others
                    crh::DisplaceConstants f = {{crh::displace_k(scale[0]), crh::displace_k(scale[1])}, {pair[0], pair[1]}, filter, edge};
                    if (filter == crh::kDisplaceLinear) crh::displace_run<crh::kDisplaceLinear>(in.data() + 1, map.data() + 1, (uint32_t)w, (uint32_t)h, f, raw.data() + 1);
                    else crh::displace_run<crh::kDisplaceNearest>(in.data() + 1, map.data() + 1, (uint32_t)w, (uint32_t)h, f, raw.data() + 1);
                    plain(in.data() + 1, map.data() + 1, w, h, scale, pair, filter, edge, expect);
                    texels += (size_t)w * h;
                    if (memcmp(raw.data() + 1, expect.data(), expect.size()) != 0) {
                        ++failures;
                        printf("differs: %d x %d scale %g %g channels %u %u filter %u edge %u\n", w, h, scale[0], scale[1], pair[0], pair[1], filter, edge);
                    }
                }
    printf("%zu texels, %zu failures\n", texels, failures);
    return failures == 0 ? 0 : 1;
}
