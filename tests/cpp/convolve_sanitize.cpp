// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_convolve_cpu.py: a stand-alone host
// program around the rule of csrc/convolve.hpp, the code crh_convolve_texels runs (no library, no device). It puts images through kernels of
// every shape the tests use — 15 x 15 on 1-texel axes among them — under all four edges and both alpha modes, in buffers that end exactly
// where the image does, at odd addresses, and compares with a plain loop in 64-bit integers that wraps by its own arithmetic and divides
// where the rule multiplies by a reciprocal; and it reaches both ends of the accumulator, where a signed overflow would be the sanitizer's
// to see. Exit status 0 = all equal.
#include <convolve.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

namespace {

long long wrap_plain(long long i, long long n, unsigned edge) { // PAD, REPEAT, REFLECT by floor division
    if (edge == 1) return i < 0 ? 0 : i >= n ? n - 1 : i;
    const long long p = edge == 2 ? n : 2 * n;
    long long k = i % p;
    if (k < 0) k += p;
    return k < n ? k : p - 1 - k;
}

void loaded_plain(const uint8_t* in, int w, int h, long long x, long long y, unsigned edge, bool preserve, long long s[4]) {
    s[0] = s[1] = s[2] = s[3] = 0;
    if (edge == 0) {
        if (x < 0 || x >= w || y < 0 || y >= h) return;
    } else {
        x = wrap_plain(x, w, edge), y = wrap_plain(y, h, edge);
    }
    const uint8_t* t = in + ((size_t)y * w + (size_t)x) * 4;
    const long long a = t[3];
    for (int c = 0; c < 3; ++c) {
        const long long v = t[c] < a ? t[c] : a;
        s[c] = preserve ? (a ? (255 * v + a / 2) / a : 0) : v;
    }
    s[3] = a;
}

void plain(const uint8_t* in, int w, int h, const crh::ConvolveCoefficients& f, int ox, int oy, int tx, int ty, unsigned edge, bool preserve, std::vector<uint8_t>& out) {
    out.assign((size_t)w * h * 4, 0);
    for (int j = 0; j < h; ++j)
        for (int i = 0; i < w; ++i) {
            long long n[4] = {255LL * f.bias_k + 32768, 255LL * f.bias_k + 32768, 255LL * f.bias_k + 32768, 255LL * f.bias_k + 32768};
            for (int r = 0; r < oy; ++r)
                for (int c = 0; c < ox; ++c) {
                    long long s[4];
                    loaded_plain(in, w, h, (long long)i - tx + (ox - 1 - c), (long long)j - ty + (oy - 1 - r), edge, preserve, s);
                    for (int ch = 0; ch < 4; ++ch) n[ch] += (long long)f.k[r * ox + c] * s[ch];
                }
            long long v[4];
            for (int ch = 0; ch < 4; ++ch) {
                const long long q = n[ch] >= 0 ? n[ch] / 65536 : -((-n[ch] + 65535) / 65536); // the floor
                v[ch] = q < 0 ? 0 : q > 255 ? 255 : q;
            }
            uint8_t* d = out.data() + ((size_t)j * w + i) * 4;
            if (preserve) {
                const long long a = in[((size_t)j * w + i) * 4 + 3];
                for (int c = 0; c < 3; ++c) d[c] = (uint8_t)((v[c] * a + 127) / 255);
                d[3] = (uint8_t)a;
            } else {
                for (int c = 0; c < 3; ++c) d[c] = (uint8_t)(v[c] < v[3] ? v[c] : v[3]);
                d[3] = (uint8_t)v[3];
            }
        }
}

uint32_t seed = 12345u;
uint32_t next() { return seed = seed * 1664525u + 1013904223u, seed >> 8; }

int run(int w, int h, const float* kernel, int ox, int oy, int tx, int ty, float divisor, float bias, unsigned edge, bool preserve, bool white, size_t& texels) {
    using namespace crh;
    ConvolveCoefficients f;
    if (convolve_quantize(kernel, (uint32_t)ox, (uint32_t)oy, divisor, bias, &f) != kConvolveOk) return 1;
    const size_t n = (size_t)w * h * 4;
    // exact-size heap buffers at an odd address: a read or write past either end is the sanitizer's to see
    uint8_t* in = (uint8_t*)std::malloc(n + 1);
    for (size_t k = 0; k < n; ++k) in[1 + k] = white ? 255 : (uint8_t)next();
    std::vector<uint8_t> expect;
    plain(in + 1, w, h, f, ox, oy, tx, ty, edge, preserve, expect);
    uint8_t* out = (uint8_t*)std::malloc(n + 3);
    if (preserve) convolve_run<true>(in + 1, (uint32_t)w, (uint32_t)h, f, (uint32_t)ox, (uint32_t)oy, (uint32_t)tx, (uint32_t)ty, edge, out + 3);
    else convolve_run<false>(in + 1, (uint32_t)w, (uint32_t)h, f, (uint32_t)ox, (uint32_t)oy, (uint32_t)tx, (uint32_t)ty, edge, out + 3);
    const int differs = std::memcmp(out + 3, expect.data(), n) != 0;
    if (differs) std::printf("%d x %d order (%d, %d) target (%d, %d) edge %u preserve %d: differs\n", w, h, ox, oy, tx, ty, edge, (int)preserve);
    texels += n / 4;
    std::free(in), std::free(out);
    return differs;
}

} // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 3}, {33, 17}};
    const int orders[][2] = {{1, 1}, {3, 3}, {2, 4}, {5, 5}, {15, 1}, {1, 15}, {15, 15}};
    size_t texels = 0;
    int failures = 0;
    for (const auto& size : sizes)
        for (const auto& order : orders) {
            const int ox = order[0], oy = order[1];
            std::vector<float> kernel((size_t)ox * oy); // exact size: a read past the kernel is the sanitizer's to see
            for (float& v : kernel) v = ((int)(next() % 2001u) - 1000) / 250.0f / (float)(ox * oy); // sum |k| <= 4 before the divisor
            const int targets[][2] = {{ox / 2, oy / 2}, {0, 0}, {ox - 1, oy - 1}};
            for (const auto& target : targets)
                for (unsigned edge = 0; edge < 4; ++edge)
                    for (int preserve = 0; preserve < 2; ++preserve)
                        failures += run(size[0], size[1], kernel.data(), ox, oy, target[0], target[1], 0.75f, 0.125f, edge, preserve != 0, false, texels);
        }
    // both ends of the accumulator: sum |k| = 2^22 exactly, all of one sign, on an all-255 image with the bias of the same sign
    for (int sign = -1; sign <= 1; sign += 2) {
        std::vector<float> kernel(15 * 15, 0.0f);
        for (int t = 0; t < 64; ++t) kernel[(size_t)t * 3] = (float)sign; // 64 entries of +-1: 64 * 65536
        for (unsigned edge = 0; edge < 4; ++edge)
            for (int preserve = 0; preserve < 2; ++preserve) failures += run(9, 5, kernel.data(), 15, 15, 7, 7, 1.0f, (float)sign, edge, preserve != 0, true, texels);
    }
    // the refusals of the quantisation
    {
        crh::ConvolveCoefficients f;
        const float inf = std::numeric_limits<float>::infinity();
        const float one[1] = {1.0f}, big[1] = {65.0f}, bad[1] = {inf}, most[2] = {32.0f, 32.0f}, over[2] = {32.0f, 32.0001f};
        if (crh::convolve_quantize(one, 1, 1, 1.0f, 0.0f, &f) != crh::kConvolveOk || f.k[0] != 65536 || f.bias != 32768) ++failures;
        if (crh::convolve_quantize(big, 1, 1, 1.0f, 0.0f, &f) != crh::kConvolveGain) ++failures;
        if (crh::convolve_quantize(one, 1, 1, 1e-30f, 0.0f, &f) != crh::kConvolveGain) ++failures; // a quotient no int32 holds
        if (crh::convolve_quantize(bad, 1, 1, 1.0f, 0.0f, &f) != crh::kConvolveNonFinite) ++failures;
        if (crh::convolve_quantize(one, 1, 1, inf, 0.0f, &f) != crh::kConvolveNonFinite) ++failures;
        if (crh::convolve_quantize(one, 1, 1, 1.0f, -inf, &f) != crh::kConvolveNonFinite) ++failures;
        if (crh::convolve_quantize(most, 2, 1, 1.0f, 1.0f, &f) != crh::kConvolveOk || f.bias_k != 65536) ++failures;
        if (crh::convolve_quantize(over, 2, 1, 1.0f, 0.0f, &f) != crh::kConvolveGain) ++failures;
    }
    std::printf("%zu texels, %d failures\n", texels, failures);
    return failures ? 1 : 0;
}
