// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_color_filter_cpu.py: a stand-alone host program around the rule of
// csrc/color_filter.hpp, the code crh_color_filter_texels runs (no library, no device). It puts all 32 896 texels c <= a, and texels that
// are not premultiplied, through the extreme matrices (every sum at its 32-bit bound), through tables, in place and at odd addresses, in
// buffers that end exactly where the run does, and compares with the six stages written with plain divisions. Exit status 0 = all equal.
#include <color_filter.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

void plain(const uint8_t* in, size_t n, const float* m, const uint8_t* tables, uint8_t* out) {
    long long k[20];
    for (int j = 0; j < 20; ++j) k[j] = (long long)std::floor((double)m[j] * 65536.0 + 0.5);
    for (size_t t = 0; t < n; ++t) {
        long long u[5];
        const long long a = in[4 * t + 3];
        for (int c = 0; c < 3; ++c) {
            const long long code = in[4 * t + c] < a ? in[4 * t + c] : a;
            u[c] = a ? (255 * code + a / 2) / a : 0;
        }
        u[3] = a, u[4] = 255;
        long long v[4];
        for (int i = 0; i < 4; ++i) {
            long long sum = 32768;
            for (int j = 0; j < 5; ++j) sum += k[5 * i + j] * u[j];
            long long s = sum >= 0 ? sum / 65536 : -((-sum + 65535) / 65536); // the floor
            v[i] = s < 0 ? 0 : s > 255 ? 255 : s;
            if (tables) v[i] = tables[256 * i + v[i]];
        }
        for (int c = 0; c < 3; ++c) out[4 * t + c] = (uint8_t)((v[c] * v[3] + 127) / 255);
        out[4 * t + 3] = (uint8_t)v[3];
    }
}

} // namespace

int main() {
    using namespace crh;
    std::vector<uint8_t> texels;
    for (unsigned a = 0; a < 256; ++a)
        for (unsigned c = 0; c <= a; ++c) {
            const uint8_t t[4] = {(uint8_t)c, (uint8_t)((c * 7 + 3) % (a + 1)), (uint8_t)(a - c), (uint8_t)a};
            texels.insert(texels.end(), t, t + 4);
        }
    for (unsigned n = 0; n < 4096; ++n) { // not premultiplied
        const uint8_t t[4] = {(uint8_t)(n * 37), (uint8_t)(n * 101 + 5), (uint8_t)(255 - n), (uint8_t)(n * 13 >> 2)};
        texels.insert(texels.end(), t, t + 4);
    }
    const size_t n = texels.size() / 4;
    float matrices[5][20] = {{1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0}, {}, {}, {0.213f, 0.715f, 0.072f, 0, 0, -0.5f, 1.25f, 0.33f, -0.1f, 0.2f, 3, -7, 2, 1, -0.4f, 0.2125f, 0.7154f, 0.0721f, 0.5f, 0.1f}, {}};
    for (int j = 0; j < 20; ++j) matrices[1][j] = 16.0f, matrices[2][j] = -16.0f, matrices[4][j] = (j % 3 ? 16.0f : -16.0f);
    std::vector<uint8_t> tables(1024);
    for (size_t j = 0; j < 1024; ++j) tables[j] = (uint8_t)((j * 167 + 13 * (j >> 8)) & 255);
    std::vector<uint8_t> expect(4 * n);
    int failures = 0;
    for (int which = 0; which < 5; ++which)
        for (int with_tables = 0; with_tables < 2; ++with_tables) {
            const uint8_t* t = with_tables ? tables.data() : nullptr;
            plain(texels.data(), n, matrices[which], t, expect.data());
            ColorFilterCoefficients f;
            if (color_filter_quantize(matrices[which], &f) != kColorFilterOk) return 2;
            // exact-size heap buffers at an odd address: a read or write past either end is the sanitizer's to see
            uint8_t* in = (uint8_t*)std::malloc(4 * n + 1);
            uint8_t* out = (uint8_t*)std::malloc(4 * n + 3);
            std::memcpy(in + 1, texels.data(), 4 * n);
            if (with_tables) color_filter_run<true>(in + 1, n, f, t, out + 3);
            else color_filter_run<false>(in + 1, n, f, t, out + 3);
            if (std::memcmp(out + 3, expect.data(), 4 * n)) ++failures, std::printf("matrix %d tables %d: differs\n", which, with_tables);
            if (with_tables) color_filter_run<true>(in + 1, n, f, t, in + 1); // in place
            else color_filter_run<false>(in + 1, n, f, t, in + 1);
            if (std::memcmp(in + 1, expect.data(), 4 * n)) ++failures, std::printf("matrix %d tables %d: differs in place\n", which, with_tables);
            std::free(in), std::free(out);
        }
    ColorFilterCoefficients f;
    float bad[20] = {};
    bad[3] = 16.000002f;
    if (color_filter_quantize(bad, &f) != kColorFilterTooLarge) ++failures;
    bad[3] = NAN;
    if (color_filter_quantize(bad, &f) != kColorFilterNonFinite) ++failures;
    if (color_filter_quantize(nullptr, &f) != kColorFilterOk || f.k[2][2] != 65536 || f.k[0][1] != 0 || f.bias[3] != 32768) ++failures;
    std::printf("%zu texels, %d failures\n", n, failures);
    return failures ? 1 : 0;
}
