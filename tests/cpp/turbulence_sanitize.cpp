// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_turbulence_cpu.py: a stand-alone host
// program around the rule of csrc/turbulence.hpp, the code crh_turbulence_texels runs (no library, no device). It makes images of every
// size the tests use, of both kinds, opaque and not, stitched and not, with 0 to 12 octaves, in buffers that end exactly where the image does,
// at odd addresses, and compares with a plain loop that writes the header's rule out again with libm's floor, a division by the ratio and
// the % operator on 64-bit integers; among the cases are the rule's edges: the seeds at both ends of int32 and the one with a zero
// gradient, frequencies 0 and 4, offsets of +-65536 on an axis of 16384 texels under 12 octaves — the largest lattice coordinates, where a
// conversion of a double no 32-bit integer holds, a shift or a product that overflows would be the sanitizer's to see. Exit status 0 = all equal.
#include <turbulence.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Case {
    unsigned kind, octaves;
    int seed;
    bool stitch, opaque;
    float frequency[2], offset[2];
};

long long wrap_plain(long long i, long long period) {
    if (period != 0) {
        i %= period;
        if (i < 0) i += period;
    }
    return i & 255;
}

double noise_plain(const crh::TurbulenceTables& t, int k, double vx, double vy, long long px, long long py) {
    const double flx = floor(vx), fly = floor(vy);
    const long long ix = (long long)flx, iy = (long long)fly;
    const double rx0 = vx - flx, ry0 = vy - fly, rx1 = rx0 - 1.0, ry1 = ry0 - 1.0;
    const long long bx0 = wrap_plain(ix, px), bx1 = wrap_plain(ix + 1, px), by0 = wrap_plain(iy, py), by1 = wrap_plain(iy + 1, py);
    const int a0 = t.lattice[bx0], a1 = t.lattice[bx1];
    const double* q00 = t.gradient + (k * 256 + t.lattice[(a0 + by0) & 255]) * 2;
    const double* q10 = t.gradient + (k * 256 + t.lattice[(a1 + by0) & 255]) * 2;
    const double* q01 = t.gradient + (k * 256 + t.lattice[(a0 + by1) & 255]) * 2;
    const double* q11 = t.gradient + (k * 256 + t.lattice[(a1 + by1) & 255]) * 2;
    const double sx = (rx0 * rx0) * (3.0 - (2.0 * rx0)), sy = (ry0 * ry0) * (3.0 - (2.0 * ry0));
    double u = (rx0 * q00[0]) + (ry0 * q00[1]);
    double v = (rx1 * q10[0]) + (ry0 * q10[1]);
    const double a = u + (sx * (v - u));
    u = (rx0 * q01[0]) + (ry1 * q01[1]);
    v = (rx1 * q11[0]) + (ry1 * q11[1]);
    const double b = u + (sx * (v - u));
    return a + (sy * (b - a));
}

void axis_plain(double f, int n_texels, bool stitch, double* f_out, long long* period) {
    *f_out = f, *period = 0;
    if (!stitch || f == 0.0) return;
    const double n = (double)n_texels, lo = floor(n * f) / n, hi = -floor(-(n * f)) / n;
    *f_out = lo == 0.0 ? hi : (f / lo < hi / f ? lo : hi);
    *period = (long long)floor(n * *f_out + 0.5);
}

void plain(const crh::TurbulenceTables& t, int w, int h, const Case& c, std::vector<uint8_t>& out) {
    out.assign((size_t)w * h * 4, 0);
    double fx, fy;
    long long px, py;
    axis_plain((double)c.frequency[0], w, c.stitch, &fx, &px);
    axis_plain((double)c.frequency[1], h, c.stitch, &fy, &py);
    for (int j = 0; j < h; ++j)
        for (int i = 0; i < w; ++i) {
            unsigned code[4] = {0, 0, 0, 255};
            for (int k = 0; k < (c.opaque ? 3 : 4); ++k) {
                double vx = ((double)c.offset[0] + (double)i) * fx, vy = ((double)c.offset[1] + (double)j) * fy, sum = 0.0, ratio = 1.0;
                for (unsigned o = 0; o < c.octaves; ++o) {
                    const double n = noise_plain(t, k, vx, vy, px << o, py << o);
                    sum = sum + ((c.kind == 0 ? n : fabs(n)) / ratio);
                    ratio = ratio * 2.0;
                    vx = vx * 2.0, vy = vy * 2.0;
                }
                const double tt = c.kind == 0 ? (sum + 1.0) * 0.5 : sum;
                code[k] = tt >= 1.0 ? 255u : tt > 0.0 ? (unsigned)floor(tt * 255.0 + 0.5) : 0u;
            }
            uint8_t* d = out.data() + ((size_t)j * w + i) * 4;
            for (int k = 0; k < 3; ++k) d[k] = (uint8_t)((code[k] * code[3] + 127u) / 255u);
            d[3] = (uint8_t)code[3];
        }
}

} // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {33, 17}, {64, 32}, {16384, 1}, {1, 16384}};
    const int seeds[] = {1, 0, -1, 346, 2147483647, -2147483647 - 1};
    const float places[][4] = {{0.05f, 0.08f, 10.0f, 20.0f}, {4.0f, 0.0f, 65536.0f, -65536.0f}, {2.0f, 3.0f, -0.5f, 7.25f}, {0.013f, 3.9f, -65536.0f, 65536.0f},
                               {0.0f, 0.3f, 1.5f, -3.75f},   {3.999f, 3.999f, 65536.0f, 65536.0f}, {3.999f, 3.999f, -65536.0f, -65536.0f}};
    const unsigned octaves[] = {0, 1, 4, 12};
    size_t texels = 0, failures = 0;
    unsigned turn = 0;
    std::vector<uint8_t> expect;
    for (const auto& size : sizes)
        for (unsigned kind = 0; kind < 2; ++kind)
            for (int stitch = 0; stitch < 2; ++stitch)
                for (int opaque = 0; opaque < 2; ++opaque)
                    for (const auto& place : places) {
                        const int w = size[0], h = size[1];
                        Case c = {kind, octaves[turn % 4], seeds[turn % 6], stitch != 0, opaque != 0, {place[0], place[1]}, {place[2], place[3]}};
                        if (w * h > 4096) {
                            if (place[0] < 3.9f) continue; // the long axes are for the largest coordinates alone
                            c.octaves = 12;
                        }
                        ++turn;
                        crh::TurbulenceTables t;
                        crh::turbulence_make_tables(c.seed, &t);
                        crh::TurbulenceConstants f;
                        crh::turbulence_prepare((uint32_t)w, (uint32_t)h, c.octaves, c.stitch, c.frequency, c.offset, &f);
                        // a buffer that ends with the image, at an odd address: a byte too many written or read is the sanitizer's to see
                        std::vector<uint8_t> raw((size_t)w * h * 4 + 1);
                        crh::turbulence_run(t, f, c.kind, c.opaque, (uint32_t)w, (uint32_t)h, raw.data() + 1);
                        plain(t, w, h, c, expect);
                        texels += (size_t)w * h;
                        if (memcmp(raw.data() + 1, expect.data(), expect.size()) != 0) {
                            ++failures;
                            printf("differs: %d x %d kind %u stitch %d opaque %d octaves %u seed %d frequency %g %g offset %g %g\n", w, h, kind, stitch, opaque, c.octaves, c.seed, place[0], place[1],
                                   place[2], place[3]);
                        }
                    }
    printf("%zu texels, %zu failures\n", texels, failures);
    return failures == 0 ? 0 : 1;
}
