// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_lighting_cpu.py: a stand-alone host
// program around the rule of csrc/lighting.hpp, the code crh_lighting_texels runs (no library, no device). It lights images of every size
// the tests use under both ops, the three lights and the four edges, in buffers that end exactly where the image does, at odd addresses,
// and compares with a plain loop that wraps by its own arithmetic, takes its gradient tap by tap and writes the rule's formulas out
// again; among the cases are the rule's edges: a surface scale of 0 and of 256, exponents at both ends, a cone through the image, a light
// inside the surface (len == 0), below it, and at the coordinate limit, where a conversion of a double no integer holds would be the
// sanitizer's to see. Exit status 0 = all equal.
#include <lighting.hpp>

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

long long alpha_plain(const uint8_t* in, int w, int h, long long x, long long y, unsigned edge) {
    if (edge == 0) {
        if (x < 0 || x >= w || y < 0 || y >= h) return 0;
    } else {
        x = wrap_plain(x, w, edge), y = wrap_plain(y, h, edge);
    }
    return in[((size_t)y * w + (size_t)x) * 4 + 3];
}

struct Case {
    unsigned op, light;
    float s, k, specular, color[3], azimuth, elevation, position[3], points_at[3], spot_exponent, cone_angle;
};

unsigned code_plain(double t) { return t >= 1.0 ? 255u : (unsigned)floor(t * 255.0 + 0.5); }

void plain(const uint8_t* in, int w, int h, const Case& c, unsigned edge, std::vector<uint8_t>& out) {
    out.assign((size_t)w * h * 4, 0);
    const double s = c.s, k = c.k;
    double distant[3] = {0, 0, 0}, axis[3] = {0, 0, 0}, cone_cos = 0.0;
    if (c.light == 0) {
        double sa, ca, se, ce;
        crh_d_sincos((double)c.azimuth * (CRH_PI / 180.0), &sa, &ca);
        crh_d_sincos((double)c.elevation * (CRH_PI / 180.0), &se, &ce);
        distant[0] = ca * ce, distant[1] = sa * ce, distant[2] = se;
    }
    if (c.light == 2) {
        for (int t = 0; t < 3; ++t) axis[t] = (double)c.points_at[t] - (double)c.position[t];
        const double len = sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
        for (int t = 0; t < 3; ++t) axis[t] = axis[t] / len;
        double unused;
        if (c.cone_angle != 0.0f) crh_d_sincos((double)c.cone_angle * (CRH_PI / 180.0), &unused, &cone_cos);
    }
    for (int j = 0; j < h; ++j)
        for (int i = 0; i < w; ++i) {
            long long gx = 0, gy = 0;
            const int weight[3] = {1, 2, 1};
            for (int t = -1; t <= 1; ++t) {
                gx += weight[t + 1] * (alpha_plain(in, w, h, i + 1, j + t, edge) - alpha_plain(in, w, h, i - 1, j + t, edge));
                gy += weight[t + 1] * (alpha_plain(in, w, h, i + t, j + 1, edge) - alpha_plain(in, w, h, i + t, j - 1, edge));
            }
            const double nx = (s * (double)(-gx)) / 1020.0, ny = (s * (double)(-gy)) / 1020.0;
            const double nlen = sqrt((nx * nx + ny * ny) + 1.0);
            double l[3] = {distant[0], distant[1], distant[2]};
            if (c.light != 0) {
                const double d[3] = {(double)c.position[0] - ((double)i + 0.5), (double)c.position[1] - ((double)j + 0.5),
                                     (double)c.position[2] - (s * (double)alpha_plain(in, w, h, i, j, 0)) / 255.0};
                const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
                for (int t = 0; t < 3; ++t) l[t] = len == 0.0 ? 0.0 : d[t] / len;
            }
            double colour[3] = {c.color[0], c.color[1], c.color[2]};
            if (c.light == 2) {
                const double m = -((l[0] * axis[0] + l[1] * axis[1]) + l[2] * axis[2]);
                const bool dark = m <= 0.0 || (c.cone_angle != 0.0f && m < cone_cos);
                const double p = dark ? 0.0 : crh_d_pow(m, (double)c.spot_exponent);
                for (int t = 0; t < 3; ++t) colour[t] = dark ? 0.0 : (double)c.color[t] * p;
            }
            uint8_t* d = out.data() + ((size_t)j * w + i) * 4;
            if (c.op == 0) {
                double q = ((nx * l[0] + ny * l[1]) + l[2]) / nlen;
                if (!(q > 0.0)) q = 0.0;
                const double v = k * q;
                for (int t = 0; t < 3; ++t) d[t] = (uint8_t)code_plain(v * colour[t]);
                d[3] = 255;
            } else {
                const double hz = l[2] + 1.0;
                const double hlen = sqrt((l[0] * l[0] + l[1] * l[1]) + hz * hz);
                double v = 0.0;
                if (hlen != 0.0) {
                    double q = ((nx * l[0] + ny * l[1]) + hz) / (nlen * hlen);
                    if (!(q > 0.0)) q = 0.0;
                    v = k * crh_d_pow(q, (double)c.specular);
                }
                unsigned most = 0;
                for (int t = 0; t < 3; ++t) {
                    const unsigned u = code_plain(v * colour[t]);
                    d[t] = (uint8_t)u;
                    most = u > most ? u : most;
                }
                d[3] = (uint8_t)most;
            }
        }
}

uint32_t seed = 12345u;
uint32_t next() { return seed = seed * 1664525u + 1013904223u, seed >> 8; }

int run(int w, int h, const Case& c, unsigned edge, bool peak, size_t& texels) {
    using namespace crh;
    const size_t n = (size_t)w * h * 4;
    // exact-size heap buffers at an odd address: a read or write past either end is the sanitizer's to see
    uint8_t* in = (uint8_t*)std::malloc(n + 1);
    for (size_t t = 0; t < n; ++t) in[1 + t] = (uint8_t)next();
    if (peak) in[1 + ((size_t)(h / 2) * w + (size_t)(w / 2)) * 4 + 3] = 255; // the texel a light inside the surface sits on
    std::vector<uint8_t> expect;
    plain(in + 1, w, h, c, edge, expect);
    LightingConstants f;
    lighting_prepare(c.op, c.light, c.s, c.k, c.specular, c.color, c.azimuth, c.elevation, c.position, c.points_at, c.spot_exponent, c.cone_angle, &f);
    uint8_t* out = (uint8_t*)std::malloc(n + 3);
    lighting_run(in + 1, (uint32_t)w, (uint32_t)h, f, c.op, c.light, edge, out + 3);
    const int differs = std::memcmp(out + 3, expect.data(), n) != 0;
    if (differs) std::printf("%d x %d op %u light %u edge %u s %g: differs\n", w, h, c.op, c.light, edge, (double)c.s);
    texels += n / 4;
    std::free(in), std::free(out);
    return differs;
}

} // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {3, 2}, {33, 17}};
    const float scales[] = {0.0f, 1.0f, -3.0f, 256.0f};
    size_t texels = 0;
    int failures = 0;
    for (const auto& size : sizes) {
        const float w = (float)size[0], h = (float)size[1];
        for (unsigned op = 0; op < 2; ++op)
            for (unsigned light = 0; light < 3; ++light)
                for (int n = 0; n < 4; ++n) {
                    const Case c = {op, light, scales[n], n == 2 ? 256.0f : 1.25f, n % 2 ? 128.0f : 1.0f, {1.0f, 0.5f, 0.25f}, 225.0f + 90.0f * (float)n, n == 3 ? 90.0f : 35.0f,
                                    {0.3f * w, 0.6f * h, 4.5f}, {0.6f * w, 0.5f * h, 0.0f}, n % 2 ? 0.0f : 128.0f, n < 2 ? 25.0f : n == 2 ? 0.0f : 90.0f};
                    for (unsigned edge = 0; edge < 4; ++edge) failures += run(size[0], size[1], c, edge, false, texels);
                }
        // a light inside the surface: exactly at (i + 0.5, j + 0.5, s A / 255) of the middle texel, whose alpha is 255
        for (unsigned op = 0; op < 2; ++op)
            for (unsigned light = 1; light < 3; ++light) {
                const Case c = {op, light, 2.0f, 1.0f, 2.0f, {1.0f, 1.0f, 1.0f}, 0.0f, 0.0f, {(float)(size[0] / 2) + 0.5f, (float)(size[1] / 2) + 0.5f, 2.0f}, {w, h, -1.0f}, 2.0f, 80.0f};
                for (unsigned edge = 0; edge < 4; ++edge) failures += run(size[0], size[1], c, edge, true, texels);
            }
        // a light below the surface, one at the coordinate limit, and a spot that shines away from the surface
        const Case more[] = {{0, 1, 1.0f, 1.0f, 1.0f, {1.0f, 1.0f, 1.0f}, 0.0f, 0.0f, {0.4f * w, 0.4f * h, -5.0f}, {0.0f, 0.0f, 0.0f}, 0.0f, 0.0f},
                             {1, 1, 1.0f, 256.0f, 128.0f, {1.0f, 1.0f, 1.0f}, 0.0f, 0.0f, {-1048576.0f, 1048576.0f, 1048576.0f}, {0.0f, 0.0f, 0.0f}, 0.0f, 0.0f},
                             {1, 2, -256.0f, 256.0f, 1.0f, {1.0f, 0.0f, 1.0f}, 0.0f, 0.0f, {1048576.0f, -1048576.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 128.0f, 90.0f},
                             {0, 2, 1.0f, 1.0f, 1.0f, {1.0f, 1.0f, 1.0f}, 0.0f, 0.0f, {0.5f * w, 0.5f * h, 3.0f}, {0.5f * w, 0.5f * h, 10.0f}, 1.0f, 0.0f},
                             {1, 0, 256.0f, 256.0f, 128.0f, {1.0f, 1.0f, 1.0f}, -3600.0f, 3600.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f, 0.0f}};
        for (const Case& c : more)
            for (unsigned edge = 0; edge < 4; ++edge) failures += run(size[0], size[1], c, edge, false, texels);
    }
    // the code at its ends
    if (crh::lighting_code(0.0) != 0u || crh::lighting_code(-0.0) != 0u || crh::lighting_code(1.0) != 255u || crh::lighting_code(65536.0) != 255u || crh::lighting_code(0.5) != 128u ||
        crh::lighting_code(0.25) != 64u || crh::lighting_code(0.001) != 0u || crh::lighting_code(0.999) != 255u)
        ++failures;
    std::printf("%zu texels, %d failures\n", texels, failures);
    return failures ? 1 : 0;
}
