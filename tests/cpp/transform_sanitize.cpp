// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_transform_cpu.py: a stand-alone
// host program around the rule of csrc/transform.hpp, the code crh_transform_texels runs (no library, no device). It checks the bounds
// the header states for the cubic table over all 256 phases, and runs the rule on heap buffers that end exactly where the images do, one
// byte off alignment — one-texel axes, positions that clamp at +-2^21 texels and read many periods out, a horizon across the result, an
// infinite quotient — under every filter and edge, against a plain restatement in 64-bit integers with its own wrap. An index that left
// an image, a shift of a negative value that is not the arithmetic one, or a sum that overflowed 32 bits would be the sanitizer's to see.
// Exit status 0 = all equal.
#include <transform.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

long long failures = 0, texels = 0;

void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
    if (ok) return;
    ++failures;
    std::printf("FAILED %s (%lld, %lld)\n", what, a, b);
}

long long wrap(long long i, long long n, unsigned edge) { // the image-paint block's wrap, restated
    if (edge == 1u) return i < 0 ? 0 : i >= n ? n - 1 : i;
    const long long p = edge == 2u ? n : 2 * n;
    long long k = i % p;
    if (k < 0) k += p;
    return k < n ? k : p - 1 - k;
}
long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

struct Source {
    const uint8_t* p;
    long long w, h;
    unsigned edge;
    long long at(long long i, long long j, int ch) const {
        if (edge == 0u) {
            if (i < 0 || i >= w || j < 0 || j >= h) return 0;
        } else {
            i = wrap(i, w, edge), j = wrap(j, h, edge);
        }
        return p[(j * w + i) * 4 + ch];
    }
};

void cubic_of(long long F, long long c[4]) {
    const long long W0 = -F * F * F + 512 * F * F - 65536 * F, W2 = -3 * F * F * F + 1024 * F * F + 65536 * F, W3 = F * F * F - 256 * F * F;
    c[0] = floor_div(W0 + 1024, 2048), c[2] = floor_div(W2 + 1024, 2048), c[3] = floor_div(W3 + 1024, 2048), c[1] = 16384 - c[0] - c[2] - c[3];
}

void restated(const Source& s, long long X, long long Y, unsigned filter, uint8_t out[4]) {
    if (filter == 0u) {
        for (int ch = 0; ch < 4; ++ch) out[ch] = (uint8_t)s.at(floor_div(X, 256), floor_div(Y, 256), ch);
        return;
    }
    const long long ax = X - 128, ay = Y - 128, i0 = floor_div(ax, 256), j0 = floor_div(ay, 256), fx = ax - 256 * i0, fy = ay - 256 * j0;
    long long value[4];
    for (int ch = 0; ch < 4; ++ch) {
        if (filter == 1u) {
            const long long top = s.at(i0, j0, ch) * (256 - fx) + s.at(i0 + 1, j0, ch) * fx, bottom = s.at(i0, j0 + 1, ch) * (256 - fx) + s.at(i0 + 1, j0 + 1, ch) * fx;
            value[ch] = (top * (256 - fy) + bottom * fy + 32768) / 65536;
        } else {
            long long cx[4], cy[4], sum = 0;
            cubic_of(fx, cx), cubic_of(fy, cy);
            for (int r = 0; r < 4; ++r) {
                long long row = 0;
                for (int k = 0; k < 4; ++k) row += cx[k] * s.at(i0 - 1 + k, j0 - 1 + r, ch);
                sum += cy[r] * floor_div(row + 32, 64);
            }
            const long long v = floor_div(sum + 2097152, 4194304);
            value[ch] = v < 0 ? 0 : v > 255 ? 255 : v;
        }
    }
    if (filter == 2u)
        for (int ch = 0; ch < 3; ++ch) value[ch] = value[ch] < value[3] ? value[ch] : value[3];
    for (int ch = 0; ch < 4; ++ch) out[ch] = (uint8_t)value[ch];
}

void check_table() {
    static constexpr crh::TransformCubicTable table{};
    long long h_lo = 0, h_hi = 0, numerator = 0;
    for (int F = 0; F < 256; ++F) {
        long long c[4], positive = 0, negative = 0;
        cubic_of(F, c);
        for (int k = 0; k < 4; ++k) {
            expect(table.c[F][k] == c[k], "a weight of the table", F, k);
            expect(c[k] >= -1214 && c[k] <= 16384, "a weight's range", F, c[k]);
            (c[k] > 0 ? positive : negative) += c[k];
        }
        expect(positive + negative == 16384 && positive <= 18432 && -negative <= 2048, "a phase's sums", positive, negative);
        const long long lo = floor_div(255 * negative + 32, 64), hi = floor_div(255 * positive + 32, 64);
        h_lo = lo < h_lo ? lo : h_lo, h_hi = hi > h_hi ? hi : h_hi;
    }
    expect(h_lo >= -8161 && h_hi == 73440, "the range of h", h_lo, h_hi);
    for (int F = 0; F < 256; ++F) {
        long long c[4], bound = 0;
        cubic_of(F, c);
        for (int k = 0; k < 4; ++k) bound += c[k] > 0 ? c[k] * 73440 : c[k] * -8161; // (the header's range of h)
        numerator = bound > numerator ? bound : numerator;
    }
    expect(numerator + 2097152 <= 1372456960 && numerator + 2097152 < 2147483648ll, "the second numerator", numerator);
    // a constant image comes back exactly at every phase pair
    for (int Fx = 0; Fx < 256; ++Fx)
        for (int Fy = 0; Fy < 256; ++Fy) {
            uint32_t s[16];
            for (uint32_t& v : s) v = 0xC9FF0107u;
            expect(crh::transform_cubic_blend(s, table.c[Fx], table.c[Fy]) == 0xC9C90107u, "a constant image", Fx, Fy); // (b = 255 above a = 201 clamps to a)
        }
}

void check_image(unsigned sw, unsigned sh, unsigned w, unsigned h, const double m[9], unsigned seed) {
    std::vector<uint8_t> in_heap((size_t)sw * sh * 4 + 1), out_heap((size_t)w * h * 4 + 1);
    uint8_t *in = in_heap.data() + 1, *out = out_heap.data() + 1;
    std::srand(seed);
    for (size_t k = 0; k < (size_t)sw * sh * 4; ++k) in[k] = (uint8_t)(std::rand() >> 7);
    crh::TransformConstants f;
    for (int k = 0; k < 9; ++k) f.m[k] = m[k];
    f.projective = crh::transform_is_affine(m) ? 0u : 1u;
    for (unsigned filter = 0; filter < 3u; ++filter)
        for (unsigned edge = 0; edge < 4u; ++edge) {
            f.filter = filter, f.edge = edge;
            if (f.projective) {
                if (filter == 0u) crh::transform_run<0u, true>(in, sw, sh, f, w, h, out);
                else if (filter == 1u) crh::transform_run<1u, true>(in, sw, sh, f, w, h, out);
                else crh::transform_run<2u, true>(in, sw, sh, f, w, h, out);
            } else {
                if (filter == 0u) crh::transform_run<0u, false>(in, sw, sh, f, w, h, out);
                else if (filter == 1u) crh::transform_run<1u, false>(in, sw, sh, f, w, h, out);
                else crh::transform_run<2u, false>(in, sw, sh, f, w, h, out);
            }
            const Source s{in, (long long)sw, (long long)sh, edge};
            for (unsigned j = 0; j < h; ++j)
                for (unsigned i = 0; i < w; ++i) {
                    const double u = (double)i + 0.5, v = (double)j + 0.5;
                    double px = (m[0] * u + m[1] * v) + m[2], py = (m[3] * u + m[4] * v) + m[5];
                    uint8_t want[4] = {0, 0, 0, 0};
                    bool visible = true;
                    if (f.projective) {
                        const double ws = (m[6] * u + m[7] * v) + m[8];
                        visible = ws > 0.0;
                        if (visible) px = px / ws, py = py / ws;
                    }
                    if (visible) {
                        px = px < -2097152.0 ? -2097152.0 : px > 2097152.0 ? 2097152.0 : px, py = py < -2097152.0 ? -2097152.0 : py > 2097152.0 ? 2097152.0 : py;
                        restated(s, (long long)std::floor(px * 256.0 + 0.5), (long long)std::floor(py * 256.0 + 0.5), filter, want);
                    }
                    const uint8_t* got = out + ((size_t)j * w + i) * 4;
                    expect(got[0] == want[0] && got[1] == want[1] && got[2] == want[2] && got[3] == want[3], "a texel", (long long)(filter * 4 + edge), (long long)j * w + i);
                    ++texels;
                }
        }
}

} // namespace

int main() {
    check_table();
    const double turn[9] = {0.8660254037844387, -0.5, 3.25, 0.5, 0.8660254037844387, -2.5, 0, 0, 1};
    const double far_away[9] = {1, 0, 3e6, 0, 1, -3e6, 0, 0, 1};
    const double huge[9] = {1099511627776.0, -1099511627776.0, 0.25, 1e-300, 0, -1099511627776.0, 0, 0, 1};
    const double horizon[9] = {1.1, 0.1, 0, -0.05, 0.9, 0.3, -0.1, -0.1, 1};
    const double tiny_w[9] = {1, 0, 0, 0, -1, 0, 0, 0, 5e-324}; // the quotients are infinite: they clamp
    const double point[9] = {0, 0, 2.3, 0, 0, 1.7, 0, 0, 1};
    const double* all[6] = {turn, far_away, huge, horizon, tiny_w, point};
    const unsigned sizes[5][4] = {{1, 1, 9, 7}, {1, 5, 6, 9}, {7, 1, 9, 4}, {13, 9, 11, 12}, {4, 3, 1, 1}}; // source w, h, result w, h
    unsigned seed = 1;
    for (const double* m : all)
        for (const unsigned* size : sizes) check_image(size[0], size[1], size[2], size[3], m, seed++);
    std::printf("%lld texels, %lld failures\n", texels, failures);
    return failures == 0 ? 0 : 1;
}
