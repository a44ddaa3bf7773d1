// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_variable_blur_cpu.py: a
// stand-alone host program around the rule of csrc/variable_blur.hpp, the code crh_variable_blur_texels runs (no library, no device).
// The tap rule is an argument of that header, so this program brings its own: any symmetric set that sums to 65536 serves, here a
// triangle of radius ceil(3 sigma), with q[0] = 65536 alone at sigma 0. It checks what the tables promise (every level's entry inside
// the words, the radius within 192, each set summing to 65536) and runs the rule on heap buffers that end exactly where the images do,
// one byte off alignment — a one-texel axis under each edge at radius 192, noise masks, a mask that is the source — against a plain
// restatement of the two sums in 64-bit integers. An index that left an image or a table, or a sum that overflowed 32 bits, would be
// the sanitizer's to see. Exit status 0 = all equal.
#include <variable_blur.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

long long failures = 0, texels = 0;

void expect(bool ok, const char* what, unsigned w, unsigned h, unsigned edge) {
    if (ok) return;
    ++failures;
    std::printf("FAILED %s: %u x %u, edge %u\n", what, w, h, edge);
}

int triangle_taps(float sigma, std::vector<uint32_t>& q) {
    const uint32_t R = (uint32_t)std::ceil(3.0 * (double)sigma);
    q.assign(R + 1u, 0u);
    uint32_t rest = 65536u;
    for (uint32_t k = R; k >= 1u; --k) {
        q[k] = 65536u * (R + 1u - k) / ((R + 1u) * (R + 1u));
        rest -= 2u * q[k];
    }
    q[0] = rest;
    return 0;
}

int wrap(long long i, long long n, unsigned edge) { // the image-paint block's wrap, restated
    if (edge == 1u) return (int)(i < 0 ? 0 : i >= n ? n - 1 : i);
    const long long p = edge == 2u ? n : 2 * n;
    long long k = i % p;
    if (k < 0) k += p;
    return (int)(k < n ? k : p - 1 - k);
}

void check_axis(const crh::VariableBlurAxis& axis, unsigned w, unsigned h) {
    expect(axis.words.size() >= 256u + 1u && axis.radius <= 192u, "the axis", w, h, 9u);
    for (unsigned u = 0; u < 256u; ++u) {
        const uint32_t R = crh::variable_blur_radius(axis.words[u]), at = crh::variable_blur_offset(axis.words[u]);
        expect(R <= axis.radius && at >= 256u && (size_t)at + R < axis.words.size(), "a level's entry", w, h, u);
        if ((size_t)at + R >= axis.words.size()) continue;
        long long sum = axis.words[at];
        for (uint32_t k = 1; k <= R; ++k) sum += 2ll * axis.words[at + k];
        expect(sum == 65536, "a level's taps sum to 65536", w, h, u);
    }
}

void check_image(unsigned w, unsigned h, const float sx[2], const float sy[2], unsigned channel, unsigned edge, unsigned seed, bool own_mask) {
    crh::VariableBlurAxis ax, ay;
    if (crh::variable_blur_axis(sx[0], sx[1], triangle_taps, &ax) != 0 || crh::variable_blur_axis(sy[0], sy[1], triangle_taps, &ay) != 0) {
        expect(false, "an axis is refused", w, h, edge);
        return;
    }
    check_axis(ax, w, h), check_axis(ay, w, h);
    // heap buffers that end exactly where the images do, one byte off alignment
    const size_t bytes = (size_t)w * h * 4u;
    std::vector<uint8_t> raw_in(bytes + 1u), raw_mask(bytes + 1u), raw_out(bytes + 1u);
    uint8_t* in = raw_in.data() + 1;
    uint8_t* mask = own_mask ? in : raw_mask.data() + 1;
    uint8_t* out = raw_out.data() + 1;
    uint32_t state = seed * 2654435761u + 1u;
    for (size_t k = 0; k < bytes; ++k) {
        state = state * 1664525u + 1013904223u;
        in[k] = (uint8_t)(state >> 24);
        if (!own_mask) mask[k] = (state >> 9) % 5u == 0u ? 255u : (state >> 9) % 5u == 1u ? 0u : (uint8_t)(state >> 13);
    }
    crh::variable_blur_run(in, mask, w, h, ax, ay, channel, edge, out);
    const auto taps = [](const crh::VariableBlurAxis& axis, unsigned u, long long* R) {
        *R = crh::variable_blur_radius(axis.words[u]);
        return axis.words.data() + crh::variable_blur_offset(axis.words[u]);
    };
    std::vector<long long> t((size_t)w * h * 4u);
    for (unsigned j = 0; j < h; ++j)
        for (unsigned i = 0; i < w; ++i) {
            long long R;
            const uint32_t* q = taps(ax, mask[((size_t)j * w + i) * 4u + channel], &R);
            for (unsigned c = 0; c < 4u; ++c) {
                long long sum = 0;
                for (long long k = -R; k <= R; ++k) {
                    const long long s = (long long)i + k;
                    if (edge == 0u && (s < 0 || s >= (long long)w)) continue;
                    sum += (long long)q[k < 0 ? -k : k] * in[((size_t)j * w + (size_t)(edge == 0u ? s : wrap(s, w, edge))) * 4u + c];
                }
                t[((size_t)j * w + i) * 4u + c] = (sum + 128) >> 8;
                if (t[((size_t)j * w + i) * 4u + c] > 65280) expect(false, "t exceeds 65280", w, h, edge);
            }
        }
    for (unsigned j = 0; j < h; ++j)
        for (unsigned i = 0; i < w; ++i) {
            long long R;
            const uint32_t* q = taps(ay, mask[((size_t)j * w + i) * 4u + channel], &R);
            for (unsigned c = 0; c < 4u; ++c) {
                long long sum = 0;
                for (long long k = -R; k <= R; ++k) {
                    const long long s = (long long)j + k;
                    if (edge == 0u && (s < 0 || s >= (long long)h)) continue;
                    sum += (long long)q[k < 0 ? -k : k] * t[((size_t)(edge == 0u ? s : wrap(s, h, edge)) * w + i) * 4u + c];
                }
                if (sum + (1ll << 23) >= (1ll << 32)) expect(false, "the vertical sum leaves 32 bits", w, h, edge);
                if (out[((size_t)j * w + i) * 4u + c] != (uint8_t)((sum + (1ll << 23)) >> 24)) expect(false, "a byte", w, h, edge);
            }
            ++texels;
        }
}

} // namespace

int main() {
    const float wide[2] = {0.0f, 64.0f}, back[2] = {64.0f, 0.0f}, small[2] = {0.3f, 2.5f}, same[2] = {3.0f, 3.0f}, none[2] = {0.0f, 0.0f}, tiny[2] = {0.0f, 0.01f};
    unsigned seed = 1;
    for (unsigned edge = 0; edge < 4u; ++edge) {
        // a one-texel axis, and a whole one-texel image, at radius 192: the index wraps many times over
        check_image(1, 1, wide, back, 3, edge, seed++, false), check_image(1, 40, wide, wide, 0, edge, seed++, false), check_image(40, 1, back, wide, 1, edge, seed++, false);
        // noise masks: every texel its own level
        check_image(37, 21, wide, back, 2, edge, seed++, false), check_image(64, 5, small, same, 3, edge, seed++, false), check_image(5, 64, none, small, 0, edge, seed++, false);
        check_image(19, 23, tiny, tiny, 1, edge, seed++, false), check_image(33, 9, same, none, 3, edge, seed++, false);
        // the source as its own mask
        check_image(23, 17, small, wide, 3, edge, seed++, true);
    }
    std::printf("%lld texels, %lld failures\n", texels, failures);
    return failures == 0 ? 0 : 1;
}
