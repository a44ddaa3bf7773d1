// csrc/variable_blur.hpp — the rule of crh_image_variable_blur (include/contrast_hip.h states it), written once: the sigma of a mask
// level, the tables that give every level its own tap set, a texel's level, the one multiply-add of a tap and the two roundings.
// k_image_variable_blur_h and k_image_variable_blur_v (image_filter.hip) and crh_variable_blur_texels (image.hip, on the host, through
// variable_blur_run) all read the tables through variable_blur_radius / variable_blur_offset and sum with variable_blur_mad. The taps
// themselves are crh_blur_taps' (image.hip's blur_taps): this header invents no tap rule and takes the function as an argument. All
// values are integers below 2^32: the same bytes on x86-64 and on gfx950. The host's wrap is edge.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "edge.hpp"

namespace crh {

constexpr uint32_t kVariableBlurLevels = 256;    // the codes of a mask's channel
constexpr uint32_t kVariableBlurMaxRadius = 192; // CRH_MAX_BLUR_RADIUS
constexpr uint32_t kVariableBlurTransparent = 0; // CRH_BLUR_EDGE_TRANSPARENT; 1, 2, 3 = PAD, REPEAT, REFLECT

// The sigma of level u <= 255 between s0 (at code 0) and s1 (at code 255): the end points are the caller's floats exactly, the rest is
// one rounding of a double expression evaluated in this order.
inline float variable_blur_sigma(float s0, float s1, uint32_t u) {
    if (u == 0u) return s0;
    if (u == 255u) return s1;
    return (float)((double)s0 + ((double)s1 - (double)s0) * (double)u / 255.0);
}

// One axis of a call: words[u], u < 256, = offset << 8 | radius of level u, then the tap sets as 32-bit words (q[0] reaches 65536):
// level u's q[0 .. radius] lie at words[offset .. offset + radius], offset >= 256. Consecutive levels of one sigma share a set, so a
// constant ramp holds one. At most 256 + 256 * 193 words, so offset < 2^16. `radius` is the largest of the 256.
struct VariableBlurAxis {
    std::vector<uint32_t> words;
    uint32_t radius = 0;
};
__host__ __device__ __forceinline__ uint32_t variable_blur_radius(uint32_t entry) { return entry & 0xFFu; }
__host__ __device__ __forceinline__ uint32_t variable_blur_offset(uint32_t entry) { return entry >> 8; }

// Builds an axis. taps(sigma, q) fills q[0 .. R] by the blur's tap rule and returns 0 on success, anything else is handed back (a sigma
// the rule refuses: the caller has checked s0 and s1, and every level's sigma lies between them). A set that breaks what the kernels
// rely on — R <= 192, q[0] <= 65536, the other taps below 2^16 — is refused with -1 and never met.
template <typename Taps>
inline int variable_blur_axis(float s0, float s1, Taps&& taps, VariableBlurAxis* axis) {
    axis->words.assign(kVariableBlurLevels, 0u);
    axis->radius = 0u;
    std::vector<uint32_t> q;
    float before = 0.0f;
    for (uint32_t u = 0; u < kVariableBlurLevels; ++u) {
        const float sigma = variable_blur_sigma(s0, s1, u);
        if (u != 0u && sigma == before) {
            axis->words[u] = axis->words[u - 1u];
            continue;
        }
        const int st = taps(sigma, q);
        if (st != 0) return st;
        const uint32_t R = (uint32_t)q.size() - 1u;
        if (q.empty() || R > kVariableBlurMaxRadius || q[0] > 65536u) return -1;
        for (uint32_t k = 1; k <= R; ++k)
            if (q[k] > 0xFFFFu) return -1;
        axis->words[u] = (uint32_t)axis->words.size() << 8 | R;
        axis->words.insert(axis->words.end(), q.begin(), q.end());
        if (R > axis->radius) axis->radius = R;
        before = sigma;
    }
    return 0;
}

// The level of a mask texel r | g << 8 | b << 16 | a << 24: the stored code of the channel, shift = 8 * channel
__host__ __device__ __forceinline__ uint32_t variable_blur_level(uint32_t mask_texel, uint32_t shift) { return (mask_texel >> shift) & 0xFFu; }

// Four channels as two words of two 16-bit fields each. acc[0..3] += q * (x.lo, x.hi, y.lo, y.hi): q <= 65536 and a field <= 65280 are
// both below 2^24 (one v_mad_u32_u24 each), and every sum of the rule stays below 2^32.
struct VariableBlurFields {
    uint32_t x, y;
};
__host__ __device__ __forceinline__ void variable_blur_mad(uint32_t acc[4], uint32_t q, VariableBlurFields v) {
#if defined(__HIP_DEVICE_COMPILE__)
    acc[0] += __umul24(q, v.x & 0xFFFFu), acc[1] += __umul24(q, v.x >> 16), acc[2] += __umul24(q, v.y & 0xFFFFu), acc[3] += __umul24(q, v.y >> 16);
#else
    acc[0] += q * (v.x & 0xFFFFu), acc[1] += q * (v.x >> 16), acc[2] += q * (v.y & 0xFFFFu), acc[3] += q * (v.y >> 16);
#endif
}
// The horizontal pass sums a source texel as (r | b << 16, g | a << 16), k_image_blur_h's split, so acc = (r, b, g, a); two texels of one
// tap may be added in their fields first (<= 510).
__host__ __device__ __forceinline__ VariableBlurFields variable_blur_split(uint32_t texel) { return VariableBlurFields{texel & 0x00FF00FFu, (texel >> 8) & 0x00FF00FFu}; }
// t = (sum + 128) >> 8 <= 65280 per channel, as the intermediate's texel (r | g << 16, b | a << 16), k_image_blur_h's
__host__ __device__ __forceinline__ VariableBlurFields variable_blur_intermediate(const uint32_t rbga[4]) {
    return VariableBlurFields{((rbga[0] + 128u) >> 8) | ((rbga[2] + 128u) >> 8) << 16, ((rbga[1] + 128u) >> 8) | ((rbga[3] + 128u) >> 8) << 16};
}
// out = (sum + 2^23) >> 24 per channel of the vertical pass's acc = (r, g, b, a), as a texel
__host__ __device__ __forceinline__ uint32_t variable_blur_texel(const uint32_t rgba[4]) {
    const uint32_t half = 1u << 23;
    return ((rgba[0] + half) >> 24) | ((rgba[1] + half) >> 24) << 8 | ((rgba[2] + half) >> 24) << 16 | ((rgba[3] + half) >> 24) << 24;
}

// The rule on a whole image on the host (crh_variable_blur_texels): w x h texels of `in` under the levels of `mask` (the same size) into
// `out`, which is neither; the caller's bytes at any alignment. Under TRANSPARENT what lies outside is skipped (zero), otherwise the index
// goes through edge.hpp's wrap — every address is formed from a tested or wrapped index, every tap from offset + k, k <= radius.
inline void variable_blur_run(const uint8_t* in, const uint8_t* mask, uint32_t w, uint32_t h, const VariableBlurAxis& ax, const VariableBlurAxis& ay, uint32_t channel, uint32_t edge, uint8_t* out) {
    std::vector<VariableBlurFields> t((size_t)w * h);
    const auto word = [](const uint8_t* s) { return s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24; };
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            const size_t at = (size_t)j * w + i;
            const uint32_t entry = ax.words[mask[at * 4u + channel]];
            const uint32_t* q = ax.words.data() + variable_blur_offset(entry);
            const int R = (int)variable_blur_radius(entry);
            uint32_t acc[4] = {0u, 0u, 0u, 0u};
            for (int k = -R; k <= R; ++k) {
                int s = (int)i + k;
                if (edge == kVariableBlurTransparent) {
                    if ((uint32_t)s >= w) continue;
                } else {
                    s = edge_wrap(s, (int)w, edge);
                }
                variable_blur_mad(acc, q[k < 0 ? -k : k], variable_blur_split(word(in + ((size_t)j * w + (size_t)s) * 4u)));
            }
            t[at] = variable_blur_intermediate(acc);
        }
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            const size_t at = (size_t)j * w + i;
            const uint32_t entry = ay.words[mask[at * 4u + channel]];
            const uint32_t* q = ay.words.data() + variable_blur_offset(entry);
            const int R = (int)variable_blur_radius(entry);
            uint32_t acc[4] = {0u, 0u, 0u, 0u};
            for (int k = -R; k <= R; ++k) {
                int s = (int)j + k;
                if (edge == kVariableBlurTransparent) {
                    if ((uint32_t)s >= h) continue;
                } else {
                    s = edge_wrap(s, (int)h, edge);
                }
                variable_blur_mad(acc, q[k < 0 ? -k : k], t[(size_t)s * w + i]);
            }
            const uint32_t r = variable_blur_texel(acc);
            out[at * 4u] = (uint8_t)r, out[at * 4u + 1u] = (uint8_t)(r >> 8), out[at * 4u + 2u] = (uint8_t)(r >> 16), out[at * 4u + 3u] = (uint8_t)(r >> 24);
        }
}

} // namespace crh
