// csrc/displace.hpp — the displacement rule of crh_image_displace (include/contrast_hip.h states it), written once: the one conversion of a
// scale to K, the offsets (qx, qy) of a map texel, the taps of a position, the blend of the fetched texels, and displace_texel, which puts
// the last two around a texel-fetch functor. k_image_displace (image_filter.hip) and crh_displace_texels (image.hip, on the host, through
// displace_run) both call displace_offsets, displace_taps and displace_blend; the host goes through displace_texel, the kernel calls its
// two halves itself so that every fetch of a lane's rows is issued before the first blend. All values are 8-bit codes and all arithmetic
// is 32-bit integer: the same bytes on x86-64 and on gfx950. The map's unpremultiply is color_filter.hpp's, the host's wrap edge.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "color_filter.hpp"
#include "edge.hpp"

namespace crh {

constexpr float kDisplaceMaxScale = 1024.0f;                   // CRH_MAX_DISPLACE_SCALE
constexpr uint32_t kDisplaceNearest = 0, kDisplaceLinear = 1;  // CRH_FILTER_NEAREST, CRH_FILTER_LINEAR
constexpr uint32_t kDisplaceAlpha = 3;                         // CRH_CHANNEL_A
constexpr uint32_t kDisplaceTransparent = 0;                   // CRH_BLUR_EDGE_TRANSPARENT; 1, 2, 3 = PAD, REPEAT, REFLECT

// What a call is after validation, for the host rule and the kernel alike (a kernel argument, by value): K per axis, the map's channels
// that move x and y, the filter and the edge.
struct DisplaceConstants {
    int32_t k[2];        // floor((double) scale * 256 + 0.5), |k| <= 2^18
    uint32_t channel[2]; // crh_channel of x and y
    uint32_t filter;     // kDisplaceNearest or kDisplaceLinear
    uint32_t edge;       // crh_blur_edge: what the source is outside itself
};

// The one place where a scale becomes K (finite, |scale| <= kDisplaceMaxScale: the caller has checked)
inline int32_t displace_k(float scale) { return (int32_t)std::floor((double)scale * 256.0 + 0.5); }

// q = floor((K (2 u - 255) + 255) / 510) for a straight code u <= 255, in units of 1/256 texel: scale (u / 255 - 1/2) rounded half up.
// |n| <= 2^18 * 255, so n + 255 + 510 * 2^17 >= 255: the floor of a negative numerator is an unsigned division and a subtraction.
__host__ __device__ __forceinline__ int32_t displace_q(int32_t k, uint32_t u) {
    const int32_t n = color_filter_mul(k, 2 * (int32_t)u - 255);
    return (int32_t)((uint32_t)(n + 255 + 510 * 131072) / 510u) - 131072;
}

// The straight code of one channel of a map texel (r | g << 8 | b << 16 | a << 24), loaded as the colour filter loads it: the alpha as it
// is, a colour min(c, a) unpremultiplied, 0 for a == 0 (`recip` = UnpremultiplyTable::r, whose entry 0 is 0)
__host__ __device__ __forceinline__ uint32_t displace_code(uint32_t texel, uint32_t channel, const uint32_t* recip) {
    const uint32_t a = texel >> 24;
    return channel == kDisplaceAlpha ? a : color_filter_unpremultiply((texel >> (8u * channel)) & 0xFFu, a, recip[a]);
}

// map texel -> (qx, qy)
__host__ __device__ __forceinline__ void displace_offsets(uint32_t map_texel, const DisplaceConstants& f, const uint32_t* recip, int32_t q[2]) {
    q[0] = displace_q(f.k[0], displace_code(map_texel, f.channel[0], recip));
    q[1] = displace_q(f.k[1], displace_code(map_texel, f.channel[1], recip));
}

// The position of texel (i, j) moved by q, in 1/256 texel: the texel's centre plus the offset, |.| < 2^23
__host__ __device__ __forceinline__ int32_t displace_position(uint32_t i, int32_t q) { return 256 * (int32_t)i + 128 + q; }

// What a position reads: NEAREST the texel (i0, j0) that holds it; LINEAR the four texels (i0, j0) .. (i0 + 1, j0 + 1) around it, with
// the weights fx and fy (of 256) of the right column and the lower row. The shifts are arithmetic.
struct DisplaceTaps {
    int32_t i0, j0;
    uint32_t fx, fy;
};
template <uint32_t FILTER>
__host__ __device__ __forceinline__ DisplaceTaps displace_taps(int32_t X, int32_t Y) {
    if (FILTER == kDisplaceNearest) return DisplaceTaps{X >> 8, Y >> 8, 0u, 0u};
    const int32_t ax = X - 128, ay = Y - 128;
    return DisplaceTaps{ax >> 8, ay >> 8, (uint32_t)ax & 255u, (uint32_t)ay & 255u};
}

// The value of the taps' texels s[0] = S(i0, j0), and under LINEAR s[1] = S(i0 + 1, j0), s[2] = S(i0, j0 + 1), s[3] = S(i0 + 1, j0 + 1):
// per channel top = s0 (256 - fx) + s1 fx, bottom the same of s2 and s3, (top (256 - fy) + bottom fy + 32768) >> 16: one rounding, the
// numerator <= 255 * 65536 + 32768 < 2^24. The rows are blended two channels to a word (r | b << 16 and g | a << 16: a row's value is
// <= 255 * 256 < 2^16, so the fields do not meet), the columns per channel.
template <uint32_t FILTER>
__host__ __device__ __forceinline__ uint32_t displace_blend(const uint32_t* s, const DisplaceTaps& t) {
    if (FILTER == kDisplaceNearest) return s[0];
    const uint32_t gx = 256u - t.fx, gy = 256u - t.fy;
    const uint32_t top_rb = (s[0] & 0x00FF00FFu) * gx + (s[1] & 0x00FF00FFu) * t.fx, top_ga = ((s[0] >> 8) & 0x00FF00FFu) * gx + ((s[1] >> 8) & 0x00FF00FFu) * t.fx;
    const uint32_t bottom_rb = (s[2] & 0x00FF00FFu) * gx + (s[3] & 0x00FF00FFu) * t.fx, bottom_ga = ((s[2] >> 8) & 0x00FF00FFu) * gx + ((s[3] >> 8) & 0x00FF00FFu) * t.fx;
    const uint32_t r = ((top_rb & 0xFFFFu) * gy + (bottom_rb & 0xFFFFu) * t.fy + 32768u) >> 16;
    const uint32_t g = ((top_ga & 0xFFFFu) * gy + (bottom_ga & 0xFFFFu) * t.fy + 32768u) >> 16;
    const uint32_t b = ((top_rb >> 16) * gy + (bottom_rb >> 16) * t.fy + 32768u) >> 16;
    const uint32_t a = ((top_ga >> 16) * gy + (bottom_ga >> 16) * t.fy + 32768u) >> 16;
    return r | g << 8 | b << 16 | a << 24;
}

// (X, Y) and S -> the result texel. S(i, j) is the source's texel at any int32 indices: the edge is the functor's.
template <uint32_t FILTER, typename Fetch>
__host__ __device__ __forceinline__ uint32_t displace_texel(int32_t X, int32_t Y, Fetch&& S) {
    const DisplaceTaps t = displace_taps<FILTER>(X, Y);
    uint32_t s[4] = {S(t.i0, t.j0), 0u, 0u, 0u};
    if (FILTER == kDisplaceLinear) s[1] = S(t.i0 + 1, t.j0), s[2] = S(t.i0, t.j0 + 1), s[3] = S(t.i0 + 1, t.j0 + 1);
    return displace_blend<FILTER>(s, t);
}

// The rule on a whole image on the host (crh_displace_texels): w x h texels of `in` through the map `map` of the same size into `out`,
// which is neither of them; the caller's bytes at any alignment, a texel's word assembled from its four bytes in memory order, r first.
// S: under TRANSPARENT zero when either index is outside, otherwise the texel at edge.hpp's wrap of each index — every address is
// formed from a tested or wrapped index.
template <uint32_t FILTER>
inline void displace_run(const uint8_t* in, const uint8_t* map, uint32_t w, uint32_t h, const DisplaceConstants& f, uint8_t* out) {
    static constexpr UnpremultiplyTable recip{};
    const uint32_t edge = f.edge;
    const auto word = [](const uint8_t* s) { return s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24; };
    const auto S = [&](int32_t i, int32_t j) -> uint32_t {
        if (edge == kDisplaceTransparent) {
            if ((uint32_t)i >= w || (uint32_t)j >= h) return 0u;
        } else {
            i = edge_wrap(i, (int)w, edge), j = edge_wrap(j, (int)h, edge);
        }
        return word(in + ((size_t)j * w + (size_t)i) * 4u);
    };
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            const size_t at = ((size_t)j * w + i) * 4u;
            int32_t q[2];
            displace_offsets(word(map + at), f, recip.r, q);
            const uint32_t r = displace_texel<FILTER>(displace_position(i, q[0]), displace_position(j, q[1]), S);
            out[at] = (uint8_t)r, out[at + 1u] = (uint8_t)(r >> 8), out[at + 2u] = (uint8_t)(r >> 16), out[at + 3u] = (uint8_t)(r >> 24);
        }
}

} // namespace crh
