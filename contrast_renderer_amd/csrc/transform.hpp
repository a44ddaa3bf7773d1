// csrc/transform.hpp — the rule of crh_image_transform (include/contrast_hip.h states it), written once: the position of a result texel in
// the source (binary64 in a fixed order, as lighting and turbulence compute), the Catmull-Rom weights and the 4 x 4 blend of CUBIC, and
// transform_texel, which puts displace.hpp's displace_texel (NEAREST, LINEAR) or the cubic blend around a texel-fetch functor.
// k_image_transform (image_filter.hip) and crh_transform_texels (image.hip, on the host, through transform_run) both call
// transform_position, displace_taps / displace_blend and transform_cubic_blend; the kernel issues its fetches itself, before the first
// blend. The position uses + * / comparisons and floor only and is compiled without contraction (-ffp-contract=off, as the whole library
// is), so x86-64 and gfx950 give the same X and Y; everything behind them is 32-bit integer. The host's wrap is edge.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "displace.hpp"
#include "edge.hpp"

namespace crh {

constexpr uint32_t kTransformNearest = 0, kTransformLinear = 1, kTransformCubic = 2; // crh_transform_filter; the first two are displace's
constexpr uint32_t kTransformTransparent = 0;                                        // CRH_BLUR_EDGE_TRANSPARENT; 1, 2, 3 = PAD, REPEAT, REFLECT
constexpr double kTransformMaxEntry = 1099511627776.0;                               // CRH_MAX_TRANSFORM_ENTRY, 2^40
constexpr double kTransformMaxPosition = 2097152.0;                                  // 2^21 texels: what a position is clamped to
static_assert(kTransformNearest == kDisplaceNearest && kTransformLinear == kDisplaceLinear && kTransformTransparent == kDisplaceTransparent, "NEAREST and LINEAR are displace's");

// What a call is after validation, for the host rule and the kernel alike (a kernel argument, by value)
struct TransformConstants {
    double m[9];         // result (x, y, 1) -> source, row-major; finite, |.| <= 2^40
    uint32_t filter;     // kTransformNearest, kTransformLinear or kTransformCubic
    uint32_t edge;       // crh_blur_edge: what the source is outside itself
    uint32_t projective; // 0 when m6 == 0 && m7 == 0 && m8 == 1: no division, every texel visible
};
__host__ __device__ __forceinline__ bool transform_is_affine(const double* m) { return m[6] == 0.0 && m[7] == 0.0 && m[8] == 1.0; }

// p texels -> 1/256 texel: clamped by comparisons to +-2^21 (an infinite quotient clamps; no NaN reaches this: see the header), then
// floor(p * 256 + 0.5), |.| <= 2^29
__host__ __device__ __forceinline__ int32_t transform_fixed(double p) {
    p = p < -kTransformMaxPosition ? -kTransformMaxPosition : p > kTransformMaxPosition ? kTransformMaxPosition : p;
    return (int32_t)floor(p * 256.0 + 0.5);
}

// Result texel (i, j) -> (X, Y) in 1/256 source texel, and whether the texel is visible (ws > 0; always when !PROJECTIVE). An invisible
// texel gets (0, 0), which nothing reads. Every product and sum is written as the header writes it; |m u| <= 2^40 * 2^15: no overflow.
template <bool PROJECTIVE>
__host__ __device__ __forceinline__ bool transform_position(const double* m, uint32_t i, uint32_t j, int32_t* X, int32_t* Y) {
    const double u = (double)i + 0.5, v = (double)j + 0.5;
    double px = (m[0] * u + m[1] * v) + m[2], py = (m[3] * u + m[4] * v) + m[5];
    bool visible = true;
    if (PROJECTIVE) {
        const double ws = (m[6] * u + m[7] * v) + m[8];
        visible = ws > 0.0;
        const double d = visible ? ws : 1.0; // (no branch: an invisible lane divides by 1 and its position is dropped)
        px = px / d, py = py / d;
    }
    *X = visible ? transform_fixed(px) : 0, *Y = visible ? transform_fixed(py) : 0;
    return visible;
}

// The Catmull-Rom weights of the phase F (of 256) over 16384, for the texels i0 - 1 .. i0 + 2: the integer statement of the header.
// W over 2^25 from the cubic polynomials with t = F / 256; c_k = (W_k + 1024) >> 11 for k = 0, 2, 3 and c_1 the rest of 16384.
__host__ __device__ constexpr void transform_cubic_weights(int32_t F, int32_t c[4]) {
    const int32_t F2 = F * F, F3 = F2 * F; // F <= 255: F3 < 2^24
    const int32_t W0 = -F3 + 512 * F2 - 65536 * F, W2 = -3 * F3 + 1024 * F2 + 65536 * F, W3 = F3 - 256 * F2;
    // (x + 1024) >> 11 as a floor division that is constexpr for negative x too: x + 1024 + 2^26 >= 0
    c[0] = (W0 + 1024 + 67108864) / 2048 - 32768, c[2] = (W2 + 1024 + 67108864) / 2048 - 32768, c[3] = (W3 + 1024 + 67108864) / 2048 - 32768;
    c[1] = 16384 - c[0] - c[2] - c[3];
}
// The 256 x 4 table of them, 16 bits each (-1214 <= c <= 16384), one phase's four in 8 bytes: a constant on the host, staged in LDS by the kernel
struct TransformCubicTable {
    alignas(8) int16_t c[256][4];
    constexpr TransformCubicTable() : c{} {
        for (int32_t F = 0; F < 256; ++F) {
            int32_t w[4] = {0, 0, 0, 0};
            transform_cubic_weights(F, w);
            for (int k = 0; k < 4; ++k) c[F][k] = (int16_t)w[k];
        }
    }
};

// What a CUBIC position reads: the 4 x 4 texels (i0 - 1, j0 - 1) .. (i0 + 2, j0 + 2) and the phases
struct TransformCubicTaps {
    int32_t i0, j0;
    uint32_t fx, fy;
};
__host__ __device__ __forceinline__ TransformCubicTaps transform_cubic_taps(int32_t X, int32_t Y) {
    const int32_t ax = X - 128, ay = Y - 128;
    return TransformCubicTaps{ax >> 8, ay >> 8, (uint32_t)ax & 255u, (uint32_t)ay & 255u};
}
// The value of s[4 r + k] = S(i0 - 1 + k, j0 - 1 + r) under the weights cx (of fx) and cy (of fy): per channel h_r = (sum_k cx_k s + 32) >> 6
// in [-8161, 73440], value = clamp((sum_r cy_r h_r + 2^21) >> 22, 0, 255), the numerator below 2^31 in magnitude; then rgb = min(rgb, a).
// The shifts are arithmetic.
__host__ __device__ __forceinline__ uint32_t transform_cubic_blend(const uint32_t* s, const int16_t* cx, const int16_t* cy) {
    uint32_t value[4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        int32_t sum = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int32_t row = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) row += (int32_t)cx[k] * (int32_t)((s[4 * r + k] >> (8 * ch)) & 0xFFu);
            sum += (int32_t)cy[r] * ((row + 32) >> 6);
        }
        const int32_t v = (sum + 2097152) >> 22;
        value[ch] = (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
    const uint32_t a = value[3];
    return (value[0] < a ? value[0] : a) | (value[1] < a ? value[1] : a) << 8 | (value[2] < a ? value[2] : a) << 16 | a << 24;
}

// (X, Y) and S -> the result texel of a visible position. S(i, j) is the source's texel at any int32 indices: the edge is the functor's.
template <uint32_t FILTER, typename Fetch>
__host__ __device__ __forceinline__ uint32_t transform_texel(int32_t X, int32_t Y, const TransformCubicTable& table, Fetch&& S) {
    if constexpr (FILTER != kTransformCubic) {
        return displace_texel<FILTER>(X, Y, S);
    } else {
        const TransformCubicTaps t = transform_cubic_taps(X, Y);
        uint32_t s[16];
        for (int r = 0; r < 4; ++r)
            for (int k = 0; k < 4; ++k) s[4 * r + k] = S(t.i0 - 1 + k, t.j0 - 1 + r);
        return transform_cubic_blend(s, table.c[t.fx], table.c[t.fy]);
    }
}

// The rule on a whole image on the host (crh_transform_texels): sw x sh texels of `in` -> w x h texels of `out`, which is not `in`; the
// caller's bytes at any alignment, a texel's word assembled from its four bytes in memory order, r first. S is displace_run's: under
// TRANSPARENT zero when either index is outside, otherwise the texel at edge.hpp's wrap of each index — every address is formed from a
// tested or wrapped index.
template <uint32_t FILTER, bool PROJECTIVE>
inline void transform_run(const uint8_t* in, uint32_t sw, uint32_t sh, const TransformConstants& f, uint32_t w, uint32_t h, uint8_t* out) {
    static constexpr TransformCubicTable table{};
    const uint32_t edge = f.edge;
    const auto S = [&](int32_t i, int32_t j) -> uint32_t {
        if (edge == kTransformTransparent) {
            if ((uint32_t)i >= sw || (uint32_t)j >= sh) return 0u;
        } else {
            i = edge_wrap(i, (int)sw, edge), j = edge_wrap(j, (int)sh, edge);
        }
        const uint8_t* s = in + ((size_t)j * sw + (size_t)i) * 4u;
        return s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
    };
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            int32_t X, Y;
            const uint32_t r = transform_position<PROJECTIVE>(f.m, i, j, &X, &Y) ? transform_texel<FILTER>(X, Y, table, S) : 0u;
            const size_t at = ((size_t)j * w + i) * 4u;
            out[at] = (uint8_t)r, out[at + 1u] = (uint8_t)(r >> 8), out[at + 2u] = (uint8_t)(r >> 16), out[at + 3u] = (uint8_t)(r >> 24);
        }
}

} // namespace crh
