// csrc/distance.hpp — the distance rule of crh_image_distance_field (include/contrast_hip.h states it), written once: the inside test of a
// texel, the target of a mode (what a distance is measured to), the thresholds that turn a squared distance into its code c(D2), and the
// scan along a row of column distances. k_image_distance_v and k_image_distance_h (image_filter.hip) and crh_distance_texels (image.hip,
// on the host, through distance_run) all call distance_target, distance_scan and distance_code. Everything is integer: squared distances
// between texel centres are integers, and the one rounding is the integer statement (2 c - 1)^2 spread^2 <= 260100 D2, taken in 64 bits
// on the host where the 255 thresholds of a spread are made. The same bytes on x86-64 and on gfx950. The wrap is edge.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "edge.hpp"

namespace crh {

constexpr uint32_t kDistanceMaxSpread = 255;                   // CRH_MAX_DISTANCE_SPREAD
constexpr uint32_t kDistanceOutside = 0, kDistanceInside = 1;  // crh_distance_mode
constexpr uint32_t kDistanceTransparent = 0;                   // CRH_BLUR_EDGE_TRANSPARENT; 1, 2, 3 = PAD, REPEAT, REFLECT
constexpr uint32_t kDistanceNone = 255;                        // a column distance g: nothing within reach (a g that counts is <= spread - 1 <= 254)

// What a call is after validation, for the host rule and the kernels alike (a kernel argument, by value)
struct DistanceConstants {
    uint32_t mode;      // kDistanceOutside or kDistanceInside
    uint32_t shift;     // 8 * crh_channel: the stored code of the channel is (texel >> shift) & 255
    uint32_t threshold; // 1..255
    uint32_t spread;    // 1..kDistanceMaxSpread
    uint32_t edge;      // crh_blur_edge
};

// The thresholds of a spread: t[c], c = 1..255, is the least D2 whose code is at least c, ceil((2 c - 1)^2 spread^2 / 260100), and
// t[0] = 0. They rise with c, so c(D2) is the number of c >= 1 with t[c] <= D2: the largest c with (2 c - 1)^2 spread^2 <= 260100 D2, a
// tie (equality) included. t[1] = 1 (spread^2 <= 65025 < 260100) and t[255] <= spread^2 (509^2 < 260100).
struct DistanceThresholds {
    uint32_t t[256];
};
inline void distance_thresholds(uint32_t spread, DistanceThresholds* into) {
    into->t[0] = 0u;
    for (uint64_t c = 1; c < 256; ++c) {
        const uint64_t n = (2u * c - 1u) * (2u * c - 1u) * (uint64_t)spread * spread; // < 2^35
        into->t[c] = (uint32_t)((n + 260099u) / 260100u);
    }
}
// c(D2) for 0 <= D2: eight halvings over the thresholds (t in LDS on the device). Every D2 >= spread^2 gives 255.
__host__ __device__ __forceinline__ uint32_t distance_code(const uint32_t* t, uint32_t d2) {
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t step = 128u; step != 0u; step >>= 1) c += t[c + step] <= d2 ? step : 0u; // c + step <= 255
    return c;
}
// the result texel of a code: v = 255 - c (OUTSIDE) or c (INSIDE) on all four channels
__host__ __device__ __forceinline__ uint32_t distance_texel(uint32_t c, uint32_t mode) { return (mode == kDistanceInside ? c : 255u - c) * 0x01010101u; }

// inside: the stored code of the channel, as it is, against the threshold
__host__ __device__ __forceinline__ bool distance_inside(uint32_t texel, const DistanceConstants& f) { return ((texel >> f.shift) & 0xFFu) >= f.threshold; }
// What a mode measures the distance TO: OUTSIDE the texels inside the shape, INSIDE those that are not. `inside` is false for a position
// outside the source under TRANSPARENT.
__host__ __device__ __forceinline__ bool distance_target(bool inside, uint32_t mode) { return inside != (mode == kDistanceInside); }
// a column distance one row further from the last target: saturates at "none"
__host__ __device__ __forceinline__ uint32_t distance_step(uint32_t d, bool target) { return target ? 0u : d < kDistanceNone ? d + 1u : kDistanceNone; }
// what is stored of a column distance: itself below the spread, else "none" (it cannot change a byte)
__host__ __device__ __forceinline__ uint32_t distance_column(uint32_t d, uint32_t spread) { return d < spread ? d : kDistanceNone; }

// D2 of one texel from the column distances of its row, min(spread^2, min over dx of dx^2 + g(x + dx)^2): `g(i)` is the column distance i
// texels from the texel, any |i| < spread. A "none" is 255 and 255^2 >= spread^2, so it never wins and needs no test. The scan stops as
// soon as dx^2 reaches the best value found: no dx beyond can lower it.
template <typename G>
__host__ __device__ __forceinline__ uint32_t distance_scan(uint32_t spread, G&& g) {
    const uint32_t g0 = g(0);
    uint32_t best = g0 * g0 < spread * spread ? g0 * g0 : spread * spread;
    for (uint32_t dx = 1u; dx < spread && dx * dx < best; ++dx) {
        const uint32_t a = g(-(int)dx), b = g((int)dx), m = a < b ? a : b;
        const uint32_t d2 = dx * dx + m * m;
        best = d2 < best ? d2 : best;
    }
    return best;
}

// The size of the result: OUTSIDE under TRANSPARENT grows by the spread on every side, everything else keeps (w, h).
inline bool distance_grows(uint32_t mode, uint32_t edge) { return mode == kDistanceOutside && edge == kDistanceTransparent; }

// The rule on a whole image on the host (crh_distance_texels): per column two sweeps that count the rows since the last target, down and
// up, over the result's rows and spread - 1 rows beyond either end; then per texel the scan of its row. Linear in the spread per texel
// at worst. The caller's bytes at any alignment; `out` holds the result's size and is not `in`. A texel's word is assembled from its
// four bytes in memory order, r first. Every source address is formed from a tested or wrapped index.
inline void distance_run(const uint8_t* in, uint32_t w, uint32_t h, const DistanceConstants& f, uint8_t* out) {
    const bool grows = distance_grows(f.mode, f.edge);
    const int s = (int)f.spread, origin = grows ? s : 0;
    const int out_w = (int)w + 2 * origin, out_h = (int)h + 2 * origin;
    DistanceThresholds thresholds;
    distance_thresholds(f.spread, &thresholds);
    const auto target = [&](int i, int j) { // any position, in source coordinates
        bool inside = false;
        if (f.edge != kDistanceTransparent) i = edge_wrap(i, (int)w, f.edge), j = edge_wrap(j, (int)h, f.edge);
        if ((uint32_t)i < w && (uint32_t)j < h) {
            const uint8_t* t = in + ((size_t)j * w + (size_t)i) * 4u;
            inside = distance_inside(t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24, f);
        }
        return distance_target(inside, f.mode);
    };
    std::vector<uint8_t> g((size_t)out_w * out_h);
    for (int x = 0; x < out_w; ++x) {
        uint32_t d = kDistanceNone;
        for (int y = -(s - 1); y < out_h; ++y) { // the rows since the last target at or above
            d = distance_step(d, target(x - origin, y - origin));
            if (y >= 0) g[(size_t)y * out_w + x] = (uint8_t)d;
        }
        d = kDistanceNone;
        for (int y = out_h - 1 + (s - 1); y >= 0; --y) { // the rows to the next target at or below
            d = distance_step(d, target(x - origin, y - origin));
            if (y < out_h) {
                uint8_t& at = g[(size_t)y * out_w + x];
                at = (uint8_t)distance_column(d < at ? d : at, f.spread);
            }
        }
    }
    for (int y = 0; y < out_h; ++y) {
        const uint8_t* row = g.data() + (size_t)y * out_w;
        for (int x = 0; x < out_w; ++x) {
            const uint32_t d2 = distance_scan(f.spread, [&](int dx) -> uint32_t {
                const int i = x + dx; // a column of g: under a same-size edge through the wrap; under TRANSPARENT nothing (OUTSIDE) or off the shape (INSIDE) outside
                if (f.edge != kDistanceTransparent) return row[edge_wrap(i, out_w, f.edge)];
                return (uint32_t)i < (uint32_t)out_w ? row[i] : f.mode == kDistanceInside ? 0u : kDistanceNone;
            });
            const uint32_t r = distance_texel(distance_code(thresholds.t, d2), f.mode);
            uint8_t* d = out + ((size_t)y * out_w + x) * 4u;
            d[0] = (uint8_t)r, d[1] = (uint8_t)(r >> 8), d[2] = (uint8_t)(r >> 16), d[3] = (uint8_t)(r >> 24);
        }
    }
}

} // namespace crh
