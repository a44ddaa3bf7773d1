// csrc/regions.hpp — the rules of crh_image_crop / crh_image_create_from_frame_region and of crh_image_statistics (include/contrast_hip.h
// states them), written once: which source texel a texel of a crop is, what a texel adds to the statistics of an image, and how two
// partial statistics join. k_image_crop, k_image_stats and k_image_stats_merge (image_filter.hip) and crh_crop_texels and
// crh_statistics_texels (image.hip, on the host, through crop_run and statistics_run) all call region_source, stats_code, stats_inside
// and StatsBounds. Everything is integer and nothing rounds: the same bytes and the same counts on x86-64 and on gfx950.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace crh {

// The crop's source index of one axis: result index i (< 16384) of a crop at `at` (any int32, passed as its 32 bits) is source index
// i + at, in range iff 0 <= i + at < n. Formed in wrapped unsigned arithmetic, as k_image_composite forms i - x: the true sum lies in
// [-2^31, 2^31 + 16384), so for n <= 65535 (a frame's largest side) the wrapped value is below n exactly when the true one is in range —
// a negative sum wraps to at least 2^31. No address is formed from `*s` unless this returns true.
__host__ __device__ __forceinline__ bool region_source(uint32_t i, uint32_t at, uint32_t n, uint32_t* s) {
    *s = i + at;
    return *s < n;
}

// The layout of a crh_image_stats in 32-bit words, which is also a workgroup's partial result on the device
constexpr uint32_t kStatsHistogramWords = 4 * 256;               // [channel][code]
constexpr uint32_t kStatsWords = kStatsHistogramWords + 5;       // + x0, y0, x1, y1, count
constexpr uint32_t kStatsX0 = kStatsHistogramWords, kStatsY0 = kStatsX0 + 1, kStatsX1 = kStatsX0 + 2, kStatsY1 = kStatsX0 + 3, kStatsCount = kStatsX0 + 4;

// What a call is after validation, for the host rule and the kernels alike (kernel arguments, by value)
struct StatsConstants {
    uint32_t shift;     // 8 * crh_channel: the stored code of the channel is (texel >> shift) & 255
    uint32_t threshold; // 1..255
};
// the stored code of channel c (0..3 = r, g, b, a) of a texel, the word its four bytes make on a little-endian machine
__host__ __device__ __forceinline__ uint32_t stats_code(uint32_t texel, uint32_t c) { return (texel >> (8u * c)) & 0xFFu; }
// inside: the stored code of the channel, as it is, against the threshold (distance.hpp's distance_inside, in the same words)
__host__ __device__ __forceinline__ bool stats_inside(uint32_t texel, const StatsConstants& f) { return ((texel >> f.shift) & 0xFFu) >= f.threshold; }

// The smallest half-open rectangle that holds a set of texels, and their number. Empty is (UINT32_MAX, UINT32_MAX, 0, 0), so that
// joining is min, min, max, max, + with no case for "nothing yet"; stats_finish turns an empty one into the header's 0, 0, 0, 0.
struct StatsBounds {
    uint32_t x0 = 0xFFFFFFFFu, y0 = 0xFFFFFFFFu, x1 = 0u, y1 = 0u, count = 0u;
};
__host__ __device__ __forceinline__ uint32_t stats_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ uint32_t stats_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
// one texel inside, at (i, j)
__host__ __device__ __forceinline__ void stats_add(StatsBounds& b, uint32_t i, uint32_t j) {
    b.x0 = stats_min(b.x0, i), b.y0 = stats_min(b.y0, j), b.x1 = stats_max(b.x1, i + 1u), b.y1 = stats_max(b.y1, j + 1u), b.count += 1u;
}
// two partial results: exact and independent of the order
__host__ __device__ __forceinline__ void stats_join(StatsBounds& b, const StatsBounds& o) {
    b.x0 = stats_min(b.x0, o.x0), b.y0 = stats_min(b.y0, o.y0), b.x1 = stats_max(b.x1, o.x1), b.y1 = stats_max(b.y1, o.y1), b.count += o.count;
}
// the five words behind the histogram, as the header states them
__host__ __device__ __forceinline__ void stats_finish(const StatsBounds& b, uint32_t* words) {
    const bool any = b.count != 0u;
    words[kStatsX0] = any ? b.x0 : 0u, words[kStatsY0] = any ? b.y0 : 0u, words[kStatsX1] = any ? b.x1 : 0u, words[kStatsY1] = any ? b.y1 : 0u, words[kStatsCount] = b.count;
}

// ---- the host rules: whole images in host memory, r g b a at any alignment, row 0 first

// crh_crop_texels: out (out_w x out_h) = the source (w x h) from (x, y) on, (0, 0, 0, 0) outside it
inline void crop_run(const uint8_t* in, uint32_t w, uint32_t h, int32_t x, int32_t y, uint32_t out_w, uint32_t out_h, uint8_t* out) {
    for (uint32_t j = 0; j < out_h; ++j) {
        uint32_t sj = 0u, si = 0u;
        const bool row = region_source(j, (uint32_t)y, h, &sj);
        for (uint32_t i = 0; i < out_w; ++i) {
            uint8_t* to = out + ((size_t)j * out_w + i) * 4;
            if (row && region_source(i, (uint32_t)x, w, &si)) memcpy(to, in + ((size_t)sj * w + si) * 4, 4);
            else memset(to, 0, 4);
        }
    }
}
// crh_statistics_texels: `words` = the kStatsWords words of a crh_image_stats
inline void statistics_run(const uint8_t* in, uint32_t w, uint32_t h, const StatsConstants& f, uint32_t* words) {
    memset(words, 0, kStatsWords * sizeof(uint32_t));
    StatsBounds bounds;
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            const uint8_t* p = in + ((size_t)j * w + i) * 4;
            const uint32_t texel = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
            for (uint32_t c = 0; c < 4u; ++c) words[256u * c + stats_code(texel, c)] += 1u;
            if (stats_inside(texel, f)) stats_add(bounds, i, j);
        }
    stats_finish(bounds, words);
}

} // namespace crh
