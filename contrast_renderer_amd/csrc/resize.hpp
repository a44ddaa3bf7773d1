// csrc/resize.hpp — the resampling rule of crh_image_resize (include/contrast_hip.h states it), written once: the five filters, the taps of
// one axis (window, weights, rounding to 1/16384, the deficit to the taps nearest the centre), the two integer sums with their clamps, and
// the table the kernels read. crh_resize_taps, crh_resize_texels (image.hip, on the host, through resize_run) and crh_image_resize's
// upload all come from resize_axis; k_image_resize_h and k_image_resize_v (image_filter.hip) and resize_run share resize_intermediate,
// resize_code and resize_texel. The real arithmetic is IEEE binary64 in the written order with only + - * / floor and crh_d_sincos of
// include/crh_fmath.h, compiled without contraction (-ffp-contract=off), and runs on the host only; everything per texel is integer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "../../include/crh_fmath.h"

namespace crh {

constexpr uint32_t kResizeBox = 0, kResizeTriangle = 1, kResizeCatmullRom = 2, kResizeMitchell = 3, kResizeLanczos3 = 4; // crh_resize_filter
constexpr uint32_t kResizeFilters = 5;
constexpr uint32_t kResizeMaxTaps = 512;  // CRH_MAX_RESIZE_TAPS
constexpr int32_t kResizeOne = 16384;     // the taps of an output sum to this
constexpr int32_t kResizeMaxGain = 32768; // the bound on the sum of |q| of an output: keeps the vertical sum inside 32 bits

// the support r of a filter
inline double resize_support(uint32_t filter) { return filter == kResizeBox ? 0.5 : filter == kResizeTriangle ? 1.0 : filter == kResizeLanczos3 ? 3.0 : 2.0; }
// f(x) of a filter, in the header's Horner order; 0 outside the support
inline double resize_weight(uint32_t filter, double x) {
    const double a = x < 0.0 ? -x : x;
    switch (filter) {
    case kResizeBox: return x >= -0.5 && x < 0.5 ? 1.0 : 0.0;
    case kResizeTriangle: return a < 1.0 ? 1.0 - a : 0.0;
    case kResizeCatmullRom:
        if (a < 1.0) return ((1.5 * a - 2.5) * a) * a + 1.0;
        if (a < 2.0) return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0;
        return 0.0;
    case kResizeMitchell:
        if (a < 1.0) return (((21.0 * a - 36.0) * a) * a + 16.0) / 18.0;
        if (a < 2.0) return (((-7.0 * a + 36.0) * a - 60.0) * a + 32.0) / 18.0;
        return 0.0;
    default: { // kResizeLanczos3
        if (a >= 3.0) return 0.0;
        if (a == 0.0) return 1.0;
        const double p = CRH_PI * a;
        double s1, s3, unused;
        crh_d_sincos(p, &s1, &unused);
        crh_d_sincos(p / 3.0, &s3, &unused);
        return ((3.0 * s1) * s3) / (p * p);
    }
    }
}

// The taps of one axis, n source texels to m: per output its window [first, first + count) and its count taps, back to back.
struct ResizeAxis {
    std::vector<int32_t> first;
    std::vector<uint16_t> count;
    std::vector<int16_t> taps;
    std::vector<uint32_t> offset; // of an output's taps in `taps`
};
enum ResizeAxisStatus { kResizeAxisOk = 0, kResizeAxisTaps = 1, kResizeAxisGain = 2 };
// 1 <= n, m <= 16384, filter < 5. kResizeAxisTaps: an output's window holds more than kResizeMaxTaps texels; kResizeAxisGain: an output's
// taps break sum |q| <= 32768 or the deficit exceeds its count (neither was ever seen). With `into` null only the windows are counted
// (*total, the number of taps), which finds kResizeAxisTaps alone.
inline ResizeAxisStatus resize_axis(uint32_t n, uint32_t m, uint32_t filter, ResizeAxis* into, uint64_t* total) {
    const double r = resize_support(filter);
    const double ratio = (double)n / (double)m, s = ratio > 1.0 ? ratio : 1.0;
    uint64_t sum = 0;
    if (into) into->first.resize(m), into->count.resize(m), into->offset.resize(m), into->taps.clear();
    std::vector<double> w;
    std::vector<int32_t> q;
    std::vector<uint32_t> order;
    for (uint32_t o = 0; o < m; ++o) {
        const double c = (((double)o + 0.5) * (double)n) / (double)m;
        const double reach = r * s;
        int32_t lo = (int32_t)std::floor(c - reach), hi = (int32_t)std::floor(c + reach);
        if (lo < 0) lo = 0;
        if (hi > (int32_t)n - 1) hi = (int32_t)n - 1;
        const int32_t count = hi - lo + 1; // >= 1: lo <= floor(c) <= n - 1 and hi >= floor(c) >= 0
        if (count > (int32_t)kResizeMaxTaps) return kResizeAxisTaps;
        sum += (uint64_t)count;
        if (!into) continue;
        w.resize((size_t)count), q.resize((size_t)count), order.resize((size_t)count);
        double S = 0.0;
        for (int32_t t = 0; t < count; ++t) {
            w[t] = resize_weight(filter, (((double)(lo + t) + 0.5) - c) / s);
            S += w[t];
        }
        if (!(S > 0.0)) return kResizeAxisGain;
        int32_t Q = 0;
        for (int32_t t = 0; t < count; ++t) {
            q[t] = (int32_t)std::floor(w[t] / S * 16384.0 + 0.5);
            Q += q[t];
        }
        const int32_t d = kResizeOne - Q, g = d < 0 ? -1 : 1, units = d < 0 ? -d : d;
        if (units > count) return kResizeAxisGain;
        if (units != 0) { // the |d| taps nearest the centre, ties to the lower t (a stable sort of the distances)
            std::iota(order.begin(), order.end(), 0u);
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
                const double da = std::fabs(((double)(lo + (int32_t)a) + 0.5) - c), db = std::fabs(((double)(lo + (int32_t)b) + 0.5) - c);
                return da < db;
            });
            for (int32_t k = 0; k < units; ++k) q[order[(size_t)k]] += g;
        }
        int32_t gain = 0;
        for (int32_t t = 0; t < count; ++t) gain += q[t] < 0 ? -q[t] : q[t];
        if (gain > kResizeMaxGain) return kResizeAxisGain;
        into->first[o] = lo, into->count[o] = (uint16_t)count, into->offset[o] = (uint32_t)into->taps.size();
        for (int32_t t = 0; t < count; ++t) into->taps.push_back((int16_t)q[t]); // |q| <= (32768 + 16384) / 2: 16 bits hold it
    }
    if (total) *total = sum;
    return kResizeAxisOk;
}

// The sums' roundings and clamps. Horizontal: the codes' sum (|.| <= 255 * 32768) to units of 1/256 code in 16 bits; vertical: the
// intermediate's sum (|.| + 2^21 < 2^31 by the gain bound) to a code. The shifts are arithmetic (floor).
__host__ __device__ __forceinline__ uint32_t resize_intermediate(int32_t sum) {
    const int32_t t = (sum + 32) >> 6;
    return (uint32_t)(t < 0 ? 0 : t > 65280 ? 65280 : t);
}
__host__ __device__ __forceinline__ uint32_t resize_code(int32_t sum) {
    const int32_t v = (sum + (1 << 21)) >> 22;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}
// the result texel of four codes: alpha as it is, each colour min(v, alpha)
__host__ __device__ __forceinline__ uint32_t resize_texel(uint32_t r, uint32_t g, uint32_t b, uint32_t a) {
    return (r < a ? r : a) | (g < a ? g : a) << 8 | (b < a ? b : a) << 16 | a << 24;
}

// What the kernels read of an axis (words; both axes go up in one upload). A window is widened to start on an even source index and to
// hold an even number of taps, with zero taps: the kernels take taps two to a word and pairs never straddle the even boundaries of the
// horizontal kernel's chunks. [0, m): the even first index; [m, 2 m): the even count; then m * pairs words, output o's at 2 m + o * pairs:
// tap 2 p | tap 2 p + 1 << 16 as signed 16-bit fields, zero beyond the count. A widened window may name index n (one past the source) under
// a zero tap, on an odd n only: the kernels stage a zero there or clamp the index. Every other index lies inside the source, which
// this asserts.
struct ResizeTable {
    uint32_t pairs; // words of taps per output
    std::vector<uint32_t> words;
};
inline bool resize_table(const ResizeAxis& axis, uint32_t n, ResizeTable* into) {
    const uint32_t m = (uint32_t)axis.first.size();
    uint32_t pairs = 1u;
    for (uint32_t o = 0; o < m; ++o) pairs = std::max(pairs, (((uint32_t)axis.first[o] & 1u) + axis.count[o] + 1u) / 2u);
    into->pairs = pairs;
    into->words.assign((size_t)m * (2u + pairs), 0u);
    for (uint32_t o = 0; o < m; ++o) {
        const uint32_t lead = (uint32_t)axis.first[o] & 1u, first = (uint32_t)axis.first[o] - lead, count = (lead + axis.count[o] + 1u) & ~1u;
        if (axis.first[o] < 0 || (uint32_t)axis.first[o] + axis.count[o] > n || first + count > n + 1u) return false;
        into->words[o] = first, into->words[(size_t)m + o] = count;
        uint32_t* q = into->words.data() + (size_t)2u * m + (size_t)o * pairs;
        for (uint32_t t = 0; t < axis.count[o]; ++t) q[(lead + t) / 2u] |= (uint32_t)(uint16_t)axis.taps[axis.offset[o] + t] << ((lead + t) % 2u ? 16 : 0);
    }
    return true;
}

// The rule on a whole image on the host (crh_resize_texels): the horizontal pass into four 16-bit values per texel at the result's width
// and the source's height, then the vertical pass. The caller's bytes at any alignment; `out` is not `in`. Every source index is
// first + t < first + count <= n.
inline void resize_run(const uint8_t* in, uint32_t w, uint32_t h, const ResizeAxis& ax, const ResizeAxis& ay, uint32_t out_w, uint32_t out_h, uint8_t* out) {
    std::vector<uint16_t> tmp((size_t)out_w * h * 4u);
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t o = 0; o < out_w; ++o) {
            const int16_t* q = ax.taps.data() + ax.offset[o];
            const uint8_t* texel = in + ((size_t)j * w + (size_t)ax.first[o]) * 4u;
            int32_t sum[4] = {0, 0, 0, 0};
            for (uint32_t t = 0; t < ax.count[o]; ++t, texel += 4)
                for (int c = 0; c < 4; ++c) sum[c] += (int32_t)q[t] * (int32_t)texel[c];
            for (int c = 0; c < 4; ++c) tmp[((size_t)j * out_w + o) * 4u + c] = (uint16_t)resize_intermediate(sum[c]);
        }
    for (uint32_t i = 0; i < out_h; ++i) {
        const int16_t* q = ay.taps.data() + ay.offset[i];
        for (uint32_t o = 0; o < out_w; ++o) {
            int32_t sum[4] = {0, 0, 0, 0};
            for (uint32_t t = 0; t < ay.count[i]; ++t) {
                const uint16_t* v = tmp.data() + ((size_t)((uint32_t)ay.first[i] + t) * out_w + o) * 4u;
                for (int c = 0; c < 4; ++c) sum[c] += (int32_t)q[t] * (int32_t)v[c];
            }
            const uint32_t texel = resize_texel(resize_code(sum[0]), resize_code(sum[1]), resize_code(sum[2]), resize_code(sum[3]));
            uint8_t* d = out + ((size_t)i * out_w + o) * 4u;
            d[0] = (uint8_t)texel, d[1] = (uint8_t)(texel >> 8), d[2] = (uint8_t)(texel >> 16), d[3] = (uint8_t)(texel >> 24);
        }
    }
}

} // namespace crh
