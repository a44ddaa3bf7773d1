// csrc/turbulence.hpp — the noise rule of crh_image_turbulence (include/contrast_hip.h states it), written once: the seeded tables, the per-call
// constants from the caller's floats, one axis of one octave's lattice cell, the noise of every channel at a point and the texel of the sums.
// k_image_turbulence (image_filter.hip) and crh_turbulence_texels (image.hip, on the host) both call turbulence_axis, turbulence_corners,
// turbulence_noise, turbulence_add and turbulence_texel; the tables and the constants are made on the host alone.
// All real arithmetic is IEEE binary64 in the written order and parenthesisation, with only + - * / sqrt and a floor, compiled without
// contraction (-ffp-contract=off), and one rounding to a code at the end: the same bytes on x86-64 and on gfx950. Three things are written
// otherwise than the header words them, each with the same value in every case:
//   floor      |v| < 2^31 here, so floor goes through a 32-bit integer (two conversions, not crh_floor_d's four through 64 bits);
//   N / ratio  ratio is 2^o, so N * 2^-o is the same real number rounded once: the division is a multiplication;
//   i mod P    q = trunc(fl * (1 / P)) is within one of floor(i / P), so i - q P lies in [-P, 2 P) and two conditional steps finish it; the
//              neighbour (i + 1) mod P is the remainder plus one, or 0 when that reaches P.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/crh_fmath.h"

#ifndef CRH_TURBULENCE_PLAIN_MODULO
#define CRH_TURBULENCE_PLAIN_MODULO 0 // (a build with -DCRH_TURBULENCE_PLAIN_MODULO=1 takes the remainder with the % operator: DESIGN.md's comparison)
#endif

namespace crh {

constexpr uint32_t kTurbulenceFractalNoise = 0, kTurbulenceTurbulence = 1; // crh_turbulence_kind
constexpr uint32_t kTurbulenceMaxOctaves = 12;
constexpr uint32_t kTurbulenceGradientDoubles = 4 * 256 * 2;               // gradient[(k * 256 + i) * 2 + c]

// The seeded tables as crh_turbulence_tables hands them out, and as the kernel reads them: 16 bytes per (channel, lattice value).
struct TurbulenceTables {
    alignas(16) double gradient[kTurbulenceGradientDoubles];
    alignas(16) uint8_t lattice[256];
};

// The caller's floats as the rule uses them, and what is computed once per call.
struct TurbulenceConstants {
    double fx, fy;           // the frequencies, adjusted when stitched
    double ox, oy;           // offset
    double inv_px, inv_py;   // stitched: 1.0 / period of octave 0 (octave o: times 2^-o, exactly 1.0 / (P << o))
    int32_t px, py;          // the periods of octave 0; both 0 = not stitched, otherwise neither is
    uint32_t octaves;
};

// One axis of one octave's cell: the fractions, the s-curve and the two wrapped lattice coordinates.
struct TurbulenceAxis {
    double r0, r1, s;
    uint32_t b0, b1;
};

// The four channels' sums of one texel.
template <int CH>
struct TurbulenceSums {
    double v[CH];
};

inline int64_t turbulence_start(int32_t seed) {
    int64_t s = seed;
    if (s <= 0) s = (-s % 2147483646) + 1;
    if (s > 2147483646) s = 2147483646;
    return s;
}

inline int64_t turbulence_random(int64_t s) {
    int64_t r = 16807 * (s % 127773) - 2836 * (s / 127773);
    if (r <= 0) r += 2147483647;
    return r;
}

inline void turbulence_make_tables(int32_t seed, TurbulenceTables* out) {
    int64_t s = turbulence_start(seed);
    for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 256; ++i) {
            s = turbulence_random(s);
            const double gx = (double)((s % 512) - 256) / 256.0;
            s = turbulence_random(s);
            const double gy = (double)((s % 512) - 256) / 256.0;
            const double n = sqrt(gx * gx + gy * gy);
            double* g = out->gradient + (k * 256 + i) * 2;
            if (n == 0.0) g[0] = 0.0, g[1] = 0.0;
            else g[0] = gx / n, g[1] = gy / n;
        }
    for (int i = 0; i < 256; ++i) out->lattice[i] = (uint8_t)i;
    for (int i = 255; i >= 1; --i) {
        s = turbulence_random(s);
        const int j = (int)(s % 256);
        const uint8_t t = out->lattice[i];
        out->lattice[i] = out->lattice[j], out->lattice[j] = t;
    }
}

// floor for |x| < 2^31, and its integer
__host__ __device__ __forceinline__ double turbulence_floor(double x, int32_t* i) {
    int32_t t = (int32_t)x;
    double d = (double)t;
    if (d > x) d = d - 1.0, t = t - 1;
    *i = t;
    return d;
}

// One axis of the frequency rule: f and the period of octave 0 (0 = not wrapped) for n texels.
inline void turbulence_frequency(double f, uint32_t n_texels, bool stitch, double* f_out, int32_t* period) {
    *f_out = f, *period = 0;
    if (!stitch || f == 0.0) return;
    const double n = (double)n_texels;
    const double lo = crh_floor_d(n * f) / n, hi = -crh_floor_d(-(n * f)) / n;
    const double chosen = lo == 0.0 ? hi : (f / lo < hi / f ? lo : hi); // (f / 0 = +inf is not below anything)
    *f_out = chosen;
    *period = (int32_t)crh_floor_d(n * chosen + 0.5);
}

// The one place where the caller's floats become the rule's constants (validated: the caller's to do).
inline void turbulence_prepare(uint32_t width, uint32_t height, uint32_t octaves, bool stitch, const float base_frequency[2], const float offset[2], TurbulenceConstants* out) {
    TurbulenceConstants f = {};
    turbulence_frequency((double)base_frequency[0], width, stitch, &f.fx, &f.px);
    turbulence_frequency((double)base_frequency[1], height, stitch, &f.fy, &f.py);
    // An axis of frequency 0 beside a wrapped one takes the period 256, which wraps nothing — (i mod (256 << o)) & 255 = i & 255 —, so that a
    // stitched call has two periods and its code no test of them.
    if (f.px != 0 && f.py == 0) f.py = 256;
    if (f.py != 0 && f.px == 0) f.px = 256;
    f.ox = (double)offset[0], f.oy = (double)offset[1];
    f.inv_px = f.px ? 1.0 / (double)f.px : 0.0, f.inv_py = f.py ? 1.0 / (double)f.py : 0.0;
    f.octaves = octaves;
    *out = f;
}

// v at octave o of one axis -> its cell. STITCH: period = P << o, not 0, and inv_period = 1.0 / period.
template <bool STITCH>
__host__ __device__ __forceinline__ TurbulenceAxis turbulence_axis(double v, int32_t period, double inv_period) {
    TurbulenceAxis a;
    int32_t i;
    const double fl = turbulence_floor(v, &i);
    a.r0 = v - fl, a.r1 = a.r0 - 1.0;
    a.s = (a.r0 * a.r0) * (3.0 - (2.0 * a.r0));
    int32_t m0 = i, m1 = i + 1;
    if (STITCH) {
#if CRH_TURBULENCE_PLAIN_MODULO
        m0 = i % period;
#else
        m0 = i - (int32_t)(fl * inv_period) * period;
#endif
        if (m0 < 0) m0 += period;
        if (m0 >= period) m0 -= period;
        m1 = m0 + 1 == period ? 0 : m0 + 1;
    }
    a.b0 = (uint32_t)m0 & 255u, a.b1 = (uint32_t)m1 & 255u;
    return a;
}

// The lattice chain of a cell, shared by the channels: a0 = lat[bx0] and a1 = lat[bx1] (the column's), y the row's axis -> b00 b10 b01 b11.
__host__ __device__ __forceinline__ void turbulence_corners(const uint8_t* lat, uint32_t a0, uint32_t a1, const TurbulenceAxis& y, uint32_t b[4]) {
    b[0] = lat[(a0 + y.b0) & 255u], b[1] = lat[(a1 + y.b0) & 255u], b[2] = lat[(a0 + y.b1) & 255u], b[3] = lat[(a1 + y.b1) & 255u];
}

// noise(k, ...) of the cell with the corners b: `g` = channel k's 256 gradients, two doubles each.
__host__ __device__ __forceinline__ double turbulence_noise(const double* g, const uint32_t b[4], const TurbulenceAxis& x, const TurbulenceAxis& y) {
    const double q00x = g[b[0] * 2u], q00y = g[b[0] * 2u + 1u], q10x = g[b[1] * 2u], q10y = g[b[1] * 2u + 1u];
    const double q01x = g[b[2] * 2u], q01y = g[b[2] * 2u + 1u], q11x = g[b[3] * 2u], q11y = g[b[3] * 2u + 1u];
    double u = (x.r0 * q00x) + (y.r0 * q00y);
    double v = (x.r1 * q10x) + (y.r0 * q10y);
    const double a = u + (x.s * (v - u));
    u = (x.r0 * q01x) + (y.r1 * q01y);
    v = (x.r1 * q11x) + (y.r1 * q11y);
    const double c = u + (x.s * (v - u));
    return a + (y.s * (c - a));
}

// sum = sum + (N / ratio) for every channel of one octave; inv_ratio = 2^-o
template <uint32_t KIND, int CH>
__host__ __device__ __forceinline__ void turbulence_add(const uint8_t* lat, const double* gradient, uint32_t a0, uint32_t a1, const TurbulenceAxis& x, const TurbulenceAxis& y, double inv_ratio,
                                                        TurbulenceSums<CH>* sums) {
    uint32_t b[4];
    turbulence_corners(lat, a0, a1, y, b);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        double n = turbulence_noise(gradient + k * 512, b, x, y);
        if (KIND == kTurbulenceTurbulence) n = n < 0.0 ? -n : n;
        sums->v[k] = sums->v[k] + (n * inv_ratio);
    }
}

template <uint32_t KIND>
__host__ __device__ __forceinline__ uint32_t turbulence_code(double sum) {
    const double t = KIND == kTurbulenceFractalNoise ? (sum + 1.0) * 0.5 : sum;
    if (t >= 1.0) return 255u;
    int32_t code = 0;
    if (t > 0.0) (void)turbulence_floor(t * 255.0 + 0.5, &code);
    return (uint32_t)code;
}

// The sums of a texel -> r | g << 8 | b << 16 | a << 24, premultiplied. CH = 3 is the opaque texel.
template <uint32_t KIND, int CH>
__host__ __device__ __forceinline__ uint32_t turbulence_texel(const TurbulenceSums<CH>& sums) {
    const uint32_t alpha = CH == 3 ? 255u : turbulence_code<KIND>(sums.v[CH - 1]);
    uint32_t texel = alpha << 24;
#pragma unroll
    for (int k = 0; k < 3; ++k) texel |= ((turbulence_code<KIND>(sums.v[k]) * alpha + 127u) / 255u) << (8 * k);
    return texel;
}

// One texel on the host: the plain loop over the octaves.
template <uint32_t KIND, int CH, bool STITCH>
inline uint32_t turbulence_texel_at(const TurbulenceTables& t, const TurbulenceConstants& f, uint32_t i, uint32_t j) {
    double vx = (f.ox + (double)i) * f.fx, vy = (f.oy + (double)j) * f.fy;
    double inv_ratio = 1.0, inv_px = f.inv_px, inv_py = f.inv_py;
    TurbulenceSums<CH> sums = {};
    for (uint32_t o = 0; o < f.octaves; ++o) {
        const TurbulenceAxis x = turbulence_axis<STITCH>(vx, f.px << o, inv_px), y = turbulence_axis<STITCH>(vy, f.py << o, inv_py);
        turbulence_add<KIND, CH>(t.lattice, t.gradient, t.lattice[x.b0], t.lattice[x.b1], x, y, inv_ratio, &sums);
        vx = vx * 2.0, vy = vy * 2.0;
        inv_ratio = inv_ratio * 0.5, inv_px = inv_px * 0.5, inv_py = inv_py * 0.5;
    }
    return turbulence_texel<KIND, CH>(sums);
}

template <uint32_t KIND, int CH, bool STITCH>
inline void turbulence_run_as(const TurbulenceTables& t, const TurbulenceConstants& f, uint32_t w, uint32_t h, uint8_t* out) {
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            const uint32_t r = turbulence_texel_at<KIND, CH, STITCH>(t, f, i, j);
            uint8_t* d = out + ((size_t)j * w + i) * 4u;
            d[0] = (uint8_t)r, d[1] = (uint8_t)(r >> 8), d[2] = (uint8_t)(r >> 16), d[3] = (uint8_t)(r >> 24);
        }
}

// The rule on a whole image on the host (crh_turbulence_texels): `out` holds w x h texels at any alignment.
inline void turbulence_run(const TurbulenceTables& t, const TurbulenceConstants& f, uint32_t kind, bool opaque, uint32_t w, uint32_t h, uint8_t* out) {
    const bool stitch = f.px != 0 || f.py != 0;
#define CRH_TURBULENCE_RUN(KIND, CH)                                       \
    do {                                                                   \
        if (stitch) turbulence_run_as<KIND, CH, true>(t, f, w, h, out);    \
        else turbulence_run_as<KIND, CH, false>(t, f, w, h, out);          \
    } while (0)
    if (kind == kTurbulenceFractalNoise) {
        if (opaque) CRH_TURBULENCE_RUN(kTurbulenceFractalNoise, 3);
        else CRH_TURBULENCE_RUN(kTurbulenceFractalNoise, 4);
    } else {
        if (opaque) CRH_TURBULENCE_RUN(kTurbulenceTurbulence, 3);
        else CRH_TURBULENCE_RUN(kTurbulenceTurbulence, 4);
    }
#undef CRH_TURBULENCE_RUN
}

} // namespace crh
