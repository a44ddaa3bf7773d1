// csrc/lighting.hpp — the lighting rule of crh_image_lighting (include/contrast_hip.h states it), written once: the per-call constants from
// the caller's floats, the Sobel gradient of the height field and the lit texel. k_image_lighting (image_filter.hip) and
// crh_lighting_texels (image.hip, on the host) both call lighting_prepare, lighting_gradient and lighting_texel; the wrap is edge.hpp's.
// All real arithmetic is IEEE binary64 in the written order and parenthesisation, with only + - * / sqrt and the functions of
// include/crh_fmath.h, compiled without contraction (-ffp-contract=off), and one rounding to a code at the end: the same bytes on x86-64 and
// on gfx950.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "../../include/crh_fmath.h"
#include "edge.hpp"

namespace crh {

constexpr uint32_t kLightingDiffuse = 0, kLightingSpecular = 1;           // crh_lighting_op
constexpr uint32_t kLightDistant = 0, kLightPoint = 1, kLightSpot = 2;    // crh_light_kind
constexpr uint32_t kLightingTransparent = 0;                              // CRH_BLUR_EDGE_TRANSPARENT; 1, 2, 3 = PAD, REPEAT, REFLECT

// The caller's floats as the rule uses them: every field widened to double, and what is computed once per call.
struct LightingConstants {
    double s;              // surface_scale
    double k;              // constant: kd or ks
    double specular;       // specular_exponent
    double color[3];
    double l[3];           // DISTANT: L = (ca ce, sa ce, se)
    double position[3];    // POINT, SPOT
    double axis[3];        // SPOT: S = (points_at - position) / its length
    double spot_exponent;  // SPOT
    double cone_cos;       // SPOT with a cone: cc = cos(rad(cone_angle))
    uint32_t cone;         // SPOT: 1 = a cone is set
    uint32_t flat;         // DISTANT: the texel of a zero gradient (lighting_texel at gx = gy = 0), which k_image_lighting writes without the arithmetic
};

__host__ __device__ __forceinline__ double lighting_rad(double degrees) { return degrees * (CRH_PI / 180.0); }

// code(t) = t >= 1 ? 255 : floor(t * 255 + 1/2); t is finite and not negative (or -0), so the product is below 255.5
__host__ __device__ __forceinline__ uint32_t lighting_code(double t) { return t >= 1.0 ? 255u : (uint32_t)(int64_t)crh_floor_d(t * 255.0 + 0.5); }

__host__ __device__ __forceinline__ double lighting_max0(double x) { return x > 0.0 ? x : 0.0; }

// The Sobel gradient of the 3 x 3 alpha codes a[row][column] around a texel: gx = the right column minus the left, gy = the bottom row minus
// the top, each weighted 1 2 1; both in [-1020, 1020].
__host__ __device__ __forceinline__ void lighting_gradient(const uint32_t a[3][3], int* gx, int* gy) {
    *gx = (int)(a[0][2] + 2u * a[1][2] + a[2][2]) - (int)(a[0][0] + 2u * a[1][0] + a[2][0]);
    *gy = (int)(a[2][0] + 2u * a[2][1] + a[2][2]) - (int)(a[0][0] + 2u * a[0][1] + a[0][2]);
}

// One texel: the gradient (gx, gy) at column i, row j, `alpha` = A(i, j) -> r | g << 8 | b << 16 | a << 24.
template <uint32_t OP, uint32_t LIGHT>
__host__ __device__ __forceinline__ uint32_t lighting_texel(const LightingConstants& f, int gx, int gy, uint32_t alpha, uint32_t i, uint32_t j) {
    const double nx = (f.s * (double)(-gx)) / 1020.0, ny = (f.s * (double)(-gy)) / 1020.0; // nz = 1
    const double nlen = sqrt((nx * nx + ny * ny) + 1.0);
    double lx, ly, lz;
    if (LIGHT == kLightDistant) {
        lx = f.l[0], ly = f.l[1], lz = f.l[2];
    } else {
        const double dx = f.position[0] - ((double)i + 0.5), dy = f.position[1] - ((double)j + 0.5), dz = f.position[2] - (f.s * (double)alpha) / 255.0;
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        if (len == 0.0) lx = ly = lz = 0.0;
        else lx = dx / len, ly = dy / len, lz = dz / len;
    }
    double c[3] = {f.color[0], f.color[1], f.color[2]};
    if (LIGHT == kLightSpot) {
        const double m = -((lx * f.axis[0] + ly * f.axis[1]) + lz * f.axis[2]);
        if (m <= 0.0 || (f.cone != 0u && m < f.cone_cos)) {
            c[0] = c[1] = c[2] = 0.0;
        } else {
            const double p = crh_d_pow(m, f.spot_exponent);
            c[0] = f.color[0] * p, c[1] = f.color[1] * p, c[2] = f.color[2] * p;
        }
    }
    if (OP == kLightingDiffuse) {
        const double v = f.k * lighting_max0(((nx * lx + ny * ly) + lz) / nlen);
        return lighting_code(v * c[0]) | lighting_code(v * c[1]) << 8 | lighting_code(v * c[2]) << 16 | 255u << 24;
    }
    const double hz = lz + 1.0;
    const double hlen = sqrt((lx * lx + ly * ly) + hz * hz);
    double v = 0.0;
    if (hlen != 0.0) v = f.k * crh_d_pow(lighting_max0(((nx * lx + ny * ly) + hz) / (nlen * hlen)), f.specular);
    const uint32_t r = lighting_code(v * c[0]), g = lighting_code(v * c[1]), b = lighting_code(v * c[2]);
    const uint32_t a = r > g ? (r > b ? r : b) : (g > b ? g : b);
    return r | g << 8 | b << 16 | a << 24;
}

// lighting_texel with op and light at run time (the host's loop and the per-call flat texel)
__host__ __forceinline__ uint32_t lighting_texel_of(uint32_t op, uint32_t light, const LightingConstants& f, int gx, int gy, uint32_t alpha, uint32_t i, uint32_t j) {
    if (op == kLightingDiffuse) {
        if (light == kLightDistant) return lighting_texel<kLightingDiffuse, kLightDistant>(f, gx, gy, alpha, i, j);
        if (light == kLightPoint) return lighting_texel<kLightingDiffuse, kLightPoint>(f, gx, gy, alpha, i, j);
        return lighting_texel<kLightingDiffuse, kLightSpot>(f, gx, gy, alpha, i, j);
    }
    if (light == kLightDistant) return lighting_texel<kLightingSpecular, kLightDistant>(f, gx, gy, alpha, i, j);
    if (light == kLightPoint) return lighting_texel<kLightingSpecular, kLightPoint>(f, gx, gy, alpha, i, j);
    return lighting_texel<kLightingSpecular, kLightSpot>(f, gx, gy, alpha, i, j);
}

// The one place where the caller's floats become the rule's constants. The fields are validated (the caller's to do): only those that
// `op` and `light` use are read, the others are left 0. points_at differs from position, so the axis's length is not 0.
inline void lighting_prepare(uint32_t op, uint32_t light, float surface_scale, float constant, float specular_exponent, const float color[3], float azimuth, float elevation,
                             const float position[3], const float points_at[3], float spot_exponent, float cone_angle, LightingConstants* out) {
    LightingConstants f = {};
    f.s = (double)surface_scale, f.k = (double)constant;
    f.specular = op == kLightingSpecular ? (double)specular_exponent : 0.0;
    for (int c = 0; c < 3; ++c) f.color[c] = (double)color[c];
    if (light == kLightDistant) {
        double sa, ca, se, ce;
        crh_d_sincos(lighting_rad((double)azimuth), &sa, &ca);
        crh_d_sincos(lighting_rad((double)elevation), &se, &ce);
        f.l[0] = ca * ce, f.l[1] = sa * ce, f.l[2] = se;
    } else {
        for (int c = 0; c < 3; ++c) f.position[c] = (double)position[c];
    }
    if (light == kLightSpot) {
        const double dx = (double)points_at[0] - f.position[0], dy = (double)points_at[1] - f.position[1], dz = (double)points_at[2] - f.position[2];
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        f.axis[0] = dx / len, f.axis[1] = dy / len, f.axis[2] = dz / len;
        f.spot_exponent = (double)spot_exponent;
        f.cone = cone_angle != 0.0f ? 1u : 0u;
        if (f.cone) {
            double sc;
            crh_d_sincos(lighting_rad((double)cone_angle), &sc, &f.cone_cos);
        }
    }
    if (light == kLightDistant) f.flat = lighting_texel_of(op, light, f, 0, 0, 0u, 0u, 0u);
    *out = f;
}

// The rule on a whole image on the host (crh_lighting_texels): the plain loop over every texel and its 3 x 3 alpha codes. The caller's bytes
// at any alignment; `out` holds w x h texels and is not `in`. Only the alpha byte of a source texel is read.
inline void lighting_run(const uint8_t* in, uint32_t w, uint32_t h, const LightingConstants& f, uint32_t op, uint32_t light, uint32_t edge, uint8_t* out) {
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            uint32_t a[3][3];
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int x = (int)i + dx, y = (int)j + dy;
                    if (edge == kLightingTransparent) a[dy + 1][dx + 1] = (uint32_t)x < w && (uint32_t)y < h ? in[((size_t)y * w + (size_t)x) * 4u + 3u] : 0u;
                    else a[dy + 1][dx + 1] = in[((size_t)edge_wrap(y, (int)h, edge) * w + (size_t)edge_wrap(x, (int)w, edge)) * 4u + 3u];
                }
            int gx, gy;
            lighting_gradient(a, &gx, &gy);
            const uint32_t r = lighting_texel_of(op, light, f, gx, gy, a[1][1], i, j);
            uint8_t* d = out + ((size_t)j * w + i) * 4u;
            d[0] = (uint8_t)r, d[1] = (uint8_t)(r >> 8), d[2] = (uint8_t)(r >> 16), d[3] = (uint8_t)(r >> 24);
        }
}

} // namespace crh
