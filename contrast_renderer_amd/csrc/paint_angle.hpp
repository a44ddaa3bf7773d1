// csrc/paint_angle.hpp — the angle of a conic gradient paint (include/contrast_hip.h, crh_scene_set_paints: CRH_PAINT_CONIC), once for host and
// device: f32 only, no libm call, every fused operation an explicit fmaf, so that with -ffp-contract=off both give the same bits. The paint block
// of the general triangle kernel (raster_tile_body.inc) evaluates it once per sample; crh_selftest_fmath (fn 10) returns it from the device and
// the tests compile this header alone with the host compiler. crh_atan2f of include/crh_fmath.h is a binary64 series for "once per join".
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRH_PAINT_ANGLE_FN __host__ __device__ inline
#else
#define CRH_PAINT_ANGLE_FN inline
#endif

namespace crh {

// |paint_turns(y, x) - atan2(y, x) / 2 pi| (taken round the circle: 1 and 0 are one angle) for finite x, y, in turns. Measured on the host
// against binary64 atan2 (tests/cpp/paint_angle_harness.cpp --measure N; DESIGN.md §7 "Conic"): all eight octants, magnitudes from the
// smallest denormal to 2^24 under random mantissas, min / max ratios dense in [0, 1] (N evenly spaced and as many random ones per magnitude)
// and down to 2^-173. The figure is that of a sample and depends on it: seven runs with N from 500 to 200 000 (1.7e9 points together) gave
// between 6.11e-8 and 6.38e-8, so the largest error seen is 6.38e-8 and a larger one may exist. The polynomial's own residue is 6e-9 and
// varies far more slowly than the sampling steps, so what a sampling can miss is a coincidence of roundings. The constant is therefore not
// the measurement plus a guess but the sum of the half ulps, as if all fell one way: the roundings of q, q^2, the seven Horner steps and the
// product move r by at most 2.2e-8 together, and the three folds add half an ulp of 0.25, 0.5 and 1 (0.7e-8 + 1.5e-8 + 3.0e-8): 8.0e-8
// with the residue, 1.6e-8 above the largest error seen.
constexpr float kPaintTurnsError = 8.0e-8f;

// The angle of (x, y) from +x towards +y in turns, in [0, 1): paint_turns(0, 0) = 0, and the four axes give exactly 0, 0.25, 0.5 and 0.75
// (a zero of either sign counts as +0). r = q P(q^2) ~ atan(q) / 2 pi for q = min(|x|, |y|) / max(|x|, |y|) in [0, 1] — P has eight
// coefficients, a weighted minimax fit in binary64 rounded to f32 — then the three octant steps, then 1 (y = -tiny) folded back to 0.
CRH_PAINT_ANGLE_FN float paint_turns(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float hi = fmaxf(ax, ay), lo = fminf(ax, ay);
    const float q = hi == 0.0f ? 0.0f : lo / hi;
    const float s = q * q;
    float p = -6.453040987e-04f;
    p = fmaf(p, s, 3.479597392e-03f);
    p = fmaf(p, s, -8.898723871e-03f);
    p = fmaf(p, s, 1.534603629e-02f);
    p = fmaf(p, s, -2.213627286e-02f);
    p = fmaf(p, s, 3.174594417e-02f);
    p = fmaf(p, s, -5.304612219e-02f);
    p = fmaf(p, s, 1.591548324e-01f);
    float r = p * q;
    if (ay > ax) r = 0.25f - r;
    if (x < 0.0f) r = 0.5f - r;
    if (y < 0.0f) r = 1.0f - r;
    return r == 1.0f ? 0.0f : r;
}

} // namespace crh
