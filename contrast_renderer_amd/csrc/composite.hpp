// csrc/composite.hpp — the compositing rule of crh_image_composite (include/contrast_hip.h states it), written once: k_image_composite
// (image_filter.hip) and crh_composite_texels (image.hip, on the host) both call composite_texel. All values are 8-bit codes, all arithmetic is
// unsigned 32-bit; nothing here divides by anything but the constants 255 and 65025.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crh {

constexpr uint32_t kCompositeOps = 13;  // CRH_COMPOSITE_CLEAR .. CRH_COMPOSITE_PLUS
constexpr uint32_t kBlendModes = 9;     // CRH_BLEND_NORMAL .. CRH_BLEND_EXCLUSION
enum : uint32_t { kBlendNormal = 0, kBlendMultiply, kBlendScreen, kBlendOverlay, kBlendDarken, kBlendLighten, kBlendHardLight, kBlendDifference, kBlendExclusion };

// The operator as the host hands it to the kernel: fa = a0 + a1 * ba, fb = b0 + b1 * sa, with a0, b0 in {0, 255} and a1, b1 in {-1, 0, 1}
struct CompositeFactors {
    int32_t a0, a1, b0, b1;
};
// crh_composite_op -> its row of the header's table
inline CompositeFactors composite_factors(uint32_t op) {
    static const CompositeFactors table[kCompositeOps] = {
        {0, 0, 0, 0},      // CLEAR
        {255, 0, 0, 0},    // COPY
        {0, 0, 255, 0},    // DST
        {255, 0, 255, -1}, // SRC_OVER
        {255, -1, 255, 0}, // DST_OVER
        {0, 1, 0, 0},      // SRC_IN
        {0, 0, 0, 1},      // DST_IN
        {255, -1, 0, 0},   // SRC_OUT
        {0, 0, 255, -1},   // DST_OUT
        {0, 1, 255, -1},   // SRC_ATOP
        {255, -1, 0, 1},   // DST_ATOP
        {255, -1, 255, -1}, // XOR
        {255, 0, 255, 0},  // PLUS
    };
    return table[op];
}

// a * b for a, b < 2^24 with a product below 2^32: the full-rate 24-bit multiply on the device (v_mul_u32_u24), the plain one on the host
__host__ __device__ __forceinline__ uint32_t composite_mul(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}
// (s * o + 127) / 255 for codes s, o: the numerator is < 2^16, where n / 255 == (n * 32897) >> 23 (and n * 32897 < 2^32)
__host__ __device__ __forceinline__ uint32_t composite_fade(uint32_t s, uint32_t o) { return composite_mul(composite_mul(s, o) + 127u, 32897u) >> 23; }

// The blend term T of one colour channel, in units of 1 / 255^2; 0 <= T <= sa * ba because sc <= sa and bc <= ba
template <uint32_t MODE>
__host__ __device__ __forceinline__ uint32_t composite_term(uint32_t sc, uint32_t sa, uint32_t bc, uint32_t ba) {
    const uint32_t sb = composite_mul(sc, ba), bs = composite_mul(bc, sa), cc = composite_mul(sc, bc);
    if (MODE == kBlendNormal) return sb;
    if (MODE == kBlendMultiply) return cc;
    if (MODE == kBlendScreen) return sb + bs - cc;
    if (MODE == kBlendDarken) return sb < bs ? sb : bs;
    if (MODE == kBlendLighten) return sb > bs ? sb : bs;
    if (MODE == kBlendDifference) return sb > bs ? sb - bs : bs - sb;
    if (MODE == kBlendExclusion) return sb + bs - 2u * cc;
    // HARD_LIGHT chooses by the source, OVERLAY by the backdrop; the two branches are the same
    const bool dark = MODE == kBlendHardLight ? 2u * sc <= sa : 2u * bc <= ba;
    return dark ? 2u * cc : composite_mul(sa, ba) - 2u * composite_mul(ba - bc, sa - sc);
}

// One texel pair -> the packed result (r | g << 8 | b << 16 | a << 24, as the texels are). `o` = the opacity's code.
template <uint32_t MODE>
__host__ __device__ __forceinline__ uint32_t composite_texel(uint32_t source, uint32_t backdrop, uint32_t o, CompositeFactors f) {
    const uint32_t ba = backdrop >> 24, sa0 = source >> 24;
    const uint32_t sa = composite_fade(sa0, o);
    const uint32_t fa = (uint32_t)(f.a0 + f.a1 * (int32_t)ba), fb = (uint32_t)(f.b0 + f.b1 * (int32_t)sa); // in [0, 255]
    const uint32_t ao = (composite_mul(fa, sa) + composite_mul(fb, ba) + 127u) / 255u;
    uint32_t out = (ao < 255u ? ao : 255u) << 24;
#pragma unroll
    for (uint32_t shift = 0; shift < 24u; shift += 8u) {
        uint32_t sc = (source >> shift) & 0xFFu, bc = (backdrop >> shift) & 0xFFu;
        sc = composite_fade(sc < sa0 ? sc : sa0, o), bc = bc < ba ? bc : ba; // load: c = min(c, a); then the opacity (monotone: sc <= sa stays)
        const uint32_t x = composite_mul(sc, 255u - ba) + composite_term<MODE>(sc, sa, bc, ba); // <= 65025
        const uint32_t co = (composite_mul(fa, x) + 255u * composite_mul(fb, bc) + 32512u) / 65025u; // the numerator is <= 33 162 750
        out |= (co < 255u ? co : 255u) << shift;
    }
    return out;
}

// The rule on n texel pairs on the host (crh_composite_texels): the caller's bytes at any alignment; a texel's word is assembled from its
// four bytes in memory order, r first, whatever the host's byte order
template <uint32_t MODE>
inline void composite_run(const uint8_t* source, const uint8_t* backdrop, uint64_t n, uint32_t o, CompositeFactors f, uint8_t* out) {
    for (uint64_t k = 0; k < n; ++k) {
        const uint8_t *s = source + 4u * k, *b = backdrop + 4u * k;
        const uint32_t r = composite_texel<MODE>(s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24,
                                                 b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24, o, f);
        out[4u * k] = (uint8_t)r, out[4u * k + 1u] = (uint8_t)(r >> 8), out[4u * k + 2u] = (uint8_t)(r >> 16), out[4u * k + 3u] = (uint8_t)(r >> 24);
    }
}

// CALL(mode constant) for a run-time mode below kBlendModes: the one branch on the mode, taken outside the texel and channel loops
#define CRH_COMPOSITE_MODES(mode, CALL) \
    switch (mode) {                     \
    case 0u: CALL(0u); break;           \
    case 1u: CALL(1u); break;           \
    case 2u: CALL(2u); break;           \
    case 3u: CALL(3u); break;           \
    case 4u: CALL(4u); break;           \
    case 5u: CALL(5u); break;           \
    case 6u: CALL(6u); break;           \
    case 7u: CALL(7u); break;           \
    default: CALL(8u); break;           \
    }

} // namespace crh
