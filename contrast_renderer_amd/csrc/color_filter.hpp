// csrc/color_filter.hpp — the colour-filter rule of crh_image_color_filter (include/contrast_hip.h states it), written once:
// k_image_color_filter (image_filter.hip) and crh_color_filter_texels (image.hip, on the host) both call color_filter_texel, and both take
// their coefficients from color_filter_quantize. All values are 8-bit codes, all arithmetic is signed 32-bit; nothing here divides by
// anything but the constant 255: the unpremultiply is one multiply by an entry of a 256-word table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "composite.hpp"

namespace crh {

constexpr float kColorMatrixMax = 16.0f; // CRH_COLOR_MATRIX_MAX

// The matrix as the host hands it to the kernel: k[i][j] = floor((double) m[i][j] * 65536 + 0.5) for the four input columns, |k| <= 2^20
// (a signed 24-bit operand), and bias[i] = 255 k[i][4] + 32768 (|bias| < 2^28): the constant column and the rounding half of row i.
struct ColorFilterCoefficients {
    int32_t k[4][4];
    int32_t bias[4];
};

enum ColorFilterRefusal { kColorFilterOk = 0, kColorFilterNonFinite, kColorFilterTooLarge };

// matrix: 20 floats, row-major 4 x 5, or nullptr for the identity. The one place where a float becomes a coefficient.
inline ColorFilterRefusal color_filter_quantize(const float* matrix, ColorFilterCoefficients* out) {
    static const float identity[20] = {1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0};
    const float* m = matrix ? matrix : identity;
    for (int n = 0; n < 20; ++n)
        if (!std::isfinite(m[n])) return kColorFilterNonFinite;
    for (int n = 0; n < 20; ++n)
        if (std::fabs(m[n]) > kColorMatrixMax) return kColorFilterTooLarge;
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 4; ++j) out->k[i][j] = (int32_t)std::floor((double)m[5 * i + j] * 65536.0 + 0.5);
        out->bias[i] = 255 * (int32_t)std::floor((double)m[5 * i + 4] * 65536.0 + 0.5) + 32768;
    }
    return kColorFilterOk;
}

// R[a] = floor(255 * 65536 / a) + 1, R[0] = 0: (c R[a] + 32768) >> 16 == (255 c + a / 2) / a for every c <= a <= 255 (all 32 896 pairs are
// checked by tests/test_color_filter_cpu.py through the library). c R[a] + 32768 <= 255 * 65536 + 255 + 32768 < 2^25.
struct UnpremultiplyTable {
    uint32_t r[256];
    constexpr UnpremultiplyTable() : r{} {
        for (uint32_t a = 1; a < 256u; ++a) r[a] = 16711680u / a + 1u;
    }
};

// a * b for |a| < 2^23, |b| < 2^23: the full-rate signed 24-bit multiply on the device (it fuses with the sum into v_mad_i32_i24)
__host__ __device__ __forceinline__ int32_t color_filter_mul(int32_t a, int32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

// The load and the unpremultiply of one colour code c beside its alpha a, `ra` = R[a]: c = min(c, a), then (255 c + a / 2) / a, <= 255
__host__ __device__ __forceinline__ uint32_t color_filter_unpremultiply(uint32_t code, uint32_t a, uint32_t ra) { return (composite_mul(code < a ? code : a, ra) + 32768u) >> 16; }

// One texel (r | g << 8 | b << 16 | a << 24, as the texels are) -> the filtered texel. `recip` = UnpremultiplyTable::r (in LDS on the
// device); `tables` = the 1024 bytes r[256] g[256] b[256] a[256] (in LDS on the device), read only when TABLES.
template <bool TABLES>
__host__ __device__ __forceinline__ uint32_t color_filter_texel(uint32_t texel, const ColorFilterCoefficients& f, const uint32_t* recip, const uint8_t* tables) {
    const uint32_t a = texel >> 24, ra = recip[a];
    int32_t u[4];
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) {
        const uint32_t code = (texel >> (8u * c)) & 0xFFu;
        u[c] = (int32_t)color_filter_unpremultiply(code, a, ra);
    }
    u[3] = (int32_t)a;
    uint32_t v[4];
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const int32_t n = color_filter_mul(f.k[i][0], u[0]) + color_filter_mul(f.k[i][1], u[1]) + color_filter_mul(f.k[i][2], u[2]) + color_filter_mul(f.k[i][3], u[3]) + f.bias[i];
        const int32_t s = n >> 16; // the floor: an arithmetic shift
        v[i] = (uint32_t)(s < 0 ? 0 : s > 255 ? 255 : s);
        if (TABLES) v[i] = tables[256u * i + v[i]];
    }
    return composite_fade(v[0], v[3]) | composite_fade(v[1], v[3]) << 8 | composite_fade(v[2], v[3]) << 16 | v[3] << 24; // premultiply: (v_c v_a + 127) / 255
}

// The rule on n texels on the host (crh_color_filter_texels): the caller's bytes at any alignment, out may be in; a texel's word is
// assembled from its four bytes in memory order, r first, whatever the host's byte order
template <bool TABLES>
inline void color_filter_run(const uint8_t* in, uint64_t n, const ColorFilterCoefficients& f, const uint8_t* tables, uint8_t* out) {
    static constexpr UnpremultiplyTable recip{};
    for (uint64_t k = 0; k < n; ++k) {
        const uint8_t* s = in + 4u * k;
        const uint32_t r = color_filter_texel<TABLES>(s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24, f, recip.r, tables);
        out[4u * k] = (uint8_t)r, out[4u * k + 1u] = (uint8_t)(r >> 8), out[4u * k + 2u] = (uint8_t)(r >> 16), out[4u * k + 3u] = (uint8_t)(r >> 24);
    }
}

} // namespace crh
