// csrc/convolve.hpp — the convolution rule of crh_image_convolve (include/contrast_hip.h states it), written once: the quantisation of the
// kernel matrix, the load of one texel (the clamp to alpha and, under preserve_alpha, the unpremultiply of color_filter.hpp) and the output
// stage. k_image_convolve (image_filter.hip) and crh_convolve_texels (image.hip, on the host) both call convolve_load, convolve_mad and
// convolve_store, and both take their coefficients from convolve_quantize; the wrap is edge.hpp's. All values are 8-bit codes, all
// arithmetic is signed 32-bit: sum |k| <= 2^22, so |sum k s| <= 2^22 * 255, and with 255 * 65536 of bias and the rounding half the largest
// magnitude is 1 086 291 968 < 2^31. Every partial sum obeys the same bound, so the order of the taps is free.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "color_filter.hpp"
#include "edge.hpp"

namespace crh {

constexpr uint32_t kConvolveMaxOrder = 15;    // CRH_MAX_CONVOLVE_ORDER
constexpr float kConvolveMaxGain = 64.0f;     // CRH_CONVOLVE_MAX_GAIN
constexpr int32_t kConvolveMaxSum = 1 << 22;  // kConvolveMaxGain * 65536: the bound of sum |k|
constexpr uint32_t kConvolveTransparent = 0;  // CRH_BLUR_EDGE_TRANSPARENT; 1, 2, 3 = PAD, REPEAT, REFLECT

// The kernel matrix as the rule uses it: k[r * order_x + c] = floor((double) kernel[r][c] / (double) divisor * 65536 + 0.5), every |k| <= 2^22
// (a signed 24-bit operand), and bias = 255 bias_k + 32768 with bias_k = floor((double) bias * 65536 + 0.5): the constant and the rounding half.
struct ConvolveCoefficients {
    int32_t k[kConvolveMaxOrder * kConvolveMaxOrder];
    int32_t bias_k, bias;
};

enum ConvolveRefusal { kConvolveOk = 0, kConvolveNonFinite, kConvolveGain };

// The one place where a float becomes a coefficient. order_x, order_y in [1, 15], divisor != 0 and |bias| <= 1 are the caller's to check;
// here: every entry, the divisor and the bias are finite, and sum |k| <= 2^22. The double quotient is compared with the gain limit before
// it is converted, so the conversion never sees a value an int32 cannot hold.
inline ConvolveRefusal convolve_quantize(const float* kernel, uint32_t order_x, uint32_t order_y, float divisor, float bias, ConvolveCoefficients* out) {
    const uint32_t n = order_x * order_y;
    if (!std::isfinite(divisor) || !std::isfinite(bias)) return kConvolveNonFinite;
    for (uint32_t t = 0; t < n; ++t)
        if (!std::isfinite(kernel[t])) return kConvolveNonFinite;
    int64_t sum = 0;
    for (uint32_t t = 0; t < n; ++t) {
        const double q = (double)kernel[t] / (double)divisor;
        if (!(std::fabs(q) <= (double)kConvolveMaxGain)) return kConvolveGain;
        out->k[t] = (int32_t)std::floor(q * 65536.0 + 0.5);
        sum += out->k[t] < 0 ? -(int64_t)out->k[t] : (int64_t)out->k[t];
    }
    if (sum > (int64_t)kConvolveMaxSum) return kConvolveGain;
    out->bias_k = (int32_t)std::floor((double)bias * 65536.0 + 0.5);
    out->bias = 255 * out->bias_k + 32768;
    return kConvolveOk;
}

// The load of one texel (r | g << 8 | b << 16 | a << 24, as the texels are): every colour code clamped to its alpha and, with PRESERVE,
// unpremultiplied by the colour filter's rule (`recip` = UnpremultiplyTable::r, in LDS on the device); the alpha stays where it is.
template <bool PRESERVE>
__host__ __device__ __forceinline__ uint32_t convolve_load(uint32_t texel, const uint32_t* recip) {
    const uint32_t a = texel >> 24;
    uint32_t out = a << 24;
    if (PRESERVE) {
        const uint32_t ra = recip[a];
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) out |= color_filter_unpremultiply((texel >> (8u * c)) & 0xFFu, a, ra) << (8u * c);
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) {
            const uint32_t code = (texel >> (8u * c)) & 0xFFu;
            out |= (code < a ? code : a) << (8u * c);
        }
    }
    return out;
}

// One tap: n[ch] += k * the channel's code of a loaded texel, for the 4 (or, with PRESERVE, the 3 colour) channels. A signed 24-bit
// multiply-add on the device (v_mad_i32_i24): |k| <= 2^22 and the code is below 2^8.
template <bool PRESERVE>
__host__ __device__ __forceinline__ void convolve_mad(int32_t* n, int32_t k, uint32_t loaded) {
#pragma unroll
    for (uint32_t ch = 0; ch < (PRESERVE ? 3u : 4u); ++ch) n[ch] += color_filter_mul(k, (int32_t)((loaded >> (8u * ch)) & 0xFFu));
}

__host__ __device__ __forceinline__ uint32_t convolve_code(int32_t n) {
    const int32_t s = n >> 16; // the floor: an arithmetic shift
    return (uint32_t)(s < 0 ? 0 : s > 255 ? 255 : s);
}

// The output stage: n = the window's sums with the bias and the rounding half in them; `centre` = the loaded texel under the output, whose
// alpha PRESERVE keeps. Without PRESERVE the colours are clamped to the new alpha; with it they are premultiplied by the colour filter's rule.
template <bool PRESERVE>
__host__ __device__ __forceinline__ uint32_t convolve_store(const int32_t* n, uint32_t centre) {
    const uint32_t v0 = convolve_code(n[0]), v1 = convolve_code(n[1]), v2 = convolve_code(n[2]);
    if (PRESERVE) {
        const uint32_t a = centre >> 24;
        return composite_fade(v0, a) | composite_fade(v1, a) << 8 | composite_fade(v2, a) << 16 | a << 24;
    }
    const uint32_t a = convolve_code(n[3]);
    return (v0 < a ? v0 : a) | (v1 < a ? v1 : a) << 8 | (v2 < a ? v2 : a) << 16 | a << 24;
}

// The rule on a whole image on the host (crh_convolve_texels): the image goes through the load stage once, then the plain loop over the
// window of every texel. The caller's bytes at any alignment; `out` holds w x h texels and is not `in`. A texel's word is assembled from
// its four bytes in memory order, r first, whatever the host's byte order.
template <bool PRESERVE>
inline void convolve_run(const uint8_t* in, uint32_t w, uint32_t h, const ConvolveCoefficients& f, uint32_t order_x, uint32_t order_y, uint32_t target_x, uint32_t target_y, uint32_t edge,
                         uint8_t* out) {
    static constexpr UnpremultiplyTable recip{};
    std::vector<uint32_t> loaded((size_t)w * h);
    for (size_t t = 0; t < loaded.size(); ++t) {
        const uint8_t* s = in + 4u * t;
        loaded[t] = convolve_load<PRESERVE>(s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24, recip.r);
    }
    std::vector<int> columns(order_x); // the source column of every kernel column, -1 for a transparent one
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            for (uint32_t c = 0; c < order_x; ++c) {
                const int x = (int)i - (int)target_x + (int)(order_x - 1u - c);
                columns[c] = edge != kConvolveTransparent ? edge_wrap(x, (int)w, edge) : (uint32_t)x < w ? x : -1;
            }
            int32_t n[4] = {f.bias, f.bias, f.bias, f.bias};
            for (uint32_t r = 0; r < order_y; ++r) {
                const int y = (int)j - (int)target_y + (int)(order_y - 1u - r);
                if (edge == kConvolveTransparent && (uint32_t)y >= h) continue;
                const uint32_t* line = loaded.data() + (size_t)(edge != kConvolveTransparent ? edge_wrap(y, (int)h, edge) : y) * w;
                for (uint32_t c = 0; c < order_x; ++c)
                    if (columns[c] >= 0) convolve_mad<PRESERVE>(n, f.k[r * order_x + c], line[columns[c]]);
            }
            const uint32_t r = convolve_store<PRESERVE>(n, loaded[(size_t)j * w + i]);
            uint8_t* d = out + ((size_t)j * w + i) * 4u;
            d[0] = (uint8_t)r, d[1] = (uint8_t)(r >> 8), d[2] = (uint8_t)(r >> 16), d[3] = (uint8_t)(r >> 24);
        }
}

} // namespace crh
