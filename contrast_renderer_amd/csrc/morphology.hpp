// csrc/morphology.hpp — the morphology rule of crh_image_morphology (include/contrast_hip.h states it), written once: the per-channel
// min / max of two packed RGBA8 texels. k_image_morph_h and k_image_morph_v (image_filter.hip) and crh_morphology_texels (image.hip, on the
// host) all call morphology_extreme, and edge.hpp's wrap. Min and max do not round, so there is no arithmetic to state beyond them: the
// values are the 8-bit codes as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "edge.hpp"

namespace crh {

constexpr uint32_t kMorphologyMaxRadius = 192; // CRH_MAX_MORPHOLOGY_RADIUS
constexpr uint32_t kMorphologyErode = 0, kMorphologyDilate = 1; // crh_morphology_op
constexpr uint32_t kMorphologyTransparent = 0; // CRH_BLUR_EDGE_TRANSPARENT; 1, 2, 3 = PAD, REPEAT, REFLECT

// A texel r | g << 8 | b << 16 | a << 24 as two words of two 16-bit fields, rb = r | b << 16 and ga = g | a << 16 (k_image_blur_h's split):
// the min or max of two such words per field is one v_pk_min_u16 / v_pk_max_u16 on the device, so a texel costs two instructions and is
// never unpacked to four words.
struct MorphologyTexel {
    uint32_t rb, ga;
};
__host__ __device__ __forceinline__ MorphologyTexel morphology_split(uint32_t texel) { return MorphologyTexel{texel & 0x00FF00FFu, (texel >> 8) & 0x00FF00FFu}; }
__host__ __device__ __forceinline__ uint32_t morphology_merge(MorphologyTexel t) { return t.rb | t.ga << 8; }

typedef unsigned short morphology_u16x2 __attribute__((ext_vector_type(2)));
template <bool DILATE>
__host__ __device__ __forceinline__ uint32_t morphology_extreme_pair(uint32_t a, uint32_t b) {
    const morphology_u16x2 x = __builtin_bit_cast(morphology_u16x2, a), y = __builtin_bit_cast(morphology_u16x2, b);
    return __builtin_bit_cast(uint32_t, DILATE ? __builtin_elementwise_max(x, y) : __builtin_elementwise_min(x, y));
}
// per channel: max (DILATE) or min (ERODE) of two texels
template <bool DILATE>
__host__ __device__ __forceinline__ MorphologyTexel morphology_extreme(MorphologyTexel a, MorphologyTexel b) {
    return MorphologyTexel{morphology_extreme_pair<DILATE>(a.rb, b.rb), morphology_extreme_pair<DILATE>(a.ga, b.ga)};
}

// The size of the result: DILATE under TRANSPARENT grows by the radius on every side, everything else keeps (w, h).
inline bool morphology_grows(uint32_t op, uint32_t edge) { return op == kMorphologyDilate && edge == kMorphologyTransparent; }

// The rule on a whole image on the host (crh_morphology_texels): the plain loop over the 2 r + 1 texels of a window, rows first, then columns
// (the window is a rectangle: any order gives the same bytes). The caller's bytes at any alignment; `out` holds out_w x out_h texels and is
// not `in`. A texel's word is assembled from its four bytes in memory order, r first, whatever the host's byte order.
template <bool DILATE>
inline void morphology_run(const uint8_t* in, uint32_t w, uint32_t h, uint32_t rx, uint32_t ry, uint32_t edge, uint8_t* out) {
    const bool grows = morphology_grows(DILATE ? kMorphologyDilate : kMorphologyErode, edge);
    const uint32_t out_w = w + (grows ? 2u * rx : 0u), out_h = h + (grows ? 2u * ry : 0u);
    const int ox = grows ? (int)rx : 0, oy = grows ? (int)ry : 0;
    std::vector<uint32_t> rows((size_t)out_w * h); // the horizontal pass: the result's width, the source's height
    for (uint32_t j = 0; j < h; ++j) {
        const uint8_t* line = in + (size_t)j * w * 4u;
        for (uint32_t o = 0; o < out_w; ++o) {
            MorphologyTexel m{};
            for (int k = -(int)rx; k <= (int)rx; ++k) {
                const int i = (int)o - ox + k;
                uint32_t texel = 0u; // TRANSPARENT outside the source
                if (edge != kMorphologyTransparent || (uint32_t)i < w) {
                    const uint8_t* s = line + 4u * (size_t)(edge != kMorphologyTransparent ? edge_wrap(i, (int)w, edge) : i);
                    texel = s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
                }
                m = k == -(int)rx ? morphology_split(texel) : morphology_extreme<DILATE>(m, morphology_split(texel));
            }
            rows[(size_t)j * out_w + o] = morphology_merge(m);
        }
    }
    for (uint32_t o = 0; o < out_h; ++o)
        for (uint32_t i = 0; i < out_w; ++i) {
            MorphologyTexel m{};
            for (int k = -(int)ry; k <= (int)ry; ++k) {
                const int j = (int)o - oy + k;
                uint32_t texel = 0u;
                if (edge != kMorphologyTransparent) texel = rows[(size_t)edge_wrap(j, (int)h, edge) * out_w + i];
                else if ((uint32_t)j < h) texel = rows[(size_t)j * out_w + i];
                m = k == -(int)ry ? morphology_split(texel) : morphology_extreme<DILATE>(m, morphology_split(texel));
            }
            const uint32_t r = morphology_merge(m);
            uint8_t* d = out + ((size_t)o * out_w + i) * 4u;
            d[0] = (uint8_t)r, d[1] = (uint8_t)(r >> 8), d[2] = (uint8_t)(r >> 16), d[3] = (uint8_t)(r >> 24);
        }
}

} // namespace crh
