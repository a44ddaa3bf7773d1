// csrc/image.hip — the host half of crh_image behind the C ABI of include/contrast_hip.h: create, size, mipmaps, level download, the ten
// filters (blur, composite, colour filter, morphology, convolve, lighting, turbulence, displace, distance field, resize), crop, statistics, the variable blur and the transform, with their host rules (crh_*_texels) and validators.
// Host code only: the kernels are image_filter.hip's and raster.hip's (launch.hpp), the rules are the filters' headers. Of a renderer it
// uses its device, its stream and "wait for every stream" (api_internal.hpp); what is about a frame or a paint table stays in api.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "api_internal.hpp"
#include "color_filter.hpp"
#include "composite.hpp"
#include "convolve.hpp"
#include "displace.hpp"
#include "distance.hpp"
#include "launch.hpp"
#include "lighting.hpp"
#include "morphology.hpp"
#include "regions.hpp"
#include "resize.hpp"
#include "transform.hpp"
#include "turbulence.hpp"
#include "variable_blur.hpp"

using namespace crh;

crh_status crh::new_image(crh_renderer* r, uint32_t width, uint32_t height, crh_image** out) {
    auto pixels = std::make_shared<ImagePixels>();
    HIP_TRY(hipMalloc(&pixels->p, (size_t)width * height * 4));
    crh_image* image = new crh_image;
    image->renderer = r, image->width = width, image->height = height, image->pixels = std::move(pixels);
    *out = image;
    return CRH_OK;
}

namespace {
// "<prefix>: <what>" as the last error; the prefix is the entry point that states the rule in the header
crh_status refuse(const char* prefix, const char* what, crh_status status = CRH_ERR_INVALID_ARGUMENT) {
    set_last_error(std::string(prefix) + ": " + what);
    return status;
}
crh_status check_size(const char* prefix, uint32_t width, uint32_t height) {
    if (width == 0u || height == 0u || width > kMaxImageSize || height > kMaxImageSize) return refuse(prefix, "width and height lie in [1, 16384]");
    return CRH_OK;
}

// What a filter call describes its work with (filter_call below): the stream, the result, at most one scratch allocation, launches in order.
struct FilterJob {
    const char* entry; // "crh_image_<filter>", for the text of a HIP failure
    hipStream_t stream;
    crh_image* image = nullptr;
    void* scratch_p = nullptr;
    bool ok = true;
    uint32_t* texels() const { return static_cast<uint32_t*>(image->pixels->p); }
    // the call's device scratch, with `staged_bytes` host bytes copied to its head on the stream: the caller keeps those alive until filter_call returns
    void* scratch(size_t bytes, const void* staged = nullptr, size_t staged_bytes = 0) {
        if (step(hipMalloc(&scratch_p, bytes), "hipMalloc(scratch)") && staged) step(hipMemcpyAsync(scratch_p, staged, staged_bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(staged)");
        return scratch_p;
    }
    // one launch and its hipGetLastError; nothing is issued behind a failed step
    template <typename Launch>
    void launch(const char* kernel, Launch&& enqueue) {
        if (!ok) return;
        enqueue();
        step(hipGetLastError(), kernel);
    }
    // the result of a runtime call that has just been made
    bool step(hipError_t e, const char* what) {
        if (e != hipSuccess) ok = hip_ok(e, (std::string(entry) + ": " + what).c_str());
        return ok;
    }
};
// The frame of a filter call, written once, around the validated call's `work(job)`: hipSetDevice and the result's texels (the only failures
// that return at once: nothing is in flight yet), the work, then a wait for every stream ALSO behind a failed step — the staged host bytes
// are read by the copy, and the scratch by the kernels, until the stream has drained —, the scratch freed, the image the caller's or deleted.
template <typename Work>
crh_status filter_call(const char* entry, crh_renderer* r, uint32_t width, uint32_t height, crh_image** out, Work&& work) {
    HIP_TRY(hipSetDevice(crh_internal_renderer_device(r)));
    FilterJob job{entry, renderer_stream(r)};
    const crh_status st = new_image(r, width, height, &job.image);
    if (st != CRH_OK) return st;
    work(job);
    job.step(renderer_sync(r), "sync");
    if (job.scratch_p) (void)hipFree(job.scratch_p);
    if (!job.ok) {
        delete job.image;
        return CRH_ERR_HIP;
    }
    *out = job.image;
    return CRH_OK;
}
const uint32_t* texels_of(const crh_image* image) { return static_cast<const uint32_t*>(image->pixels->p); }
} // namespace

crh_status crh_image_create(crh_renderer* r, uint32_t width, uint32_t height, const void* rgba8, crh_image** out) {
    if (!r || !rgba8 || !out || width == 0u || height == 0u || width > kMaxImageSize || height > kMaxImageSize) return CRH_ERR_INVALID_ARGUMENT;
    HIP_TRY(hipSetDevice(crh_internal_renderer_device(r)));
    crh_image* image = nullptr;
    const crh_status st = new_image(r, width, height, &image);
    if (st != CRH_OK) return st;
    if (!hip_ok(hipMemcpy(image->pixels->p, rgba8, (size_t)width * height * 4, hipMemcpyHostToDevice), "hipMemcpy(image)")) { // (returns with the bytes copied)
        delete image;
        return CRH_ERR_HIP;
    }
    *out = image;
    return CRH_OK;
}
crh_status crh_image_size(const crh_image* image, uint32_t* width, uint32_t* height) {
    if (!image || !width || !height) return CRH_ERR_INVALID_ARGUMENT;
    *width = image->width, *height = image->height;
    return CRH_OK;
}
crh_status crh_image_generate_mipmaps(crh_image* image) {
    if (!image || !image->renderer) return CRH_ERR_INVALID_ARGUMENT;
    ImagePixels& px = *image->pixels;
    if (px.chain) return CRH_OK; // (the levels are what they were: level 0 never changes)
    crh_renderer* r = image->renderer;
    const hipStream_t stream = renderer_stream(r);
    HIP_TRY(hipSetDevice(crh_internal_renderer_device(r)));
    std::vector<ImageLevel> levels;
    uint32_t w = image->width, h = image->height, words = kImageLevelTableWords;
    for (;;) {
        ImageLevel l = {};
        l.offset = levels.empty() ? 0u : words, l.width = w, l.height = h;
        l.sx = (float)w / (float)image->width, l.sy = (float)h / (float)image->height;
        if (!levels.empty()) words += w * h; // (< 2^27 + 2^25 ...: the levels >= 1 of a 16384^2 image are a third of its 2^28 texels)
        levels.push_back(l);
        if (w == 1u && h == 1u) break;
        w = std::max(1u, w >> 1), h = std::max(1u, h >> 1);
    }
    void* chain = nullptr;
    HIP_TRY(hipMalloc(&chain, (size_t)words * 4));
    bool ok = hip_ok(hipMemsetAsync(chain, 0, (size_t)kImageLevelTableWords * 4, stream), "hipMemsetAsync(levels)") &&
              hip_ok(hipMemcpyAsync(chain, levels.data(), levels.size() * sizeof(ImageLevel), hipMemcpyHostToDevice, stream), "hipMemcpyAsync(levels)");
    for (size_t l = 1; ok && l < levels.size(); ++l) {
        const uint32_t* src = l == 1 ? static_cast<const uint32_t*>(px.p) : static_cast<const uint32_t*>(chain) + levels[l - 1].offset;
        launch_image_downsample(src, levels[l - 1].width, levels[l - 1].height, static_cast<uint32_t*>(chain) + levels[l].offset, levels[l].width, levels[l].height, stream);
        ok = hip_ok(hipGetLastError(), "k_image_downsample");
    }
    ok = hip_ok(renderer_sync(r), "sync(mipmaps)") && ok; // (also behind a failed launch: `levels` is read by the copy above until the stream has drained)
    if (!ok) {
        (void)hipFree(chain);
        return CRH_ERR_HIP;
    }
    px.chain = chain, px.levels = std::move(levels);
    return CRH_OK;
}
crh_status crh_image_level_count(const crh_image* image, uint32_t* count) {
    if (!image || !count) return CRH_ERR_INVALID_ARGUMENT;
    *count = image->pixels->chain ? (uint32_t)image->pixels->levels.size() : 1u;
    return CRH_OK;
}
crh_status crh_image_download_level(const crh_image* image, uint32_t level, void* rgba8, uint32_t* width, uint32_t* height) {
    if (!image || !image->renderer) return CRH_ERR_INVALID_ARGUMENT;
    const ImagePixels& px = *image->pixels;
    if (level >= (px.chain ? (uint32_t)px.levels.size() : 1u)) return CRH_ERR_INVALID_ARGUMENT;
    const uint32_t w = level ? px.levels[level].width : image->width, h = level ? px.levels[level].height : image->height;
    if (width) *width = w;
    if (height) *height = h;
    if (!rgba8) return CRH_OK; // the size alone
    crh_renderer* r = image->renderer;
    HIP_TRY(hipSetDevice(crh_internal_renderer_device(r)));
    const void* src = level ? static_cast<const void*>(static_cast<const uint32_t*>(px.chain) + px.levels[level].offset) : px.p;
    HIP_TRY(hipMemcpyAsync(rgba8, src, (size_t)w * h * 4, hipMemcpyDeviceToHost, renderer_stream(r)));
    HIP_TRY(renderer_sync(r));
    return CRH_OK;
}
void crh_image_destroy(crh_image* image) { delete image; } // (the pixels and their mipmaps stay while a Scene's paint table names them)
// ---- blur
namespace {
static_assert(CRH_MAX_BLUR_RADIUS == kBlurMaxRadius, "k_image_blur_h's apron is the largest radius");
constexpr const char* kBlur = "crh_blur_taps";
// The tap rule of include/contrast_hip.h (crh_image_blur), in double: q[0 .. R] of one axis, summing to exactly 65536 over the 2 R + 1 positions.
crh_status blur_taps(float sigma, std::vector<uint32_t>& q) {
    if (!std::isfinite(sigma)) return CRH_ERR_NON_FINITE;
    if (sigma < 0.0f) return refuse(kBlur, "sigma is negative");
    if (sigma > CRH_MAX_BLUR_SIGMA) return refuse(kBlur, "sigma exceeds CRH_MAX_BLUR_SIGMA");
    const double s = (double)sigma;
    const uint32_t R = (uint32_t)std::ceil(3.0 * s);
    q.assign(R + 1u, 0u);
    if (R == 0u) {
        q[0] = 65536u;
        return CRH_OK;
    }
    std::vector<double> w(R + 1u);
    for (uint32_t k = 0; k <= R; ++k) w[k] = std::exp(-(double)(k * k) / (2.0 * s * s));
    double S = w[0];
    for (uint32_t k = 1; k <= R; ++k) S += 2.0 * w[k];
    int64_t total = 0;
    for (uint32_t k = 0; k <= R; ++k) {
        q[k] = (uint32_t)std::floor(w[k] / S * 65536.0 + 0.5);
        total += k == 0u ? (int64_t)q[k] : 2 * (int64_t)q[k];
    }
    // the rounding's deficit d goes to the taps next to the centre in pairs, its odd unit to the centre (|d| / 2 <= R: |d| <= 27 over (0, 64])
    const int64_t d = 65536 - total, g = d < 0 ? -1 : 1, m = std::min<int64_t>((d < 0 ? -d : d) / 2, (int64_t)R);
    for (int64_t k = 1; k <= m; ++k) q[k] = (uint32_t)((int64_t)q[k] + g);
    q[0] = (uint32_t)((int64_t)q[0] + d - 2 * g * m);
    return CRH_OK;
}
} // namespace
crh_status crh_blur_taps(float sigma, uint32_t* taps, uint32_t capacity, uint32_t* radius) {
    std::vector<uint32_t> q;
    const crh_status st = blur_taps(sigma, q);
    if (st != CRH_OK) return st;
    if (taps) {
        if (capacity < (uint32_t)q.size()) return refuse(kBlur, "capacity is below radius + 1");
        std::copy(q.begin(), q.end(), taps);
    }
    if (radius) *radius = (uint32_t)q.size() - 1u;
    return CRH_OK;
}
crh_status crh_image_blur(const crh_image* src, float sigma_x, float sigma_y, uint32_t edge, crh_image** out) {
    if (!src || !src->renderer || !out || edge > CRH_BLUR_EDGE_REFLECT) return CRH_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> qx, qy;
    crh_status st = blur_taps(sigma_x, qx);
    if (st == CRH_OK) st = blur_taps(sigma_y, qy);
    if (st != CRH_OK) return st;
    const uint32_t rx = (uint32_t)qx.size() - 1u, ry = (uint32_t)qy.size() - 1u;
    const bool grows = edge == CRH_BLUR_EDGE_TRANSPARENT;
    const uint32_t out_w = src->width + (grows ? 2u * rx : 0u), out_h = src->height + (grows ? 2u * ry : 0u);
    if (out_w > kMaxImageSize || out_h > kMaxImageSize) return refuse("crh_image_blur", "a side of the grown result exceeds 16384", CRH_ERR_UNSUPPORTED);
    // The kernels take 16-bit taps two to a word (v_dot2_u32_u16). Only q[0] = 65536 does not fit, and then every other tap is 0: that axis is the
    // identity, which the kernels do with radius 0 (the result still grows by the axis's radius under TRANSPARENT).
    const uint32_t kx = qx[0] == 65536u ? 0u : rx, ky = qy[0] == 65536u ? 0u : ry;
    // one upload, at the head of the intermediate's allocation: [q_x[0] | q_x[2 p + 1] | q_x[2 p + 2] << 16 ...] for k_image_blur_h, then, unless
    // the vertical axis is the identity, F[n] | F[n - 1] << 16 over F = q_y[|d|], d = -ky .. ky, between kBlurTapPad zeros on either side
    std::vector<uint32_t> words(1u + (kx + 1u) / 2u, 0u);
    words[0] = qx[0];
    for (uint32_t k = 1; k <= kx; ++k) words[(k + 1u) / 2u] |= qx[k] << (k % 2u ? 0 : 16);
    const size_t vertical = words.size();
    if (qy[0] != 65536u) {
        std::vector<uint32_t> F(2u * ky + 1u + 2u * kBlurTapPad, 0u);
        for (uint32_t k = 0; k <= ky; ++k) F[kBlurTapPad + ky - k] = F[kBlurTapPad + ky + k] = qy[k];
        for (size_t n = 0; n < F.size(); ++n) words.push_back(F[n] | (n ? F[n - 1] << 16 : 0u));
    }
    const size_t taps_bytes = (words.size() * 4 + 255) / 256 * 256; // (the intermediate behind them stays 256-byte aligned)
    return filter_call("crh_image_blur", src->renderer, out_w, out_h, out, [&](FilterJob& job) {
        // [the taps | the intermediate: four 16-bit values per texel, the source's rows at the result's width]
        void* scratch = job.scratch(taps_bytes + (size_t)out_w * src->height * 8, words.data(), words.size() * 4);
        const uint32_t* taps_dev = static_cast<const uint32_t*>(scratch);
        void* tmp = static_cast<char*>(scratch) + taps_bytes;
        job.launch("k_image_blur_h", [&] { launch_image_blur_h(texels_of(src), src->width, src->height, tmp, out_w, taps_dev, kx, grows ? rx : 0u, edge, job.stream); });
        job.launch("k_image_blur_v", [&] { launch_image_blur_v(tmp, src->height, job.texels(), out_w, out_h, qy[0] != 65536u ? taps_dev + vertical : nullptr, ky, grows ? ry : 0u, edge, job.stream); });
    });
}
// ---- composite
namespace {
static_assert(CRH_COMPOSITE_PLUS + 1 == kCompositeOps && CRH_BLEND_EXCLUSION + 1 == kBlendModes, "composite.hpp's table and modes are the header's");
static_assert(CRH_BLEND_NORMAL == kBlendNormal && CRH_BLEND_MULTIPLY == kBlendMultiply && CRH_BLEND_SCREEN == kBlendScreen && CRH_BLEND_OVERLAY == kBlendOverlay && CRH_BLEND_DARKEN == kBlendDarken &&
                  CRH_BLEND_LIGHTEN == kBlendLighten && CRH_BLEND_HARD_LIGHT == kBlendHardLight && CRH_BLEND_DIFFERENCE == kBlendDifference && CRH_BLEND_EXCLUSION == kBlendExclusion,
              "composite.hpp's modes are the header's");
constexpr const char* kComposite = "crh_composite_validate";
uint32_t opacity_code(float opacity) { return (uint32_t)std::floor((double)opacity * 255.0 + 0.5); }
} // namespace
crh_status crh_composite_validate(const crh_composite* how) {
    if (!how) return CRH_ERR_INVALID_ARGUMENT;
    if (how->op > CRH_COMPOSITE_PLUS) return refuse(kComposite, "op is above CRH_COMPOSITE_PLUS");
    if (how->mode > CRH_BLEND_EXCLUSION) return refuse(kComposite, "mode is above CRH_BLEND_EXCLUSION");
    if (!std::isfinite(how->opacity)) return CRH_ERR_NON_FINITE;
    if (how->opacity < 0.0f || how->opacity > 1.0f) return refuse(kComposite, "opacity is outside [0, 1]");
    return CRH_OK;
}
crh_status crh_composite_texels(const crh_composite* how, const void* source_rgba8, const void* backdrop_rgba8, uint64_t n, void* out_rgba8) {
    const crh_status st = crh_composite_validate(how);
    if (st != CRH_OK) return st;
    if (n == 0u) return CRH_OK;
    if (!source_rgba8 || !backdrop_rgba8 || !out_rgba8) return CRH_ERR_INVALID_ARGUMENT;
    const uint8_t* source = static_cast<const uint8_t*>(source_rgba8);
    const uint8_t* backdrop = static_cast<const uint8_t*>(backdrop_rgba8);
    uint8_t* out = static_cast<uint8_t*>(out_rgba8);
    const uint32_t o = opacity_code(how->opacity);
    const CompositeFactors f = composite_factors(how->op);
#define CRH_COMPOSITE_RUN(M) composite_run<M>(source, backdrop, n, o, f, out)
    CRH_COMPOSITE_MODES(how->mode, CRH_COMPOSITE_RUN)
#undef CRH_COMPOSITE_RUN
    return CRH_OK;
}
crh_status crh_image_composite(const crh_image* backdrop, const crh_image* source, const crh_composite* how, crh_image** out) {
    if (!backdrop || !backdrop->renderer || !source || !how || !out) return CRH_ERR_INVALID_ARGUMENT;
    const crh_status st = crh_composite_validate(how);
    if (st != CRH_OK) return st;
    if (source->renderer != backdrop->renderer) return refuse("crh_image_composite", "the images belong to different renderers");
    return filter_call("crh_image_composite", backdrop->renderer, backdrop->width, backdrop->height, out, [&](FilterJob& job) {
        job.launch("k_image_composite", [&] {
            launch_image_composite(texels_of(backdrop), backdrop->width, backdrop->height, texels_of(source), source->width, source->height, how->x, how->y, opacity_code(how->opacity), how->mode,
                                   how->op, job.texels(), job.stream);
        });
    });
}
// ---- colour filter
namespace {
static_assert(CRH_COLOR_MATRIX_MAX == kColorMatrixMax, "color_filter.hpp's bound is the header's");
// validates and quantises: the one way from the caller's floats to the coefficients, for the host rule and the kernel alike
crh_status color_filter_coefficients(const float* matrix, ColorFilterCoefficients* f) {
    switch (color_filter_quantize(matrix, f)) {
    case kColorFilterNonFinite: return CRH_ERR_NON_FINITE;
    case kColorFilterTooLarge: return refuse("crh_color_filter_validate", "a coefficient is outside [-CRH_COLOR_MATRIX_MAX, CRH_COLOR_MATRIX_MAX]");
    default: return CRH_OK;
    }
}
} // namespace
crh_status crh_color_filter_validate(const float* matrix, const uint8_t* tables) {
    (void)tables; // (every byte is a legal entry)
    ColorFilterCoefficients f;
    return color_filter_coefficients(matrix, &f);
}
crh_status crh_color_filter_texels(const float* matrix, const uint8_t* tables, const void* rgba8, uint64_t n, void* out) {
    ColorFilterCoefficients f;
    const crh_status st = color_filter_coefficients(matrix, &f);
    if (st != CRH_OK) return st;
    if (n == 0u) return CRH_OK;
    if (!rgba8 || !out) return CRH_ERR_INVALID_ARGUMENT;
    if (tables) color_filter_run<true>(static_cast<const uint8_t*>(rgba8), n, f, tables, static_cast<uint8_t*>(out));
    else color_filter_run<false>(static_cast<const uint8_t*>(rgba8), n, f, nullptr, static_cast<uint8_t*>(out));
    return CRH_OK;
}
crh_status crh_image_color_filter(const crh_image* src, const float* matrix, const uint8_t* tables, crh_image** out) {
    if (!src || !src->renderer || !out) return CRH_ERR_INVALID_ARGUMENT;
    ColorFilterCoefficients f;
    const crh_status st = color_filter_coefficients(matrix, &f);
    if (st != CRH_OK) return st;
    return filter_call("crh_image_color_filter", src->renderer, src->width, src->height, out, [&](FilterJob& job) {
        const void* tables_dev = tables ? job.scratch(1024, tables, 1024) : nullptr; // the caller's 1024 bytes, as they are
        job.launch("k_image_color_filter", [&] { launch_image_color_filter(texels_of(src), src->width, src->height, f, static_cast<const uint32_t*>(tables_dev), job.texels(), job.stream); });
    });
}
// ---- morphology
namespace {
static_assert(CRH_MAX_MORPHOLOGY_RADIUS == kMorphologyMaxRadius && CRH_MORPHOLOGY_ERODE == kMorphologyErode && CRH_MORPHOLOGY_DILATE == kMorphologyDilate &&
                  CRH_BLUR_EDGE_TRANSPARENT == kMorphologyTransparent,
              "morphology.hpp's limit, operators and edge are the header's");
constexpr const char* kMorphology = "crh_morphology_size";
// validates, and gives the size of the result: the one check of crh_morphology_size, crh_morphology_texels and crh_image_morphology
crh_status morphology_size(uint32_t width, uint32_t height, uint32_t op, uint32_t radius_x, uint32_t radius_y, uint32_t edge, uint32_t* out_width, uint32_t* out_height) {
    const crh_status st = check_size(kMorphology, width, height);
    if (st != CRH_OK) return st;
    if (op > CRH_MORPHOLOGY_DILATE) return refuse(kMorphology, "op is above CRH_MORPHOLOGY_DILATE");
    if (edge > CRH_BLUR_EDGE_REFLECT) return refuse(kMorphology, "edge is above CRH_BLUR_EDGE_REFLECT");
    if (radius_x > CRH_MAX_MORPHOLOGY_RADIUS || radius_y > CRH_MAX_MORPHOLOGY_RADIUS) return refuse(kMorphology, "a radius exceeds CRH_MAX_MORPHOLOGY_RADIUS");
    const bool grows = morphology_grows(op, edge);
    const uint32_t w = width + (grows ? 2u * radius_x : 0u), h = height + (grows ? 2u * radius_y : 0u);
    if (w > kMaxImageSize || h > kMaxImageSize) return refuse(kMorphology, "a side of the grown result exceeds 16384", CRH_ERR_UNSUPPORTED);
    *out_width = w, *out_height = h;
    return CRH_OK;
}
} // namespace
crh_status crh_morphology_size(uint32_t width, uint32_t height, uint32_t op, uint32_t radius_x, uint32_t radius_y, uint32_t edge, uint32_t* out_width, uint32_t* out_height) {
    if (!out_width || !out_height) return refuse(kMorphology, "a null argument");
    return morphology_size(width, height, op, radius_x, radius_y, edge, out_width, out_height); // (writes them on success only)
}
crh_status crh_morphology_texels(uint32_t width, uint32_t height, const void* rgba8, uint32_t op, uint32_t radius_x, uint32_t radius_y, uint32_t edge, void* out_rgba8) {
    if (!rgba8 || !out_rgba8) return refuse(kMorphology, "a null argument");
    if (rgba8 == out_rgba8) return refuse(kMorphology, "out_rgba8 is rgba8");
    uint32_t w = 0u, h = 0u;
    const crh_status st = morphology_size(width, height, op, radius_x, radius_y, edge, &w, &h);
    if (st != CRH_OK) return st;
    if (op == CRH_MORPHOLOGY_DILATE) morphology_run<true>(static_cast<const uint8_t*>(rgba8), width, height, radius_x, radius_y, edge, static_cast<uint8_t*>(out_rgba8));
    else morphology_run<false>(static_cast<const uint8_t*>(rgba8), width, height, radius_x, radius_y, edge, static_cast<uint8_t*>(out_rgba8));
    return CRH_OK;
}
crh_status crh_image_morphology(const crh_image* src, uint32_t op, uint32_t radius_x, uint32_t radius_y, uint32_t edge, crh_image** out) {
    if (!src || !src->renderer || !out) return refuse(kMorphology, "a null argument");
    uint32_t out_w = 0u, out_h = 0u;
    const crh_status st = morphology_size(src->width, src->height, op, radius_x, radius_y, edge, &out_w, &out_h);
    if (st != CRH_OK) return st;
    const bool grows = morphology_grows(op, edge);
    const uint32_t origin_x = grows ? radius_x : 0u, origin_y = grows ? radius_y : 0u;
    // A zero radius skips its pass (and does not grow its axis): no pass is a copy, one pass goes from the source to the result, and only two
    // passes need the intermediate — packed RGBA8, the result's width and the source's height.
    return filter_call("crh_image_morphology", src->renderer, out_w, out_h, out, [&](FilterJob& job) {
        const uint32_t* from = texels_of(src);
        uint32_t* to = job.texels();
        if (radius_x == 0u && radius_y == 0u) {
            job.step(hipMemcpyAsync(to, from, (size_t)out_w * out_h * 4, hipMemcpyDeviceToDevice, job.stream), "hipMemcpyAsync(copy)"); // (the first step: none before it has failed)
        } else if (radius_y == 0u) {
            job.launch("k_image_morph_h", [&] { launch_image_morph_h(from, src->width, src->height, to, out_w, op, radius_x, origin_x, edge, job.stream); });
        } else if (radius_x == 0u) {
            job.launch("k_image_morph_v", [&] { launch_image_morph_v(from, src->height, to, out_w, out_h, op, radius_y, origin_y, edge, job.stream); });
        } else {
            uint32_t* tmp = static_cast<uint32_t*>(job.scratch((size_t)out_w * src->height * 4));
            job.launch("k_image_morph_h", [&] { launch_image_morph_h(from, src->width, src->height, tmp, out_w, op, radius_x, origin_x, edge, job.stream); });
            job.launch("k_image_morph_v", [&] { launch_image_morph_v(tmp, src->height, to, out_w, out_h, op, radius_y, origin_y, edge, job.stream); });
        }
    });
}
// ---- convolve
namespace {
static_assert(CRH_MAX_CONVOLVE_ORDER == kConvolveMaxOrder && CRH_CONVOLVE_MAX_GAIN == kConvolveMaxGain && CRH_BLUR_EDGE_TRANSPARENT == kConvolveTransparent,
              "convolve.hpp's limits and edge are the header's");
constexpr const char* kConvolve = "crh_convolve_validate";
// validates and quantises: the one check of the four entry points, and the one way from the caller's floats to the coefficients
crh_status convolve_coefficients(const crh_convolve* how, ConvolveCoefficients* f) {
    if (!how || !how->kernel) return refuse(kConvolve, "a null argument");
    if (how->order_x == 0u || how->order_y == 0u || how->order_x > CRH_MAX_CONVOLVE_ORDER || how->order_y > CRH_MAX_CONVOLVE_ORDER) return refuse(kConvolve, "an order is outside [1, CRH_MAX_CONVOLVE_ORDER]");
    if (how->target_x >= how->order_x || how->target_y >= how->order_y) return refuse(kConvolve, "a target is not below its order");
    if (how->edge > CRH_BLUR_EDGE_REFLECT) return refuse(kConvolve, "edge is above CRH_BLUR_EDGE_REFLECT");
    if (how->preserve_alpha > 1u) return refuse(kConvolve, "preserve_alpha is above 1");
    if (how->divisor == 0.0f) return refuse(kConvolve, "divisor is 0");
    if (std::isfinite(how->bias) && std::fabs(how->bias) > 1.0f) return refuse(kConvolve, "bias is outside [-1, 1]");
    switch (convolve_quantize(how->kernel, how->order_x, how->order_y, how->divisor, how->bias, f)) {
    case kConvolveNonFinite: return CRH_ERR_NON_FINITE;
    case kConvolveGain: return refuse(kConvolve, "the kernel over the divisor exceeds CRH_CONVOLVE_MAX_GAIN: sum |k| is above 64 * 65536");
    default: return CRH_OK;
    }
}
} // namespace
crh_status crh_convolve_validate(const crh_convolve* how) {
    ConvolveCoefficients f;
    return convolve_coefficients(how, &f);
}
crh_status crh_convolve_coefficients(const crh_convolve* how, int32_t* k, uint32_t capacity, int32_t* bias_k) {
    ConvolveCoefficients f;
    const crh_status st = convolve_coefficients(how, &f);
    if (st != CRH_OK) return st;
    const uint32_t n = how->order_x * how->order_y;
    if (k && capacity < n) return refuse(kConvolve, "capacity is below order_x * order_y");
    if (k) std::copy(f.k, f.k + n, k);
    if (bias_k) *bias_k = f.bias_k;
    return CRH_OK;
}
crh_status crh_convolve_texels(uint32_t width, uint32_t height, const void* rgba8, const crh_convolve* how, void* out_rgba8) {
    if (!rgba8 || !out_rgba8) return refuse(kConvolve, "a null argument");
    if (rgba8 == out_rgba8) return refuse(kConvolve, "out_rgba8 is rgba8");
    ConvolveCoefficients f;
    crh_status st = convolve_coefficients(how, &f);
    if (st == CRH_OK) st = check_size(kConvolve, width, height);
    if (st != CRH_OK) return st;
    const uint8_t* in = static_cast<const uint8_t*>(rgba8);
    uint8_t* to = static_cast<uint8_t*>(out_rgba8);
    if (how->preserve_alpha) convolve_run<true>(in, width, height, f, how->order_x, how->order_y, how->target_x, how->target_y, how->edge, to);
    else convolve_run<false>(in, width, height, f, how->order_x, how->order_y, how->target_x, how->target_y, how->edge, to);
    return CRH_OK;
}
crh_status crh_image_convolve(const crh_image* src, const crh_convolve* how, crh_image** out) {
    if (!src || !src->renderer || !out) return refuse(kConvolve, "a null argument");
    ConvolveCoefficients f;
    crh_status st = convolve_coefficients(how, &f);
    if (st == CRH_OK) st = check_size(kConvolve, src->width, src->height);
    if (st != CRH_OK) return st;
    return filter_call("crh_image_convolve", src->renderer, src->width, src->height, out, [&](FilterJob& job) {
        job.launch("k_image_convolve", [&] {
            launch_image_convolve(texels_of(src), src->width, src->height, f, how->order_x, how->order_y, how->target_x, how->target_y, how->edge, how->preserve_alpha != 0u, job.texels(), job.stream);
        });
    });
}
// ---- lighting
namespace {
static_assert(CRH_LIGHTING_DIFFUSE == kLightingDiffuse && CRH_LIGHTING_SPECULAR == kLightingSpecular && CRH_LIGHT_DISTANT == kLightDistant && CRH_LIGHT_POINT == kLightPoint &&
                  CRH_LIGHT_SPOT == kLightSpot && CRH_BLUR_EDGE_TRANSPARENT == kLightingTransparent,
              "lighting.hpp's ops, lights and edge are the header's");
constexpr const char* kLighting = "crh_lighting_validate";
// validates and prepares: the one check of the three entry points, and the one way from the caller's floats to the rule's constants.
// Only the fields that op and light use are read: first whether they are finite, then their ranges.
crh_status lighting_constants(const crh_lighting* how, LightingConstants* f) {
    if (!how) return refuse(kLighting, "a null argument");
    if (how->op > CRH_LIGHTING_SPECULAR) return refuse(kLighting, "op is above CRH_LIGHTING_SPECULAR");
    if (how->light > CRH_LIGHT_SPOT) return refuse(kLighting, "light is above CRH_LIGHT_SPOT");
    if (how->edge > CRH_BLUR_EDGE_REFLECT) return refuse(kLighting, "edge is above CRH_BLUR_EDGE_REFLECT");
    const bool specular = how->op == CRH_LIGHTING_SPECULAR, distant = how->light == CRH_LIGHT_DISTANT, spot = how->light == CRH_LIGHT_SPOT;
    bool finite = std::isfinite(how->surface_scale) && std::isfinite(how->constant) && (!specular || std::isfinite(how->specular_exponent));
    for (int c = 0; c < 3; ++c) finite = finite && std::isfinite(how->color[c]);
    if (distant) finite = finite && std::isfinite(how->azimuth) && std::isfinite(how->elevation);
    else
        for (int c = 0; c < 3; ++c) finite = finite && std::isfinite(how->position[c]);
    if (spot) {
        for (int c = 0; c < 3; ++c) finite = finite && std::isfinite(how->points_at[c]);
        finite = finite && std::isfinite(how->spot_exponent) && std::isfinite(how->cone_angle);
    }
    if (!finite) return CRH_ERR_NON_FINITE;
    if (std::fabs(how->surface_scale) > 256.0f) return refuse(kLighting, "surface_scale is outside [-256, 256]");
    if (how->constant < 0.0f || how->constant > 256.0f) return refuse(kLighting, "constant is outside [0, 256]");
    if (specular && (how->specular_exponent < 1.0f || how->specular_exponent > 128.0f)) return refuse(kLighting, "specular_exponent is outside [1, 128]");
    for (int c = 0; c < 3; ++c)
        if (how->color[c] < 0.0f || how->color[c] > 1.0f) return refuse(kLighting, "a colour is outside [0, 1]");
    if (distant) {
        if (std::fabs(how->azimuth) > 3600.0f || std::fabs(how->elevation) > 3600.0f) return refuse(kLighting, "azimuth or elevation is outside [-3600, 3600]");
    } else {
        for (int c = 0; c < 3; ++c)
            if (std::fabs(how->position[c]) > 1048576.0f) return refuse(kLighting, "a position is outside [-2^20, 2^20]");
    }
    if (spot) {
        for (int c = 0; c < 3; ++c)
            if (std::fabs(how->points_at[c]) > 1048576.0f) return refuse(kLighting, "a points_at is outside [-2^20, 2^20]");
        if (how->points_at[0] == how->position[0] && how->points_at[1] == how->position[1] && how->points_at[2] == how->position[2]) return refuse(kLighting, "points_at is position");
        if (how->spot_exponent < 0.0f || how->spot_exponent > 128.0f) return refuse(kLighting, "spot_exponent is outside [0, 128]");
        if (how->cone_angle < 0.0f || how->cone_angle > 90.0f) return refuse(kLighting, "cone_angle is neither 0 nor in (0, 90]");
    }
    lighting_prepare(how->op, how->light, how->surface_scale, how->constant, how->specular_exponent, how->color, how->azimuth, how->elevation, how->position, how->points_at,
                     how->spot_exponent, how->cone_angle, f);
    return CRH_OK;
}
} // namespace
crh_status crh_lighting_validate(const crh_lighting* how) {
    LightingConstants f;
    return lighting_constants(how, &f);
}
crh_status crh_lighting_texels(uint32_t width, uint32_t height, const void* rgba8, const crh_lighting* how, void* out_rgba8) {
    if (!rgba8 || !out_rgba8) return refuse(kLighting, "a null argument");
    if (rgba8 == out_rgba8) return refuse(kLighting, "out_rgba8 is rgba8");
    LightingConstants f;
    crh_status st = lighting_constants(how, &f);
    if (st == CRH_OK) st = check_size(kLighting, width, height);
    if (st != CRH_OK) return st;
    lighting_run(static_cast<const uint8_t*>(rgba8), width, height, f, how->op, how->light, how->edge, static_cast<uint8_t*>(out_rgba8));
    return CRH_OK;
}
crh_status crh_image_lighting(const crh_image* src, const crh_lighting* how, crh_image** out) {
    if (!src || !src->renderer || !out) return refuse(kLighting, "a null argument");
    LightingConstants f;
    crh_status st = lighting_constants(how, &f);
    if (st == CRH_OK) st = check_size(kLighting, src->width, src->height);
    if (st != CRH_OK) return st;
    return filter_call("crh_image_lighting", src->renderer, src->width, src->height, out, [&](FilterJob& job) {
        job.launch("k_image_lighting", [&] { launch_image_lighting(texels_of(src), src->width, src->height, f, how->op, how->light, how->edge, job.texels(), job.stream); });
    });
}
// ---- turbulence
namespace {
static_assert(CRH_TURBULENCE_FRACTAL_NOISE == kTurbulenceFractalNoise && CRH_TURBULENCE_TURBULENCE == kTurbulenceTurbulence && CRH_MAX_TURBULENCE_OCTAVES == kTurbulenceMaxOctaves,
              "turbulence.hpp's kinds and limit are the header's");
constexpr const char* kTurbulence = "crh_turbulence_validate";
// the one check of the fields, for the four entry points
crh_status turbulence_fields(const crh_turbulence* how) {
    if (!how) return refuse(kTurbulence, "a null argument");
    if (how->kind > CRH_TURBULENCE_TURBULENCE) return refuse(kTurbulence, "kind is above CRH_TURBULENCE_TURBULENCE");
    if (how->stitch > 1u) return refuse(kTurbulence, "stitch is neither 0 nor 1");
    if (how->opaque > 1u) return refuse(kTurbulence, "opaque is neither 0 nor 1");
    if (how->octaves > CRH_MAX_TURBULENCE_OCTAVES) return refuse(kTurbulence, "octaves is above CRH_MAX_TURBULENCE_OCTAVES");
    for (int c = 0; c < 2; ++c)
        if (!std::isfinite(how->base_frequency[c]) || !std::isfinite(how->offset[c])) return refuse(kTurbulence, "a frequency or an offset is not finite", CRH_ERR_NON_FINITE);
    for (int c = 0; c < 2; ++c)
        if (how->base_frequency[c] < 0.0f || how->base_frequency[c] > CRH_TURBULENCE_MAX_FREQUENCY) return refuse(kTurbulence, "a base_frequency is outside [0, 4]");
    for (int c = 0; c < 2; ++c)
        if (std::fabs(how->offset[c]) > CRH_TURBULENCE_MAX_OFFSET) return refuse(kTurbulence, "an offset is outside [-65536, 65536]");
    return CRH_OK;
}
// validates a whole call and prepares it: the one way from the caller's floats to the rule's constants
crh_status turbulence_constants(uint32_t width, uint32_t height, const crh_turbulence* how, TurbulenceConstants* f) {
    crh_status st = turbulence_fields(how);
    if (st == CRH_OK) st = check_size(kTurbulence, width, height);
    if (st != CRH_OK) return st;
    turbulence_prepare(width, height, how->octaves, how->stitch != 0u, how->base_frequency, how->offset, f);
    return CRH_OK;
}
} // namespace
crh_status crh_turbulence_validate(const crh_turbulence* how) { return turbulence_fields(how); }
crh_status crh_turbulence_tables(int32_t seed, uint8_t lattice[256], double gradient[4 * 256 * 2]) {
    if (!lattice || !gradient) return refuse(kTurbulence, "a null argument");
    TurbulenceTables t;
    turbulence_make_tables(seed, &t);
    std::memcpy(lattice, t.lattice, sizeof(t.lattice));
    std::memcpy(gradient, t.gradient, sizeof(t.gradient));
    return CRH_OK;
}
crh_status crh_turbulence_texels(uint32_t width, uint32_t height, const crh_turbulence* how, void* out_rgba8) {
    if (!out_rgba8) return refuse(kTurbulence, "a null argument");
    TurbulenceConstants f;
    const crh_status st = turbulence_constants(width, height, how, &f);
    if (st != CRH_OK) return st;
    TurbulenceTables t;
    turbulence_make_tables(how->seed, &t);
    turbulence_run(t, f, how->kind, how->opaque != 0u, width, height, static_cast<uint8_t*>(out_rgba8));
    return CRH_OK;
}
crh_status crh_image_turbulence(crh_renderer* r, uint32_t width, uint32_t height, const crh_turbulence* how, crh_image** out) {
    if (!r || !out) return refuse(kTurbulence, "a null argument");
    TurbulenceConstants f;
    const crh_status st = turbulence_constants(width, height, how, &f);
    if (st != CRH_OK) return st;
    TurbulenceTables t;
    turbulence_make_tables(how->seed, &t);
    return filter_call("crh_image_turbulence", r, width, height, out, [&](FilterJob& job) {
        const TurbulenceTables* tables_dev = static_cast<const TurbulenceTables*>(job.scratch(sizeof(t), &t, sizeof(t)));
        job.launch("k_image_turbulence", [&] { launch_image_turbulence(tables_dev, width, height, f, how->kind, how->opaque != 0u, job.texels(), job.stream); });
    });
}
// ---- displace
namespace {
static_assert(CRH_MAX_DISPLACE_SCALE == kDisplaceMaxScale && CRH_FILTER_NEAREST == kDisplaceNearest && CRH_FILTER_LINEAR == kDisplaceLinear && CRH_CHANNEL_A == kDisplaceAlpha &&
                  CRH_BLUR_EDGE_TRANSPARENT == kDisplaceTransparent,
              "displace.hpp's limit, filters, alpha channel and edge are the header's");
constexpr const char* kDisplace = "crh_displace_validate";
// validates the fields and prepares them: the one check of the four entry points, and the one way from the caller's floats to the rule's constants
crh_status displace_constants(const crh_displace* how, DisplaceConstants* f) {
    if (!how) return refuse(kDisplace, "a null argument");
    if (how->x_channel > CRH_CHANNEL_A || how->y_channel > CRH_CHANNEL_A) return refuse(kDisplace, "a channel is above CRH_CHANNEL_A");
    if (how->filter != CRH_FILTER_NEAREST && how->filter != CRH_FILTER_LINEAR) return refuse(kDisplace, "filter is neither CRH_FILTER_NEAREST nor CRH_FILTER_LINEAR");
    if (how->edge > CRH_BLUR_EDGE_REFLECT) return refuse(kDisplace, "edge is above CRH_BLUR_EDGE_REFLECT");
    if (!std::isfinite(how->scale[0]) || !std::isfinite(how->scale[1])) return refuse(kDisplace, "a scale is not finite", CRH_ERR_NON_FINITE);
    if (std::fabs(how->scale[0]) > CRH_MAX_DISPLACE_SCALE || std::fabs(how->scale[1]) > CRH_MAX_DISPLACE_SCALE) return refuse(kDisplace, "a scale is outside [-1024, 1024]");
    f->k[0] = displace_k(how->scale[0]), f->k[1] = displace_k(how->scale[1]);
    f->channel[0] = how->x_channel, f->channel[1] = how->y_channel, f->filter = how->filter, f->edge = how->edge;
    return CRH_OK;
}
} // namespace
crh_status crh_displace_validate(const crh_displace* how) {
    DisplaceConstants f;
    return displace_constants(how, &f);
}
crh_status crh_displace_offset(const crh_displace* how, uint32_t code_x, uint32_t code_y, int32_t q[2]) {
    if (!q) return refuse(kDisplace, "a null argument");
    DisplaceConstants f;
    const crh_status st = displace_constants(how, &f);
    if (st != CRH_OK) return st;
    if (code_x > 255u || code_y > 255u) return refuse(kDisplace, "a code is above 255");
    q[0] = displace_q(f.k[0], code_x), q[1] = displace_q(f.k[1], code_y);
    return CRH_OK;
}
crh_status crh_displace_texels(uint32_t width, uint32_t height, const void* rgba8, const void* map_rgba8, const crh_displace* how, void* out_rgba8) {
    if (!rgba8 || !map_rgba8 || !out_rgba8) return refuse(kDisplace, "a null argument");
    DisplaceConstants f;
    crh_status st = displace_constants(how, &f);
    if (st == CRH_OK) st = check_size(kDisplace, width, height);
    if (st != CRH_OK) return st;
    if (out_rgba8 == rgba8 || out_rgba8 == map_rgba8) return refuse(kDisplace, "out_rgba8 is rgba8 or map_rgba8");
    const uint8_t* in = static_cast<const uint8_t*>(rgba8);
    const uint8_t* map = static_cast<const uint8_t*>(map_rgba8);
    if (f.filter == kDisplaceLinear) displace_run<kDisplaceLinear>(in, map, width, height, f, static_cast<uint8_t*>(out_rgba8));
    else displace_run<kDisplaceNearest>(in, map, width, height, f, static_cast<uint8_t*>(out_rgba8));
    return CRH_OK;
}
crh_status crh_image_displace(const crh_image* src, const crh_image* map, const crh_displace* how, crh_image** out) {
    if (!src || !map || !out) return refuse(kDisplace, "a null argument");
    DisplaceConstants f;
    crh_status st = displace_constants(how, &f); // (the fields before the images: a refused `how` does not look at them)
    if (st == CRH_OK && !src->renderer) st = refuse(kDisplace, "a null argument");
    if (st == CRH_OK) st = check_size(kDisplace, src->width, src->height);
    if (st != CRH_OK) return st;
    if (map->width != src->width || map->height != src->height) return refuse(kDisplace, "the map is of another size");
    if (map->renderer != src->renderer) return refuse(kDisplace, "the images belong to different renderers");
    return filter_call("crh_image_displace", src->renderer, src->width, src->height, out, [&](FilterJob& job) {
        job.launch("k_image_displace", [&] { launch_image_displace(texels_of(src), texels_of(map), src->width, src->height, f, job.texels(), job.stream); });
    });
}
// ---- distance field
namespace {
static_assert(CRH_MAX_DISTANCE_SPREAD == kDistanceMaxSpread && CRH_DISTANCE_OUTSIDE == kDistanceOutside && CRH_DISTANCE_INSIDE == kDistanceInside && CRH_BLUR_EDGE_TRANSPARENT == kDistanceTransparent &&
                  CRH_CHANNEL_A == 3,
              "distance.hpp's limit, modes, edge and channel shift are the header's");
constexpr const char* kDistance = "crh_distance_validate";
// validates the fields and prepares them: the one check of the five entry points
crh_status distance_constants(const crh_distance* how, DistanceConstants* f) {
    if (!how) return refuse(kDistance, "a null argument");
    if (how->mode > CRH_DISTANCE_INSIDE) return refuse(kDistance, "mode is above CRH_DISTANCE_INSIDE");
    if (how->channel > CRH_CHANNEL_A) return refuse(kDistance, "channel is above CRH_CHANNEL_A");
    if (how->threshold < 1u || how->threshold > 255u) return refuse(kDistance, "threshold is outside [1, 255]");
    if (how->spread < 1u || how->spread > CRH_MAX_DISTANCE_SPREAD) return refuse(kDistance, "spread is outside [1, CRH_MAX_DISTANCE_SPREAD]");
    if (how->edge > CRH_BLUR_EDGE_REFLECT) return refuse(kDistance, "edge is above CRH_BLUR_EDGE_REFLECT");
    f->mode = how->mode, f->shift = 8u * how->channel, f->threshold = how->threshold, f->spread = how->spread, f->edge = how->edge;
    return CRH_OK;
}
// The checks after the null arguments, in the header's order, in two steps, so that crh_distance_texels can name an output that is
// its input between them: the fields and the source's size, then the result's size (written on success only).
crh_status distance_source(uint32_t width, uint32_t height, const crh_distance* how, DistanceConstants* f) {
    const crh_status st = distance_constants(how, f);
    return st != CRH_OK ? st : check_size(kDistance, width, height);
}
crh_status distance_result(uint32_t width, uint32_t height, const DistanceConstants& f, uint32_t* out_width, uint32_t* out_height) {
    const uint32_t grown = distance_grows(f.mode, f.edge) ? 2u * f.spread : 0u;
    if (width + grown > kMaxImageSize || height + grown > kMaxImageSize) return refuse(kDistance, "a side of the grown result exceeds 16384", CRH_ERR_UNSUPPORTED);
    *out_width = width + grown, *out_height = height + grown;
    return CRH_OK;
}
} // namespace
crh_status crh_distance_validate(const crh_distance* how) {
    DistanceConstants f;
    return distance_constants(how, &f);
}
crh_status crh_distance_code(const crh_distance* how, uint64_t squared_distance, uint32_t* code) {
    if (!how || !code) return refuse(kDistance, "a null argument");
    DistanceConstants f;
    const crh_status st = distance_constants(how, &f);
    if (st != CRH_OK) return st;
    DistanceThresholds thresholds;
    distance_thresholds(f.spread, &thresholds);
    const uint64_t cap = (uint64_t)f.spread * f.spread; // every D2 >= spread^2 gives 255
    *code = distance_texel(distance_code(thresholds.t, (uint32_t)(squared_distance < cap ? squared_distance : cap)), f.mode) & 0xFFu;
    return CRH_OK;
}
crh_status crh_distance_size(uint32_t width, uint32_t height, const crh_distance* how, uint32_t* out_width, uint32_t* out_height) {
    if (!how || !out_width || !out_height) return refuse(kDistance, "a null argument");
    DistanceConstants f;
    const crh_status st = distance_source(width, height, how, &f);
    return st != CRH_OK ? st : distance_result(width, height, f, out_width, out_height);
}
crh_status crh_distance_texels(uint32_t width, uint32_t height, const void* rgba8, const crh_distance* how, void* out_rgba8) {
    if (!rgba8 || !how || !out_rgba8) return refuse(kDistance, "a null argument");
    DistanceConstants f;
    uint32_t w = 0u, h = 0u;
    crh_status st = distance_source(width, height, how, &f);
    if (st != CRH_OK) return st;
    if (out_rgba8 == rgba8) return refuse(kDistance, "out_rgba8 is rgba8");
    st = distance_result(width, height, f, &w, &h);
    if (st != CRH_OK) return st;
    distance_run(static_cast<const uint8_t*>(rgba8), width, height, f, static_cast<uint8_t*>(out_rgba8));
    return CRH_OK;
}
crh_status crh_image_distance_field(const crh_image* src, const crh_distance* how, crh_image** out) {
    if (!src || !how || !out) return refuse(kDistance, "a null argument");
    DistanceConstants f;
    crh_status st = distance_constants(how, &f); // (the fields before the image: a refused `how` does not look at it)
    if (st == CRH_OK && !src->renderer) st = refuse(kDistance, "a null argument");
    uint32_t out_w = 0u, out_h = 0u;
    if (st == CRH_OK) st = check_size(kDistance, src->width, src->height);
    if (st == CRH_OK) st = distance_result(src->width, src->height, f, &out_w, &out_h);
    if (st != CRH_OK) return st;
    const uint32_t origin = distance_grows(f.mode, f.edge) ? f.spread : 0u;
    DistanceThresholds thresholds; // (alive until filter_call returns: the staged bytes of the scratch)
    distance_thresholds(f.spread, &thresholds);
    // one scratch: the thresholds at its head, then g, a byte of column distance per texel of the result
    return filter_call("crh_image_distance_field", src->renderer, out_w, out_h, out, [&](FilterJob& job) {
        uint8_t* scratch = static_cast<uint8_t*>(job.scratch(sizeof thresholds + (size_t)out_w * out_h, &thresholds, sizeof thresholds));
        uint8_t* g = scratch ? scratch + sizeof thresholds : nullptr; // (a failed allocation: no launch follows)
        job.launch("k_image_distance_v", [&] { launch_image_distance_v(texels_of(src), src->width, src->height, g, out_w, out_h, origin, f, job.stream); });
        job.launch("k_image_distance_h", [&] { launch_image_distance_h(g, out_w, out_h, reinterpret_cast<const uint32_t*>(scratch), f, job.texels(), job.stream); });
    });
}
// ---- resize
namespace {
static_assert(CRH_MAX_RESIZE_TAPS == kResizeMaxTaps && CRH_RESIZE_BOX == kResizeBox && CRH_RESIZE_TRIANGLE == kResizeTriangle && CRH_RESIZE_CATMULL_ROM == kResizeCatmullRom &&
                  CRH_RESIZE_MITCHELL == kResizeMitchell && CRH_RESIZE_LANCZOS3 == kResizeLanczos3 && CRH_RESIZE_LANCZOS3 + 1 == kResizeFilters,
              "resize.hpp's cap and filters are the header's");
constexpr const char* kResize = "crh_resize_taps";
// validates an axis and builds its taps: the one check of the three entry points behind their null arguments
crh_status resize_taps(uint32_t n, uint32_t m, uint32_t filter, ResizeAxis* axis) {
    if (n == 0u || m == 0u || n > kMaxImageSize || m > kMaxImageSize) return refuse(kResize, "a side lies outside [1, 16384]");
    if (filter > CRH_RESIZE_LANCZOS3) return refuse(kResize, "filter is above CRH_RESIZE_LANCZOS3");
    switch (resize_axis(n, m, filter, axis, nullptr)) {
    case kResizeAxisTaps: return refuse(kResize, "an output's window exceeds CRH_MAX_RESIZE_TAPS texels: chain two calls", CRH_ERR_UNSUPPORTED);
    case kResizeAxisGain: return refuse(kResize, "an output's taps exceed sum |q| <= 32768", CRH_ERR_UNSUPPORTED);
    default: return CRH_OK;
    }
}
// both axes of a call: the sizes and the filter are checked for both before either axis is built, in the header's order
crh_status resize_axes(uint32_t width, uint32_t height, uint32_t out_width, uint32_t out_height, uint32_t filter, ResizeAxis* ax, ResizeAxis* ay) {
    crh_status st = check_size(kResize, width, height);
    if (st == CRH_OK) st = check_size(kResize, out_width, out_height);
    if (st == CRH_OK) st = resize_taps(width, out_width, filter, ax);
    if (st == CRH_OK && height == width && out_height == out_width) *ay = *ax; // (the same axis: its taps are built once)
    else if (st == CRH_OK) st = resize_taps(height, out_height, filter, ay);
    return st;
}
} // namespace
crh_status crh_resize_taps(uint32_t n, uint32_t m, uint32_t filter, int32_t* first, uint16_t* count, int16_t* taps, uint64_t capacity, uint64_t* total) {
    const bool arrays = first && count && taps;
    if ((!arrays && (first || count || taps)) || (!arrays && !total)) return refuse(kResize, "a null argument");
    ResizeAxis axis;
    const crh_status st = resize_taps(n, m, filter, &axis);
    if (st != CRH_OK) return st;
    if (arrays) {
        if (capacity < axis.taps.size()) return refuse(kResize, "capacity is below the total");
        std::copy(axis.first.begin(), axis.first.end(), first);
        std::copy(axis.count.begin(), axis.count.end(), count);
        std::copy(axis.taps.begin(), axis.taps.end(), taps);
    }
    if (total) *total = axis.taps.size();
    return CRH_OK;
}
crh_status crh_resize_texels(uint32_t width, uint32_t height, const void* rgba8, uint32_t out_width, uint32_t out_height, uint32_t filter, void* out_rgba8) {
    if (!rgba8 || !out_rgba8) return refuse(kResize, "a null argument");
    if (rgba8 == out_rgba8) return refuse(kResize, "out_rgba8 is rgba8");
    ResizeAxis ax, ay;
    const crh_status st = resize_axes(width, height, out_width, out_height, filter, &ax, &ay);
    if (st != CRH_OK) return st;
    resize_run(static_cast<const uint8_t*>(rgba8), width, height, ax, ay, out_width, out_height, static_cast<uint8_t*>(out_rgba8));
    return CRH_OK;
}
crh_status crh_image_resize(const crh_image* src, uint32_t width, uint32_t height, uint32_t filter, crh_image** out) {
    if (!src || !src->renderer || !out) return refuse(kResize, "a null argument");
    ResizeAxis ax, ay;
    const crh_status st = resize_axes(src->width, src->height, width, height, filter, &ax, &ay);
    if (st != CRH_OK) return st;
    ResizeTable tx, ty;
    if (!resize_table(ax, src->width, &tx) || !resize_table(ay, src->height, &ty)) return refuse(kResize, "a tap lies outside the source", CRH_ERR_UNSUPPORTED); // (the builder's assertion: never met)
    // one upload, at the head of the intermediate's allocation: [the horizontal table | the vertical table], resize.hpp's layout
    std::vector<uint32_t> words(tx.words);
    words.insert(words.end(), ty.words.begin(), ty.words.end());
    const size_t tables_bytes = (words.size() * 4 + 255) / 256 * 256; // (the intermediate behind them stays 256-byte aligned)
    return filter_call("crh_image_resize", src->renderer, width, height, out, [&](FilterJob& job) {
        // [the tables | the intermediate: four 16-bit values per texel, the source's rows at the result's width]
        void* scratch = job.scratch(tables_bytes + (size_t)width * src->height * 8, words.data(), words.size() * 4);
        const uint32_t* table_x = static_cast<const uint32_t*>(scratch);
        const uint32_t* table_y = table_x + tx.words.size();
        void* tmp = static_cast<char*>(scratch) + tables_bytes;
        job.launch("k_image_resize_h", [&] { launch_image_resize_h(texels_of(src), src->width, src->height, tmp, width, table_x, tx.pairs, job.stream); });
        job.launch("k_image_resize_v", [&] { launch_image_resize_v(tmp, src->height, job.texels(), width, height, table_y, ty.pairs, job.stream); });
    });
}
// ---- regions and statistics
namespace {
static_assert(sizeof(crh_image_stats) == kStatsWords * sizeof(uint32_t) && offsetof(crh_image_stats, x0) == kStatsX0 * sizeof(uint32_t) && offsetof(crh_image_stats, count) == kStatsCount * sizeof(uint32_t),
              "regions.hpp's words are the header's struct");
constexpr const char* kCrop = "crh_crop_texels";
constexpr const char* kStatistics = "crh_statistics_texels";
// The checks after the null arguments, in the header's order: the channel, the threshold, then the size
crh_status statistics_constants(uint32_t width, uint32_t height, uint32_t channel, uint32_t threshold, StatsConstants* f) {
    if (channel > CRH_CHANNEL_A) return refuse(kStatistics, "channel is above CRH_CHANNEL_A");
    if (threshold < 1u || threshold > 255u) return refuse(kStatistics, "threshold is outside [1, 255]");
    f->shift = 8u * channel, f->threshold = threshold;
    return check_size(kStatistics, width, height);
}
} // namespace
crh_status crh_crop_texels(uint32_t width, uint32_t height, const void* rgba8, int32_t x, int32_t y, uint32_t out_width, uint32_t out_height, void* out_rgba8) {
    if (!rgba8 || !out_rgba8) return refuse(kCrop, "a null argument");
    crh_status st = check_size(kCrop, width, height);
    if (st == CRH_OK) st = check_size(kCrop, out_width, out_height);
    if (st != CRH_OK) return st;
    if (out_rgba8 == rgba8) return refuse(kCrop, "out_rgba8 is rgba8");
    crop_run(static_cast<const uint8_t*>(rgba8), width, height, x, y, out_width, out_height, static_cast<uint8_t*>(out_rgba8));
    return CRH_OK;
}
crh_status crh_image_crop(const crh_image* src, int32_t x, int32_t y, uint32_t width, uint32_t height, crh_image** out) {
    if (!src || !src->renderer || !out) return refuse(kCrop, "a null argument");
    const crh_status st = check_size(kCrop, width, height);
    if (st != CRH_OK) return st;
    return filter_call("crh_image_crop", src->renderer, width, height, out, [&](FilterJob& job) {
        job.launch("k_image_crop", [&] { launch_image_crop(texels_of(src), src->width, src->height, x, y, job.texels(), width, height, job.stream); });
    });
}
crh_status crh_statistics_texels(uint32_t width, uint32_t height, const void* rgba8, uint32_t channel, uint32_t threshold, crh_image_stats* out) {
    if (!rgba8 || !out) return refuse(kStatistics, "a null argument");
    StatsConstants f;
    const crh_status st = statistics_constants(width, height, channel, threshold, &f);
    if (st != CRH_OK) return st;
    statistics_run(static_cast<const uint8_t*>(rgba8), width, height, f, out->histogram);
    return CRH_OK;
}
crh_status crh_image_statistics(const crh_image* src, uint32_t channel, uint32_t threshold, crh_image_stats* out) {
    if (!src || !src->renderer || !out) return refuse(kStatistics, "a null argument");
    StatsConstants f;
    const crh_status st = statistics_constants(src->width, src->height, channel, threshold, &f);
    if (st != CRH_OK) return st;
    // filter_call's frame without a result image: the device, the one scratch — [a partial result per workgroup | the result] —, the two
    // kernels, the 4116 bytes to a host copy of the struct, the wait also behind a failed step, the scratch freed; *out is written last.
    crh_renderer* r = src->renderer;
    HIP_TRY(hipSetDevice(crh_internal_renderer_device(r)));
    FilterJob job{"crh_image_statistics", renderer_stream(r)};
    const uint32_t partials = image_stats_partials(src->width, src->height);
    uint32_t* scratch = static_cast<uint32_t*>(job.scratch((size_t)(partials + 1u) * sizeof(crh_image_stats)));
    uint32_t* result = scratch ? scratch + (size_t)partials * kStatsWords : nullptr; // (a failed allocation: no launch follows)
    crh_image_stats stats;
    job.launch("k_image_stats", [&] { launch_image_stats(texels_of(src), src->width, src->height, f, scratch, job.stream); });
    job.launch("k_image_stats_merge", [&] { launch_image_stats_merge(scratch, partials, result, job.stream); });
    if (job.ok) job.step(hipMemcpyAsync(&stats, result, sizeof stats, hipMemcpyDeviceToHost, job.stream), "hipMemcpyAsync(statistics)");
    job.step(renderer_sync(r), "sync");
    if (job.scratch_p) (void)hipFree(job.scratch_p);
    if (!job.ok) return CRH_ERR_HIP;
    *out = stats;
    return CRH_OK;
}
// ---- variable blur
namespace {
static_assert(CRH_MAX_BLUR_RADIUS == kVariableBlurMaxRadius && CRH_BLUR_EDGE_TRANSPARENT == kVariableBlurTransparent, "variable_blur.hpp's largest radius and edge are the header's");
constexpr const char* kVariableBlur = "crh_variable_blur_validate";
// the checks of the fields behind the null arguments, in the header's order: the one check of the four entry points
crh_status variable_blur_fields(const crh_variable_blur* how) {
    if (!how) return refuse(kVariableBlur, "a null argument");
    const float sigmas[4] = {how->sigma_x[0], how->sigma_x[1], how->sigma_y[0], how->sigma_y[1]};
    for (float s : sigmas)
        if (!std::isfinite(s)) return refuse(kVariableBlur, "a sigma is not finite", CRH_ERR_NON_FINITE);
    for (float s : sigmas)
        if (s < 0.0f || s > CRH_MAX_BLUR_SIGMA) return refuse(kVariableBlur, "a sigma is outside [0, CRH_MAX_BLUR_SIGMA]");
    if (how->channel > CRH_CHANNEL_A) return refuse(kVariableBlur, "channel is above CRH_CHANNEL_A");
    if (how->edge > CRH_BLUR_EDGE_REFLECT) return refuse(kVariableBlur, "edge is above CRH_BLUR_EDGE_REFLECT");
    return CRH_OK;
}
// the 256 tap sets of both axes, by the blur's own tap rule (validated fields: blur_taps refuses none of their sigmas)
crh_status variable_blur_axes(const crh_variable_blur* how, VariableBlurAxis* ax, VariableBlurAxis* ay) {
    const auto taps = [](float sigma, std::vector<uint32_t>& q) { return (int)blur_taps(sigma, q); };
    if (variable_blur_axis(how->sigma_x[0], how->sigma_x[1], taps, ax) != 0 || variable_blur_axis(how->sigma_y[0], how->sigma_y[1], taps, ay) != 0)
        return refuse(kVariableBlur, "a level's taps leave the kernels' fields", CRH_ERR_UNSUPPORTED); // (the builder's assertion: never met)
    return CRH_OK;
}
} // namespace
crh_status crh_variable_blur_validate(const crh_variable_blur* how) { return variable_blur_fields(how); }
crh_status crh_variable_blur_sigma(const crh_variable_blur* how, uint32_t code, float* sigma_x, float* sigma_y) {
    if (!how || !sigma_x || !sigma_y) return refuse(kVariableBlur, "a null argument");
    const crh_status st = variable_blur_fields(how);
    if (st != CRH_OK) return st;
    if (code > 255u) return refuse(kVariableBlur, "a code is above 255");
    *sigma_x = variable_blur_sigma(how->sigma_x[0], how->sigma_x[1], code), *sigma_y = variable_blur_sigma(how->sigma_y[0], how->sigma_y[1], code);
    return CRH_OK;
}
crh_status crh_variable_blur_texels(uint32_t width, uint32_t height, const void* rgba8, const void* mask_rgba8, const crh_variable_blur* how, void* out_rgba8) {
    if (!rgba8 || !mask_rgba8 || !how || !out_rgba8) return refuse(kVariableBlur, "a null argument");
    crh_status st = variable_blur_fields(how);
    if (st == CRH_OK) st = check_size(kVariableBlur, width, height);
    if (st != CRH_OK) return st;
    if (out_rgba8 == rgba8 || out_rgba8 == mask_rgba8) return refuse(kVariableBlur, "out_rgba8 is rgba8 or mask_rgba8");
    VariableBlurAxis ax, ay;
    st = variable_blur_axes(how, &ax, &ay);
    if (st != CRH_OK) return st;
    variable_blur_run(static_cast<const uint8_t*>(rgba8), static_cast<const uint8_t*>(mask_rgba8), width, height, ax, ay, how->channel, how->edge, static_cast<uint8_t*>(out_rgba8));
    return CRH_OK;
}
crh_status crh_image_variable_blur(const crh_image* src, const crh_image* mask, const crh_variable_blur* how, crh_image** out) {
    if (!src || !mask || !how || !out) return refuse(kVariableBlur, "a null argument");
    crh_status st = variable_blur_fields(how); // (the fields before the images: a refused `how` does not look at them)
    if (st == CRH_OK && !src->renderer) st = refuse(kVariableBlur, "a null argument");
    if (st == CRH_OK) st = check_size(kVariableBlur, src->width, src->height);
    if (st != CRH_OK) return st;
    if (mask->width != src->width || mask->height != src->height) return refuse(kVariableBlur, "the mask is of another size");
    if (mask->renderer != src->renderer) return refuse(kVariableBlur, "the images belong to different renderers");
    VariableBlurAxis ax, ay;
    st = variable_blur_axes(how, &ax, &ay);
    if (st != CRH_OK) return st;
    // one upload, at the head of the intermediate's allocation: [the x axis's entries and taps | the y axis's], variable_blur.hpp's layout
    std::vector<uint32_t> words(ax.words);
    words.insert(words.end(), ay.words.begin(), ay.words.end());
    const size_t tables_bytes = (words.size() * 4 + 255) / 256 * 256; // (the intermediate behind them stays 256-byte aligned)
    const uint32_t w = src->width, h = src->height, shift = 8u * how->channel, edge = how->edge;
    return filter_call("crh_image_variable_blur", src->renderer, w, h, out, [&](FilterJob& job) {
        // [the tables | the intermediate: four 16-bit values per texel]
        void* scratch = job.scratch(tables_bytes + (size_t)w * h * 8, words.data(), words.size() * 4);
        const uint32_t* table_x = static_cast<const uint32_t*>(scratch);
        const uint32_t* table_y = table_x + ax.words.size();
        void* tmp = static_cast<char*>(scratch) + tables_bytes;
        job.launch("k_image_variable_blur_h", [&] { launch_image_variable_blur_h(texels_of(src), texels_of(mask), w, h, tmp, table_x, ax.radius, shift, edge, job.stream); });
        job.launch("k_image_variable_blur_v", [&] { launch_image_variable_blur_v(tmp, texels_of(mask), job.texels(), w, h, table_y, shift, edge, job.stream); });
    });
}
// ---- transform
namespace {
static_assert(CRH_TRANSFORM_NEAREST == kTransformNearest && CRH_TRANSFORM_LINEAR == kTransformLinear && CRH_TRANSFORM_CUBIC == kTransformCubic && CRH_MAX_TRANSFORM_ENTRY == kTransformMaxEntry &&
                  CRH_BLUR_EDGE_TRANSPARENT == kTransformTransparent,
              "transform.hpp's filters, limit and edge are the header's");
constexpr const char* kTransform = "crh_transform_validate";
// the rows of the validation that are about a matrix, a filter and an edge: crh_transform's own and crh_transform_fit's `forward`
crh_status transform_check(const double* m, uint32_t filter, uint32_t edge) {
    if (filter > CRH_TRANSFORM_CUBIC) return refuse(kTransform, "filter is above CRH_TRANSFORM_CUBIC");
    if (edge > CRH_BLUR_EDGE_REFLECT) return refuse(kTransform, "edge is above CRH_BLUR_EDGE_REFLECT");
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(m[k])) return refuse(kTransform, "an entry of the matrix is not finite", CRH_ERR_NON_FINITE);
    for (int k = 0; k < 9; ++k)
        if (std::fabs(m[k]) > CRH_MAX_TRANSFORM_ENTRY) return refuse(kTransform, "an entry of the matrix is above 2^40 in magnitude");
    return CRH_OK;
}
// validates the fields and prepares them: the one check of the entry points that take a crh_transform
crh_status transform_constants(const crh_transform* how, TransformConstants* f) {
    if (!how) return refuse(kTransform, "a null argument");
    crh_status st = transform_check(how->matrix, how->filter, how->edge);
    if (st == CRH_OK) st = check_size(kTransform, how->width, how->height);
    if (st != CRH_OK) return st;
    std::copy(how->matrix, how->matrix + 9, f->m);
    f->filter = how->filter, f->edge = how->edge, f->projective = transform_is_affine(how->matrix) ? 0u : 1u;
    return CRH_OK;
}
template <bool PROJECTIVE>
void transform_run_filter(const uint8_t* in, uint32_t sw, uint32_t sh, const TransformConstants& f, uint32_t w, uint32_t h, uint8_t* out) {
    if (f.filter == kTransformCubic) transform_run<kTransformCubic, PROJECTIVE>(in, sw, sh, f, w, h, out);
    else if (f.filter == kTransformLinear) transform_run<kTransformLinear, PROJECTIVE>(in, sw, sh, f, w, h, out);
    else transform_run<kTransformNearest, PROJECTIVE>(in, sw, sh, f, w, h, out);
}
} // namespace
crh_status crh_transform_validate(const crh_transform* how) {
    TransformConstants f;
    return transform_constants(how, &f);
}
crh_status crh_transform_position(const crh_transform* how, uint32_t i, uint32_t j, int32_t position[2], uint32_t* visible) {
    if (!position || !visible) return refuse(kTransform, "a null argument");
    TransformConstants f;
    const crh_status st = transform_constants(how, &f);
    if (st != CRH_OK) return st;
    if (i >= how->width || j >= how->height) return refuse(kTransform, "a texel is outside the result");
    *visible = (f.projective ? transform_position<true>(f.m, i, j, &position[0], &position[1]) : transform_position<false>(f.m, i, j, &position[0], &position[1])) ? 1u : 0u;
    return CRH_OK;
}
crh_status crh_transform_fit(uint32_t width, uint32_t height, const double forward[9], uint32_t filter, uint32_t edge, crh_transform* out, int32_t origin[2]) {
    if (!forward || !out || !origin) return refuse(kTransform, "a null argument");
    crh_status st = transform_check(forward, filter, edge);
    if (st == CRH_OK) st = check_size(kTransform, width, height);
    if (st != CRH_OK) return st;
    const double a = forward[0], b = forward[1], c = forward[2], d = forward[3], e = forward[4], f = forward[5], g = forward[6], h = forward[7], i = forward[8];
    const bool affine = transform_is_affine(forward);
    // the four corners in the header's order, each min and max by comparisons
    double lo[2] = {0.0, 0.0}, hi[2] = {0.0, 0.0};
    for (int corner = 0; corner < 4; ++corner) {
        const double x = corner & 1 ? (double)width : 0.0, y = corner & 2 ? (double)height : 0.0;
        double p[2] = {(a * x + b * y) + c, (d * x + e * y) + f};
        if (!affine) {
            const double W = (g * x + h * y) + i;
            if (!(W > 0.0)) return refuse(kTransform, "a corner is behind the horizon");
            p[0] = p[0] / W, p[1] = p[1] / W;
        }
        for (int axis = 0; axis < 2; ++axis) {
            if (corner == 0 || p[axis] < lo[axis]) lo[axis] = p[axis];
            if (corner == 0 || p[axis] > hi[axis]) hi[axis] = p[axis];
        }
    }
    const double x0 = std::floor(lo[0]), x1 = std::ceil(hi[0]), y0 = std::floor(lo[1]), y1 = std::ceil(hi[1]);
    const double w = x1 - x0 < 1.0 ? 1.0 : x1 - x0, t = y1 - y0 < 1.0 ? 1.0 : y1 - y0;
    if (!(w <= (double)kMaxImageSize) || !(t <= (double)kMaxImageSize)) return refuse(kTransform, "the result is outside [1, 16384]");
    if (!(std::fabs(x0) <= 1073741824.0) || !(std::fabs(y0) <= 1073741824.0)) return refuse(kTransform, "the origin is beyond 2^30");
    const double A[9] = {e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d};
    const double det = (a * A[0] + b * A[3]) + c * A[6];
    if (det == 0.0) return refuse(kTransform, "forward is singular");
    crh_transform fitted = {};
    for (int k = 0; k < 9; ++k) {
        fitted.matrix[k] = A[k] / det;
        if (!std::isfinite(fitted.matrix[k])) return refuse(kTransform, "forward is singular");
    }
    for (int row = 0; row < 3; ++row) fitted.matrix[3 * row + 2] = (fitted.matrix[3 * row] * x0 + fitted.matrix[3 * row + 1] * y0) + fitted.matrix[3 * row + 2];
    fitted.width = (uint32_t)w, fitted.height = (uint32_t)t, fitted.filter = filter, fitted.edge = edge;
    TransformConstants checked;
    st = transform_constants(&fitted, &checked);
    if (st != CRH_OK) return st;
    *out = fitted;
    origin[0] = (int32_t)-x0, origin[1] = (int32_t)-y0;
    return CRH_OK;
}
crh_status crh_transform_texels(uint32_t width, uint32_t height, const void* rgba8, const crh_transform* how, void* out_rgba8) {
    if (!rgba8 || !out_rgba8) return refuse(kTransform, "a null argument");
    TransformConstants f;
    crh_status st = transform_constants(how, &f);
    if (st == CRH_OK) st = check_size(kTransform, width, height);
    if (st != CRH_OK) return st;
    if (out_rgba8 == rgba8) return refuse(kTransform, "out_rgba8 is rgba8");
    if (f.projective) transform_run_filter<true>(static_cast<const uint8_t*>(rgba8), width, height, f, how->width, how->height, static_cast<uint8_t*>(out_rgba8));
    else transform_run_filter<false>(static_cast<const uint8_t*>(rgba8), width, height, f, how->width, how->height, static_cast<uint8_t*>(out_rgba8));
    return CRH_OK;
}
crh_status crh_image_transform(const crh_image* src, const crh_transform* how, crh_image** out) {
    if (!src || !out) return refuse(kTransform, "a null argument");
    TransformConstants f;
    crh_status st = transform_constants(how, &f); // (the fields before the image: a refused `how` does not look at it)
    if (st == CRH_OK && !src->renderer) st = refuse(kTransform, "a null argument");
    if (st == CRH_OK) st = check_size(kTransform, src->width, src->height);
    if (st != CRH_OK) return st;
    return filter_call("crh_image_transform", src->renderer, how->width, how->height, out, [&](FilterJob& job) {
        job.launch("k_image_transform", [&] { launch_image_transform(texels_of(src), src->width, src->height, f, job.texels(), how->width, how->height, job.stream); });
    });
}
