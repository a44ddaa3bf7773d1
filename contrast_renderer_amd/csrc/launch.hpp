// csrc/launch.hpp — the interface to the kernels: what api.hip and image.hip call in tessellate.hip, raster.hip, image_filter.hip, bin_edges.hip and raster_edges.hip, and
// what those call in each other (api_internal.hpp is the interface between the host files). Included by the callers AND by every file that defines one of these, so that the compiler checks each
// definition against its declaration.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "raster_params.hpp"
#include "scene.hpp"

namespace crh {

typedef void (*MarkFn)(void*, const char*, uint64_t); // a timing mark: (ctx, name, bytes moved)

// tessellate.hip
void launch_tessellate(const SceneDev& s, hipStream_t stream, MarkFn mark, void* ctx, const uint64_t bytes[4], bool has_stroke, bool need_totals);
void launch_emit(const SceneDev& s, hipStream_t stream, MarkFn mark, void* ctx, const uint64_t bytes[4], bool has_stroke, bool big_shapes, const uint32_t* hull_queued);
void launch_build_elements(const UploadBuild& u, hipStream_t stream);
void launch_fmath(int fn, const float* a, const float* b, float* out, uint64_t n, hipStream_t stream);

// raster.hip: the general path (triangle strips as the reference draws them), the scans, the multi-GPU composite
void launch_prim_ranges(const SceneDev& s, uint32_t* shape_ncand, uint32_t* shape_prim_begin, uint32_t* scratch, hipStream_t stream);
void launch_item_ranges(const SceneDev& s, const RasterParams& r, uint32_t* item_ncand, uint32_t* item_prim_begin, uint32_t* scratch, hipStream_t stream);
void launch_bin(const SceneDev& s, const RasterParams& r, uint32_t samples, hipStream_t stream, MarkFn mark, void* ctx, hipEvent_t after_setup);
void launch_fill(const SceneDev& s, const RasterParams& r, uint32_t samples, hipStream_t stream, MarkFn mark, void* ctx, hipEvent_t after_fill);
uint32_t launch_raster(const SceneDev& s, const RasterParams& r, uint32_t samples, hipStream_t stream, MarkFn mark, void* ctx, uint64_t raster_bytes, bool has_stroke,
                       const BlendForm* blend, const PaintArgs* paint = nullptr, const ImageArgs* images = nullptr, bool mips = false); // -> RasterVariant; blend: nullptr = premultiplied "over", otherwise k_raster_blend; paint (with blend): k_raster_paint; images (with paint): k_raster_image; mips (with images): k_raster_mip
void launch_paint_items(const RasterParams& r, const PaintTable& t, hipStream_t stream); // behind launch_bin: the PaintItem records and the tags of a painted pass
void launch_paint_items_images(const RasterParams& r, const PaintTable& t, uint32_t n_gradients, hipStream_t stream); // behind launch_paint_items in an image-painted pass: which records name an image paint
void launch_image_downsample(const uint32_t* src, uint32_t src_w, uint32_t src_h, uint32_t* dst, uint32_t dst_w, uint32_t dst_h, hipStream_t stream); // one level of a mip chain from the level above
void launch_scan_u32(const uint32_t* in, uint32_t* out, uint32_t* block_sum, uint32_t n, hipStream_t stream); // exclusive scan; out[n] = the total
void launch_scan_u32_pair(const uint32_t* in0, uint32_t* out0, uint32_t* block_sum0, const uint32_t* in1, uint32_t* out1, uint32_t* block_sum1, uint32_t n, hipStream_t stream);
void launch_scan_tiles(const RasterParams& r, hipStream_t stream); // exclusive scan of tile_count -> tile_offset, pair total, longest list
void launch_state_colors_from_image(const RasterParams& r, uint32_t samples, hipStream_t stream);
void launch_selftest_srgb(const float* x, uint8_t* codes, uint64_t n, float* decoded, hipStream_t stream);
void launch_composite(const uint8_t* const* layers_dev, uint32_t n_layers, uint64_t n_pixels, uint8_t* dst, hipStream_t stream);

// image_filter.hip (its header comment is the map of the kernels; edge.hpp holds the edge rule every `edge` below follows, image_geometry.hpp
// the geometries the kernels share): crh_image_blur's two passes (the kernels' comments state the two tap tables). `tmp` = four 16-bit values per texel, src_h rows
// of out_w; origin = the axis's radius for CRH_BLUR_EDGE_TRANSPARENT (the result grows), else 0; radius = 0 for an axis whose q[0] is 65536.
constexpr uint32_t kBlurMaxRadius = 192; // CRH_MAX_BLUR_RADIUS
constexpr uint32_t kBlurTapPad = 8;      // zero taps on either side of k_image_blur_v's table: the output rows a lane accumulates
void launch_image_blur_h(const uint32_t* src, uint32_t src_w, uint32_t src_h, void* tmp, uint32_t out_w, const uint32_t* taps, uint32_t radius, uint32_t origin, uint32_t edge, hipStream_t stream);
void launch_image_blur_v(const void* tmp, uint32_t tmp_h, uint32_t* out, uint32_t out_w, uint32_t out_h, const uint32_t* pairs, uint32_t radius, uint32_t origin, uint32_t edge, hipStream_t stream); // pairs == nullptr: the identity
// image_filter.hip: crh_image_composite's kernel. The result (w x h, as the backdrop) pairs its texel (i, j) with source texel (i - x, j - y), (0, 0, 0, 0)
// outside the source; o = the opacity's code, mode < 9, op < 13 (composite.hpp holds the rule and the operator's table). x, y: any int32.
void launch_image_composite(const uint32_t* backdrop, uint32_t w, uint32_t h, const uint32_t* source, uint32_t source_w, uint32_t source_h, int32_t x, int32_t y, uint32_t o, uint32_t mode,
                            uint32_t op, uint32_t* out, hipStream_t stream);
// image_filter.hip: crh_image_color_filter's kernel. src and out: w x h texels; f from color_filter_quantize; tables: the 1024 table bytes on the
// device (256 words), or nullptr for none (color_filter.hpp holds the rule).
struct ColorFilterCoefficients;
void launch_image_color_filter(const uint32_t* src, uint32_t w, uint32_t h, const ColorFilterCoefficients& f, const uint32_t* tables, uint32_t* out, hipStream_t stream);
// image_filter.hip: crh_image_morphology's two passes (morphology.hpp holds the rule, min and max; op < 2, 1 <= radius <= 192, edge < 4). h: src_h rows of src_w
// texels -> src_h rows of out_w; v: in_h rows of out_w texels -> out_h rows of out_w. origin = the axis's radius where the result grows, else 0.
void launch_image_morph_h(const uint32_t* src, uint32_t src_w, uint32_t src_h, uint32_t* out, uint32_t out_w, uint32_t op, uint32_t radius, uint32_t origin, uint32_t edge, hipStream_t stream);
void launch_image_morph_v(const uint32_t* in, uint32_t in_h, uint32_t* out, uint32_t out_w, uint32_t out_h, uint32_t op, uint32_t radius, uint32_t origin, uint32_t edge, hipStream_t stream);
// image_filter.hip: crh_image_convolve's kernel (convolve.hpp holds the rule; 1 <= order <= 15, target < order, edge < 4). src and out: h rows of w texels.
struct ConvolveCoefficients;
void launch_image_convolve(const uint32_t* src, uint32_t w, uint32_t h, const ConvolveCoefficients& f, uint32_t order_x, uint32_t order_y, uint32_t target_x, uint32_t target_y, uint32_t edge,
                           bool preserve_alpha, uint32_t* out, hipStream_t stream);
// image_filter.hip: crh_image_lighting's kernel (lighting.hpp holds the rule; op < 2, light < 3, edge < 4). src and out: h rows of w texels.
struct LightingConstants;
void launch_image_lighting(const uint32_t* src, uint32_t w, uint32_t h, const LightingConstants& f, uint32_t op, uint32_t light, uint32_t edge, uint32_t* out, hipStream_t stream);
// image_filter.hip: crh_image_turbulence's kernel (turbulence.hpp holds the rule; kind < 2). tables: the seeded tables on the device; out: h rows of w texels.
struct TurbulenceTables;
struct TurbulenceConstants;
void launch_image_turbulence(const TurbulenceTables* tables, uint32_t w, uint32_t h, const TurbulenceConstants& f, uint32_t kind, bool opaque, uint32_t* out, hipStream_t stream);
// image_filter.hip: crh_image_displace's kernel (displace.hpp holds the rule; f.filter < 2, f.edge < 4, f.channel < 4). src, map and out: h rows of w texels; out is neither input.
struct DisplaceConstants;
void launch_image_displace(const uint32_t* src, const uint32_t* map, uint32_t w, uint32_t h, const DisplaceConstants& f, uint32_t* out, hipStream_t stream);
// image_filter.hip: crh_image_distance_field's kernels (distance.hpp holds the rule; f.mode < 2, f.shift = 0, 8, 16 or 24, 1 <= f.spread <= 255, f.edge < 4). `g`: out_h rows of out_w bytes, the
// column distances between the two passes; `origin`: the source texel under result texel (0, 0) is (-origin, -origin); `thresholds`: the 256 words of distance_thresholds(f.spread) on the device.
struct DistanceConstants;
void launch_image_distance_v(const uint32_t* src, uint32_t src_w, uint32_t src_h, uint8_t* g, uint32_t out_w, uint32_t out_h, uint32_t origin, const DistanceConstants& f, hipStream_t stream);
void launch_image_distance_h(const uint8_t* g, uint32_t out_w, uint32_t out_h, const uint32_t* thresholds, const DistanceConstants& f, uint32_t* out, hipStream_t stream);
// image_filter.hip: crh_image_resize's two passes (resize.hpp holds the rule and the layout of `table`, an axis's ResizeTable on the device, `pairs` its words of taps per output).
// h: src_h rows of src_w texels -> `tmp`, src_h rows of out_w texels of four 16-bit values; v: tmp_h rows of `tmp` -> out_h rows of out_w texels.
void launch_image_resize_h(const uint32_t* src, uint32_t src_w, uint32_t src_h, void* tmp, uint32_t out_w, const uint32_t* table, uint32_t pairs, hipStream_t stream);
void launch_image_resize_v(const void* tmp, uint32_t tmp_h, uint32_t* out, uint32_t out_w, uint32_t out_h, const uint32_t* table, uint32_t pairs, hipStream_t stream);
// image_filter.hip: the kernel of crh_image_crop and crh_image_create_from_frame_region (regions.hpp holds the index rule). out: h rows of w texels, 1 <= w, h <= 16384, each written
// once; its texel (i, j) is the source's (x + i, y + j), (0, 0, 0, 0) outside source_w x source_h (each <= 65535, a frame's limit); x, y: any int32. out is not the source.
void launch_image_crop(const uint32_t* source, uint32_t source_w, uint32_t source_h, int32_t x, int32_t y, uint32_t* out, uint32_t w, uint32_t h, hipStream_t stream);
// image_filter.hip: crh_image_statistics' kernels (regions.hpp holds the rule and the kStatsWords words of a result). launch_image_stats leaves one partial result per workgroup in
// `partial`, image_stats_partials(w, h) slabs of kStatsWords words; launch_image_stats_merge joins n of them into the kStatsWords words at `out`. Nothing needs clearing first.
struct StatsConstants;
uint32_t image_stats_partials(uint32_t w, uint32_t h); // <= 1024
void launch_image_stats(const uint32_t* src, uint32_t w, uint32_t h, const StatsConstants& f, uint32_t* partial, hipStream_t stream);
void launch_image_stats_merge(const uint32_t* partial, uint32_t n, uint32_t* out, hipStream_t stream);
// image_filter.hip: crh_image_variable_blur's two passes (variable_blur.hpp holds the rule and the layout of `table`, an axis's VariableBlurAxis::words on the device). src, mask and out: h rows
// of w texels; `tmp`: h rows of w texels of four 16-bit values; apron = the axis's largest radius <= 192; shift = 8 * the mask's channel; edge < 4. out is neither input.
void launch_image_variable_blur_h(const uint32_t* src, const uint32_t* mask, uint32_t w, uint32_t h, void* tmp, const uint32_t* table, uint32_t apron, uint32_t shift, uint32_t edge, hipStream_t stream);
void launch_image_variable_blur_v(const void* tmp, const uint32_t* mask, uint32_t* out, uint32_t w, uint32_t h, const uint32_t* table, uint32_t shift, uint32_t edge, hipStream_t stream);
// image_filter.hip: crh_image_transform's kernel (transform.hpp holds the rule; f.filter < 3, f.edge < 4, f.projective = !transform_is_affine(f.m)). src: src_h rows of src_w texels;
// out: h rows of w texels, each written once; 1 <= every size <= 16384. out is not the source.
struct TransformConstants;
void launch_image_transform(const uint32_t* src, uint32_t src_w, uint32_t src_h, const TransformConstants& f, uint32_t* out, uint32_t w, uint32_t h, hipStream_t stream);

// bin_edges.hip: the plain Stencil + Color pass as boundary edges + backdrop (edge_slots.hpp), binned in one traversal; the slot ranges and scans around it
void launch_clear_words(uint32_t* words, size_t n_words, hipStream_t stream); // zeroes n_words 32-bit words with single-wave workgroups (the clear in front of both passes' binning kernels)
void launch_slot_ranges(const SceneDev& s, const RasterParams& r, uint32_t n_items, uint32_t* item_nslots, uint32_t* slot_begin, uint32_t* scratch, hipStream_t stream);
uint32_t launch_bin_edges(const SceneDev& s, const RasterParams& r, uint32_t samples, hipStream_t stream, MarkFn mark, void* ctx, hipEvent_t after_bin); // -> BinRoute | kBinReplayed | items per workgroup << 16
void launch_scatter(const RasterParams& r, hipStream_t stream, MarkFn mark, void* ctx);
void launch_shape_bounds(const SceneDev& s, float* bounds, hipStream_t stream);
void launch_slab_items(const RasterParams& r, uint8_t* elsewhere, hipStream_t stream);
void launch_plain_ranges(const SceneDev& s, uint32_t* shape_ncand, uint32_t* shape_prim_begin, uint32_t* shape_nslots, uint32_t* shape_slot_begin, uint32_t* scratch0, uint32_t* scratch1, hipStream_t stream);
bool bin_itemwise(const RasterParams& r);
void flat_batches(const uint32_t* cost, uint32_t n_items, std::vector<uint32_t>& runs);
void flat_batch_limits(uint32_t n_items, uint32_t limits[4]);
void launch_tile_bases(const uint32_t* tile_count, uint32_t* caps, uint32_t* tile_base, uint32_t* scratch, uint32_t n_tiles, uint32_t tiles_x, uint32_t radius, hipStream_t stream);

// raster_edges.hip: the per-tile raster kernels of that pass
uint32_t launch_raster_edges(const SceneDev& s, const RasterParams& r, uint32_t samples, hipStream_t stream, MarkFn mark, void* ctx, uint64_t raster_bytes, bool has_stroke); // -> RasterVariant

} // namespace crh
