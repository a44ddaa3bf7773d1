/* contrast_hip.h — C ABI of the MI355X-native tessellate + raster hot path of contrast_renderer.
 *
 * Every entry point names the reference interface it replaces (file:line relative to the
 * reference tree, contrast_renderer v0.1.4). The reference has no FFI; its seam for this path is
 * `Shape::from_paths` / `Shape::render` (renderer.rs:177, :267) over the private modules
 * fill / stroke / vertex (lib.rs:12,16,20). A Rust shim that keeps those signatures binds exactly
 * the functions below (see INTEGRATION.md for the `extern "C"` block).
 *
 * Conventions: plain pointers and sizes, host memory unless a name ends in `_dev`; all functions
 * return crh_status; handles are thread-compatible (one HIP stream per renderer), not thread-safe.
 * Batch first: the unit of work is a *scene* = many Shapes built and rendered together, because one
 * kernel launch per Shape would be launch-bound on a 256-CU part. A scene with n_shapes == 1 is the
 * reference's single `Shape`.
 */
#ifndef CONTRAST_HIP_H
#define CONTRAST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: 1..5 are error.rs:5-16 in declaration order ---------------------------------- */
typedef enum crh_status {
    CRH_OK = 0,
    CRH_ERR_NUMBER_OF_STENCIL_BITS_IS_UNSUPPORTED = 1,    /* renderer.rs:433-435 */
    CRH_ERR_CLIP_STACK_OVERFLOW = 2,                      /* renderer.rs:933-935 */
    CRH_ERR_TOO_MANY_NESTED_OPACITY_GROUPS = 3,           /* renderer.rs:947-949, :980-982 */
    CRH_ERR_TOO_MANY_DASH_INTERVALS = 4,                  /* renderer.rs:32-34 */
    CRH_ERR_DYNAMIC_STROKE_OPTIONS_INDEX_OUT_OF_BOUNDS = 5, /* renderer.rs:189-191, :366-368 */
    CRH_ERR_NON_FINITE = 6,        /* the reference panics: safe_float.rs:46,114 */
    CRH_ERR_DEGENERATE_CUBIC = 7,  /* the reference panics: fill.rs:174,178 */
    CRH_ERR_UNSUPPORTED = 8,       /* documented limit of this implementation */
    CRH_ERR_HIP = 9,               /* a HIP runtime call failed; crh_last_error() has the text */
    CRH_ERR_INVALID_ARGUMENT = 10
} crh_status;

/* ---- the Path data model (path.rs:15-230) -------------------------------------------------------- */

/* SegmentType discriminants, path.rs:56-67 */
enum {
    CRH_SEGMENT_LINE = 0,               /* control data: x y                          (path.rs:15-18)  */
    CRH_SEGMENT_INTEGRAL_QUADRATIC = 1, /* control data: c0x c0y c1x c1y              (path.rs:22-25)  */
    CRH_SEGMENT_INTEGRAL_CUBIC = 2,     /* control data: c0x c0y c1x c1y c2x c2y      (path.rs:29-32)  */
    CRH_SEGMENT_RATIONAL_QUADRATIC = 3, /* control data: weight c0x c0y c1x c1y       (path.rs:36-43)  */
    CRH_SEGMENT_RATIONAL_CUBIC = 4      /* control data: w0 w1 w2 w3 c0x c0y .. c2y   (path.rs:47-52)  */
};
/* Join, path.rs:71-82 ; Cap, path.rs:86-101 */
enum { CRH_JOIN_MITER = 0, CRH_JOIN_BEVEL = 1, CRH_JOIN_ROUND = 2 };
enum { CRH_CAP_SQUARE = 0, CRH_CAP_ROUND = 1, CRH_CAP_OUT = 2, CRH_CAP_IN = 3, CRH_CAP_RIGHT = 4, CRH_CAP_LEFT = 5, CRH_CAP_BUTT = 6 };
/* CurveApproximation, path.rs:153-167 */
enum { CRH_CURVE_UNIFORMLY_SPACED_PARAMETERS = 0, CRH_CURVE_UNIFORM_TANGENT_ANGLE = 1 };
#define CRH_MAX_DASH_INTERVALS 4 /* path.rs:121 */

/* StrokeOptions, path.rs:171-192 (already legalize()d by the caller, path.rs:196-200) */
typedef struct crh_stroke_options {
    float width;
    float offset;
    float miter_clip;
    uint32_t closed;
    uint32_t dynamic_stroke_options_group;
    uint32_t curve_approximation; /* CRH_CURVE_* */
    uint32_t steps;               /* UniformlySpacedParameters(steps) */
    float angle_step;             /* UniformTangentAngle(angle_step) */
} crh_stroke_options;

/* DashInterval, path.rs:105-118 */
typedef struct crh_dash_interval {
    float gap_start;
    float gap_end;
    uint32_t dash_start; /* CRH_CAP_* */
    uint32_t dash_end;   /* CRH_CAP_* */
} crh_dash_interval;

/* DynamicStrokeOptions, path.rs:127-149 */
typedef struct crh_dynamic_stroke_options {
    uint32_t dashed;      /* 1 = Dashed{join, pattern, phase}, 0 = Solid{join, start, end} */
    uint32_t join;        /* CRH_JOIN_* */
    uint32_t pattern_len; /* > CRH_MAX_DASH_INTERVALS -> CRH_ERR_TOO_MANY_DASH_INTERVALS; 0 is invalid as in the reference */
    crh_dash_interval pattern[CRH_MAX_DASH_INTERVALS];
    float phase;
    uint32_t start; /* CRH_CAP_* (Solid) */
    uint32_t end;   /* CRH_CAP_* (Solid) */
} crh_dynamic_stroke_options;

/* DynamicStrokeDescriptor, renderer.rs:20-27: the 48-byte record the raster reads */
typedef struct crh_dynamic_stroke_descriptor {
    float gap_start[CRH_MAX_DASH_INTERVALS];
    float gap_end[CRH_MAX_DASH_INTERVALS];
    uint32_t caps;
    uint32_t count_dashed_join;
    float phase;
    uint32_t _padding;
} crh_dynamic_stroke_descriptor;

/* A batch of Shapes, each a contiguous run of Paths (the argument `paths: &[Path]` of
 * renderer.rs:181, for many shapes at once). Struct-of-arrays flattening of path.rs:213-230:
 * `control_data` holds the segments' floats in path order, one record per segment with the layout
 * given at CRH_SEGMENT_* above; `path_start` is Path::start. All floats must be finite; -0.0 is
 * canonicalised to +0.0 on upload (SafeFloat::from, safe_float.rs:44-52). */
typedef struct crh_path_batch {
    uint32_t n_shapes;
    const uint32_t* shape_path_begin; /* [n_shapes + 1] */
    uint32_t n_paths;
    const uint32_t* path_segment_begin;  /* [n_paths + 1] into segment_types */
    const float* path_start;             /* [n_paths][2] */
    const int32_t* path_stroke_options;  /* [n_paths]: index into stroke_options, or -1 = filled (Path::stroke_options == None) */
    uint32_t n_segments;
    const uint8_t* segment_types; /* [n_segments] CRH_SEGMENT_* */
    const float* control_data;    /* sum over segments of {2,4,6,5,10}[type] floats */
    uint32_t n_control_floats;
    uint32_t n_stroke_options;
    const crh_stroke_options* stroke_options;
    const uint32_t* shape_dynamic_begin; /* [n_shapes + 1] into dynamic_stroke_options (the per-shape `&[DynamicStrokeOptions]`, renderer.rs:180) */
    uint32_t n_dynamic_stroke_options;
    const crh_dynamic_stroke_options* dynamic_stroke_options;
} crh_path_batch;

/* ---- Renderer (renderer.rs:380-435) --------------------------------------------------------------- */

/* Configuration, renderer.rs:380-405. The fields that change results on this path:
 * `blending` (the colour cover's wgpu::ColorTargetState, renderer.rs:380-382, :736-754) is not a member of crh_config: it is given to
 * crh_renderer_create_blended below (crh_renderer_create = premultiplied "over", One / OneMinusSrcAlpha, examples/showcase/main.rs:32-43);
 * the depth attachment is f32 per sample (depth_stencil_format is a wgpu detail), color_attachment_in_stencil_pass has no meaning in a
 * compute rasterizer.
 * The three depth / cull fields act on the colour cover only, as in the reference (renderer.rs:743-745: every other pipeline is
 * built with cull None, CompareFunction::Always and no depth write). Zero-initialised = no culling, Always, no write. */
typedef enum crh_cull { CRH_CULL_NONE = 0, CRH_CULL_FRONT = 1, CRH_CULL_BACK = 2 } crh_cull; /* Option<wgpu::Face>; front = counter-clockwise on screen (renderer.rs:477) */
typedef enum crh_compare { /* wgpu::CompareFunction of `fragment depth  OP  stored depth` */
    CRH_COMPARE_ALWAYS = 0,
    CRH_COMPARE_NEVER = 1,
    CRH_COMPARE_LESS = 2,
    CRH_COMPARE_EQUAL = 3,
    CRH_COMPARE_LESS_EQUAL = 4,
    CRH_COMPARE_GREATER = 5,
    CRH_COMPARE_NOT_EQUAL = 6,
    CRH_COMPARE_GREATER_EQUAL = 7
} crh_compare;
/* msaa_sample_count: 1, 2, 4 or 8 (wgpu::MultisampleState::count, renderer.rs:490-494); anything else is CRH_ERR_UNSUPPORTED. The sample
 * locations are the standard ones (Vulkan standardSampleLocations = D3D), in 1/16 pixel, x right and y down, in sample-index order — the order
 * of the per-sample data, e.g. crh_frame_download_depth's [height][width][msaa]:
 *   1: (8, 8)
 *   2: (12, 12), (4, 4)
 *   4: (6, 2), (14, 6), (2, 10), (10, 14)
 *   8: (9, 5), (7, 11), (13, 9), (5, 3), (3, 13), (1, 7), (11, 15), (15, 1)
 * The resolve is the box average of a pixel's samples, summed in sample-index order. */
typedef struct crh_config {
    uint32_t msaa_sample_count;         /* 1, 2, 4 or 8 (the table above) */
    uint32_t clip_nesting_counter_bits; /* validated as in renderer.rs:433 */
    uint32_t winding_counter_bits;      /* >= 1, sum <= 8 */
    uint32_t alpha_layer_count;         /* <= 4; layers of the alpha-context operations (renderer.rs:403-404) */
    uint32_t cull_mode;                 /* crh_cull, renderer.rs:383-384 */
    uint32_t depth_compare;             /* crh_compare, renderer.rs:387-388 */
    uint32_t depth_write_enabled;       /* 0 / 1, renderer.rs:389-390 */
} crh_config;

typedef struct crh_renderer crh_renderer; /* Renderer, renderer.rs:408 */
typedef struct crh_scene crh_scene;       /* n Shapes (renderer.rs:163-171) built together */
typedef struct crh_frame crh_frame;       /* the caller-owned colour + stencil attachments of the render pass */

/* RenderOperation, renderer.rs:145-160, same order */
typedef enum crh_render_op {
    CRH_OP_STENCIL = 0,
    CRH_OP_CLIP = 1,
    CRH_OP_UNCLIP = 2,
    CRH_OP_COLOR = 3,
    CRH_OP_SAVE_ALPHA_CONTEXT = 4,
    CRH_OP_SCALE_ALPHA_CONTEXT = 5,
    CRH_OP_RESTORE_ALPHA_CONTEXT = 6
} crh_render_op;

/* Renderer::new, renderer.rs:432-435. device_ordinal = HIP device (cuda:N). */
crh_status crh_renderer_create(const crh_config* config, int device_ordinal, crh_renderer** out);
void crh_renderer_destroy(crh_renderer* renderer);
/* Renderer::get_config, renderer.rs:887 */
crh_status crh_renderer_get_config(const crh_renderer* renderer, crh_config* out);

/* Configuration::blending, renderer.rs:380-382: the blend state of the Color operation's pipeline (color_cover, renderer.rs:736-754).
 * Stencil, Clip / UnClip and the alpha-context covers keep their fixed states (renderer.rs:761-861), as in the reference.
 * crh_blend_factor has the order of wgpu::BlendFactor, crh_blend_operation that of wgpu::BlendOperation. */
typedef enum crh_blend_factor {
    CRH_BLEND_ZERO = 0,
    CRH_BLEND_ONE = 1,
    CRH_BLEND_SRC = 2,
    CRH_BLEND_ONE_MINUS_SRC = 3,
    CRH_BLEND_SRC_ALPHA = 4,
    CRH_BLEND_ONE_MINUS_SRC_ALPHA = 5,
    CRH_BLEND_DST = 6,
    CRH_BLEND_ONE_MINUS_DST = 7,
    CRH_BLEND_DST_ALPHA = 8,
    CRH_BLEND_ONE_MINUS_DST_ALPHA = 9,
    CRH_BLEND_SRC_ALPHA_SATURATED = 10, /* min(As, 1 - Ad) for rgb, 1 for alpha */
    CRH_BLEND_CONSTANT = 11,
    CRH_BLEND_ONE_MINUS_CONSTANT = 12,
    CRH_BLEND_SRC1 = 13, /* 13-16: the dual-source factors; the colour cover has one output: CRH_ERR_UNSUPPORTED */
    CRH_BLEND_ONE_MINUS_SRC1 = 14,
    CRH_BLEND_SRC1_ALPHA = 15,
    CRH_BLEND_ONE_MINUS_SRC1_ALPHA = 16
} crh_blend_factor;
typedef enum crh_blend_operation {
    CRH_BLEND_OP_ADD = 0,
    CRH_BLEND_OP_SUBTRACT = 1,          /* src * src_factor - dst * dst_factor */
    CRH_BLEND_OP_REVERSE_SUBTRACT = 2,  /* dst * dst_factor - src * src_factor */
    CRH_BLEND_OP_MIN = 3,               /* min(src, dst): both factors must be One (WebGPU validation) */
    CRH_BLEND_OP_MAX = 4
} crh_blend_operation;
typedef struct crh_blend_component { /* wgpu::BlendComponent */
    uint32_t src_factor; /* crh_blend_factor */
    uint32_t dst_factor; /* crh_blend_factor */
    uint32_t operation;  /* crh_blend_operation */
} crh_blend_component;
enum { CRH_COLOR_WRITE_RED = 1, CRH_COLOR_WRITE_GREEN = 2, CRH_COLOR_WRITE_BLUE = 4, CRH_COLOR_WRITE_ALPHA = 8, CRH_COLOR_WRITE_ALL = 15 }; /* wgpu::ColorWrites */
typedef struct crh_color_target_state { /* wgpu::ColorTargetState without the format (the frame's: crh_frame_create_format) */
    uint32_t blend_enabled;    /* 0 = `blend: None`: the source replaces the target */
    crh_blend_component color; /* rgb channels */
    crh_blend_component alpha; /* alpha channel */
    uint32_t write_mask;       /* CRH_COLOR_WRITE_*: channels outside the mask keep the target's value */
    float constant[4];         /* RenderPass::set_blend_constant — kept with the renderer here (a deviation: wgpu sets it per pass) */
} crh_color_target_state;
/* Renderer::new with Configuration::blending. `blending` NULL = the showcase's premultiplied "over" (blend enabled, both components
 * One / OneMinusSrcAlpha / Add, write mask 15), exactly crh_renderer_create. Validated before any device is touched: a factor > 16, an
 * operation > 4, a write mask > 15, a non-finite constant, or Min / Max with a factor other than One -> CRH_ERR_INVALID_ARGUMENT; a
 * dual-source factor -> CRH_ERR_UNSUPPORTED.
 * Per sample of the Color operation, where today's stencil and depth tests let it blend: the source is color_cover's premultiplied
 * (rgb * a, a) (shaders.wgsl:304-309); factors follow WebGPU's table. A state other than "over" treats the target as an Rgba8Unorm
 * attachment on every frame format: source and constant are clamped to [0, 1] (NaN -> 0) before the blend, the result after it, and a
 * CRH_FORMAT_RGBA8_ATTACHMENT frame rounds every written value to 8 bits. Products and the operation round separately (no fused
 * multiply-add). Such passes are drawn by the general (triangle) formulation, and crh_frame_exchange refuses their layers
 * (CRH_ERR_UNSUPPORTED on every rank: its composite is "over"); crh_frame_gather_slabs works with any state. */
crh_status crh_renderer_create_blended(const crh_config* config, const crh_color_target_state* blending, int device_ordinal, crh_renderer** out);
/* the state the renderer was created with (the "over" state for crh_renderer_create) */
crh_status crh_renderer_get_blending(const crh_renderer* renderer, crh_color_target_state* out);

/* convert_dynamic_stroke_options, renderer.rs:29-60 (host-side, pure) */
crh_status crh_convert_dynamic_stroke_options(const crh_dynamic_stroke_options* options, crh_dynamic_stroke_descriptor* out);

/* ---- Shape::from_paths (renderer.rs:177-249) ------------------------------------------------------ */

/* Host -> HBM: validates (finite, stroke-group bounds renderer.rs:188-191, dash count renderer.rs:32-34),
 * canonicalises -0, lays the batch out for the kernels and copies it to the device. This is the part of
 * from_paths that is not arithmetic; it is outside bench.py's timed region. `existing` may be NULL; when
 * given, its device allocations are reused if large enough (Buffer::update, renderer.rs:89-95). Paths of the
 * STRUCTURE `existing` holds (as many Shapes, paths and segments, stroked or not — an animation of control
 * points) also keep the capacities of its vertex streams: the next crh_scene_tessellate does not wait for
 * the totals of the new paths; a tessellation that does not fit after all is noticed when a frame drawn from
 * it is settled (crh_frame_synchronize, crh_frame_download, ...) or by crh_scene_status, sized and repeated,
 * the frame drawn again. The host arrays of `batch` are copied before the call returns. `existing` keeps its paint table and
 * association (crh_scene_set_paints, crh_scene_set_paints_with_images) whatever the new Shape count: instance i of the new Shapes has the
 * paint instance_paint[i] where the association reaches and its solid colour beyond it; its instances are to be set again. */
crh_status crh_scene_upload(crh_renderer* renderer, const crh_path_batch* batch, crh_scene* existing, crh_scene** out);
/* The arithmetic of from_paths for every shape of the scene, on the GPU:
 * StrokeBuilder::add_path (stroke.rs:205-465), FillBuilder::add_path (fill.rs:263-367),
 * convex_hull::andrew + triangle_fan_to_strip (convex_hull.rs:7-40, vertex.rs:28-35) and the
 * concat_buffers! offsets (renderer.rs:198-209). Asynchronous on the renderer's stream. */
crh_status crh_scene_tessellate(crh_scene* scene);
/* Waits for the stream and returns the first per-path error raised by the kernels (codes 6, 7, 8). */
crh_status crh_scene_status(crh_scene* scene);
void crh_scene_destroy(crh_scene* scene);

/* The reference's single-shape entry point: upload + tessellate of a batch with n_shapes == 1. */
crh_status crh_shape_from_paths(crh_renderer* renderer, const crh_path_batch* one_shape, crh_scene* existing, crh_scene** out);

/* Parity tap: exactly the byte image renderer.rs:198-209 uploads for shape `shape_index`.
 * vertex_offsets[8] / index_offsets[3] are the cumulative byte END offsets of
 * [line, joint, solid, integral_quadratic, integral_cubic, rational_quadratic, rational_cubic, hull]
 * and [line_indices, joint_indices, solid_indices]. Call with NULL byte pointers to query sizes. */
crh_status crh_scene_shape_layout(crh_scene* scene, uint32_t shape_index, uint64_t vertex_offsets[8], uint64_t index_offsets[3]);
crh_status crh_scene_shape_download(crh_scene* scene, uint32_t shape_index, void* vertex_bytes, void* index_bytes);
/* All shapes at once: layout[shape][11] u64 (8 vertex + 3 index END offsets); sizes in bytes of the
 * concatenation over shapes are returned so the caller can allocate, then download. */
crh_status crh_scene_layout_all(crh_scene* scene, uint64_t* layout /* [n_shapes][11] */, uint64_t* total_vertex_bytes, uint64_t* total_index_bytes);
crh_status crh_scene_download_all(crh_scene* scene, void* vertex_bytes, void* index_bytes);
/* Bytes the tessellation kernels read and wrote (the algorithmic traffic of SURVEY.md §8(d)). */
crh_status crh_scene_traffic(crh_scene* scene, uint64_t* bytes_read, uint64_t* bytes_written);

/* Shape::set_dynamic_stroke_options, renderer.rs:360-376 */
crh_status crh_scene_set_dynamic_stroke_options(crh_scene* scene, uint32_t shape_index, uint32_t group_index, const crh_dynamic_stroke_options* options);

/* ---- render pass (renderer.rs:267-355 + shaders.wgsl) --------------------------------------------- */

/* The colour target (RGBA8 unorm, premultiplied) plus the per-sample winding ("stencil") state. */
crh_status crh_frame_create(crh_renderer* renderer, uint32_t width, uint32_t height, crh_frame** out);
/* The same with the storage format of the resolved image named. CRH_FORMAT_RGBA8 is the reference's target (main.rs:205-215 renders to
 * the surface format, 8 bits per channel). CRH_FORMAT_RGBA16F keeps four binary16 values per pixel — the per-rank LAYERS of the multi-GPU
 * exchange (layers exchanged as RGBA16F keep the composite within 1/255 of a single-GPU render, RGBA8 layers within 2/255). */
enum {
    CRH_FORMAT_RGBA8 = 0,
    CRH_FORMAT_RGBA16F = 1,
    CRH_FORMAT_RGBA8_ATTACHMENT = 2,
    CRH_FORMAT_BGRA8 = 3,                     /* wgpu Bgra8Unorm, f32 colours within a pass (as CRH_FORMAT_RGBA8) */
    CRH_FORMAT_BGRA8_ATTACHMENT = 4,          /* wgpu Bgra8Unorm, every write rounded (as CRH_FORMAT_RGBA8_ATTACHMENT) */
    CRH_FORMAT_RGBA8_SRGB = 5,                /* wgpu Rgba8UnormSrgb, f32 linear colours within a pass, encoded once at the end */
    CRH_FORMAT_RGBA8_SRGB_ATTACHMENT = 6,     /* wgpu Rgba8UnormSrgb, every write encoded to sRGB8 and read back decoded */
    CRH_FORMAT_BGRA8_SRGB = 7,                /* wgpu Bgra8UnormSrgb, as CRH_FORMAT_RGBA8_SRGB */
    CRH_FORMAT_BGRA8_SRGB_ATTACHMENT = 8      /* wgpu Bgra8UnormSrgb, as CRH_FORMAT_RGBA8_SRGB_ATTACHMENT */
};
/* CRH_FORMAT_RGBA8_ATTACHMENT: RGBA8 storage like CRH_FORMAT_RGBA8, and the frame behaves like the wgpu::TextureFormat::Rgba8Unorm colour
 * ATTACHMENT the reference blends into (renderer.rs:736-754, examples/showcase/main.rs:32-43,205-215): every colour write of a cover — the
 * premultiplied "over" of Color, the alpha writes of Scale / RestoreAlphaContext — is rounded to 8 bits per channel where it happens, as a
 * hardware blender reads and writes the texture. CRH_FORMAT_RGBA8 keeps f32 colours for the whole pass and rounds once at the end: up to a
 * few 1/255 closer to the exact composite where many translucent Shapes overlap. Same download / upload entry points as CRH_FORMAT_RGBA8.
 *
 * Formats 3-8 are the other colour targets of Configuration::blending's `format` (renderer.rs:380-382). All store 4 bytes per pixel:
 *   BGRA byte order: B G R A in memory — crh_frame_download / crh_frame_device_pointer hand out, and crh_frame_upload takes, bytes in the
 *       frame's storage order; nothing else differs from the RGBA formats (a Bgra8Unorm swapchain image is the frame's bytes as they are).
 *   sRGB (*_SRGB): as a wgpu *Srgb attachment, colours are linear within a pass — the MSAA resolve averages linear samples — and rgb is
 *       encoded at the store; loads (a pass over existing content, crh_frame_upload) decode rgb. Alpha is never converted (unorm8 as RGBA8).
 *       *_SRGB_ATTACHMENT encodes and decodes rgb at every write where CRH_FORMAT_RGBA8_ATTACHMENT rounds. A blend state other than "over"
 *       blends the decoded (linear) target. The codec is correctly rounded — hardware blenders are allowed a tolerance here, so no GPU
 *       gives a bit-exact answer to copy; this library defines its contract as: linear(s) = s / 12.92 (s <= 0.04045) or
 *       ((s + 0.055) / 1.055)^2.4 in float64 (utils.rs:203-226); decode D[c] = float32 round-to-nearest of linear(c / 255); encode of a
 *       float32 x = the number of k in 1..255 with x >= T[k], T[k] = the smallest float32 not below linear((k - 0.5) / 255), NaN -> 0.
 *   crh_frame_clear, crh_frame_set_tile_rows, crh_frame_download, crh_frame_device_pointer and crh_frame_gather_slabs move bytes and work on
 *   every 8-bit format (gathered layers and the result share one byte encoding: X and X_ATTACHMENT count as one; a mismatch is
 *   CRH_ERR_INVALID_ARGUMENT on every rank); crh_frame_download_f16 refuses them; crh_frame_exchange returns CRH_ERR_UNSUPPORTED on every
 *   rank for a BGRA or sRGB layer or result (its composite is unorm RGBA "over"). Passes take the formulation an RGBA8 frame would. */
crh_status crh_frame_create_format(crh_renderer* renderer, uint32_t width, uint32_t height, uint32_t format, crh_frame** out);
crh_status crh_frame_format(const crh_frame* frame, uint32_t* format);
void crh_frame_destroy(crh_frame* frame);
/* LoadOp::Clear(TRANSPARENT) + depth clear 1.0 + stencil clear 0 (examples/showcase/main.rs:217-230) */
crh_status crh_frame_clear(crh_frame* frame);
/* The stencil attachment and the alpha layers of the reference are caller-owned textures: what one Shape::render call leaves in them
 * — an open Clip, the winding of a Stencil without its cover, a saved alpha context — is seen by the next call, whatever Shape (object) it
 * belongs to (renderer.rs:148-158, 257-266, 932-985). A frame keeps that state across crh_scene_render* calls, in HBM: the stencil byte
 * (clip nesting counter << winding bits | winding counter, renderer.rs:565-566, 936), the saved alphas and the f32 colour of every sample.
 * It starts to do so by itself at the first recorded pass that ENDS with state left over; this call starts it now — a pass that will
 * span several Shape / Scene objects calls it in front of its first crh_scene_render_draws, so that colours drawn before the state
 * appears are kept per sample and unrounded too (CRH_FORMAT_RGBA8 rounds once, at the resolve — as within one crh_scene_render_draws).
 * In force until crh_frame_clear. Passes into such a frame are drawn by the general (triangle) formulation. */
crh_status crh_frame_keep_pass_state(crh_frame* frame);
/* The depth attachment (f32 per sample, [height][width][msaa_sample_count]); it exists when the renderer's configuration tests or
 * writes depth. clear_depth = LoadOp::Clear(value) (main.rs:223-226); upload_depth places the depth of a 3-D scene the Shapes are
 * decals in (README.md:8-12): `depth` = [height][width] host floats, replicated to every sample; download_depth copies all samples out. */
crh_status crh_frame_clear_depth(crh_frame* frame, float value);
crh_status crh_frame_upload_depth(crh_frame* frame, const float* depth);
crh_status crh_frame_download_depth(crh_frame* frame, float* depth_samples);

/* For every shape i of the scene, in index order: Shape::render(Stencil) then Shape::render(Color)
 * with instance transform `transforms[i]` (column-major mat4, 64 B: shaders.wgsl:13-27) and colour
 * `colors[i]` (straight RGBA, 16 B: shaders.wgsl:304-309) — the loop of examples/showcase/main.rs:236-250.
 * Any 4x4 matrix is accepted: perspective instances (utils.rs:181-203, main.rs:162-202) are rasterised with homogeneous edge functions,
 * a per-sample near / far test and perspective-correct attributes.
 * Pointers are host memory; they are copied to the device when they change. Asynchronous. */
crh_status crh_scene_render(crh_scene* scene, crh_frame* frame, const float* transforms, const float* colors);
/* Same, with per-shape data already in HBM (used by bench.py so that PCIe is outside the step). */
crh_status crh_scene_set_instances(crh_scene* scene, const float* transforms, const float* colors);
crh_status crh_scene_render_resident(crh_scene* scene, crh_frame* frame);

/* A recorded render pass. One crh_draw = one call of Shape::render(renderer, pass, instance_indices, op) (renderer.rs:267-273) together
 * with the pass state it sees: the stencil reference set by Renderer::set_clip_depth (renderer.rs:932-938) and, for the alpha-context
 * operations, the layer bound by Renderer::save_alpha_context / restore_alpha_context (renderer.rs:941-985). `instance` indexes
 * `transforms` / `colors` (the instance buffers, shaders.wgsl:13-27): a Shape may be drawn any number of times.
 *   Stencil                     the seven stencil pipelines (renderer.rs:275-337)
 *   Clip / UnClip               increment / decrement_clip_nesting_counter pipelines (renderer.rs:692-729)
 *   Color                       color_cover (renderer.rs:736-754, shaders.wgsl:304-309)
 *   Save / Scale / Restore      the alpha-context covers (renderer.rs:761-861, shaders.wgsl:311-355); the saved layers live with the frame
 * Draws execute in order. Errors as the reference: clip_depth >= 2^clip_nesting_counter_bits -> CRH_ERR_CLIP_STACK_OVERFLOW,
 * alpha_layer >= alpha_layer_count -> CRH_ERR_TOO_MANY_NESTED_OPACITY_GROUPS. At most 4 alpha layers are supported. */
typedef struct crh_draw {
    uint32_t shape;       /* index of the Shape in the scene */
    uint32_t instance;    /* index into transforms / colors */
    uint32_t op;          /* crh_render_op */
    uint32_t clip_depth;  /* Renderer::set_clip_depth value in effect */
    uint32_t alpha_layer; /* alpha_layer of save_alpha_context / restore_alpha_context in effect (alpha-context operations only) */
} crh_draw;
crh_status crh_scene_render_draws(crh_scene* scene, crh_frame* frame, const float* transforms, const float* colors, uint32_t n_instances,
                                  const crh_draw* draws, uint32_t n_draws);

/* Gradient paints: the source of a Color cover, per sample, in place of the instance's one colour (what a user of the reference does with a
 * cover pipeline of their own). The model, which the tests check against float64:
 *   coordinates  a paint lives in the Shape's path coordinates: it moves, scales and tilts with the instance transform. p is the sample's
 *                position in those coordinates (Shapes lie in z = 0: the sample's place on the frame through the inverse of the
 *                3x3 homography made of columns 0, 1, 3 and rows x, y, w of the transform and the clip -> pixel map).
 *   linear       t = dot(p - p0, p1 - p0) / dot(p1 - p0, p1 - p0)
 *   radial       t = |p - p0| / radius         (p0 the centre, radius = p1[0] > 0, p1[1] = 0)
 *   conic        p0 the centre, p1[0] the start angle and p1[1] the end angle, both in radians. With a = turns(p.y - p0.y, p.x - p0.x) in
 *                [0, 1), the angle of p - p0 in the Shape's path coordinates from +x towards +y in turns (turns(0, 0) = 0; the four axes give
 *                exactly 0, 0.25, 0.5 and 0.75), and the table's sweep = p1[1] - p1[0], s = (p1[0] / 2 pi) - floor(p1[0] / 2 pi), k = 2 pi / |sweep|:
 *                b = a - s for sweep > 0, b = s - a for sweep < 0 (the same stops read clockwise); if b < 0 then b = b + 1; t = b k.
 *                (In f32 the sum may round to exactly 1 on the start ray: inside the stated error, and on the seam.) With |sweep| < 2 pi, t runs
 *                past 1: PAD holds the last stop over the rest of the turn, REPEAT and REFLECT tile the wedge round the circle. The device
 *                evaluates a in f32 (csrc/paint_angle.hpp paint_turns, which states its error against the exact angle as kPaintTurnsError).
 *   spread       PAD: t = clamp(t, 0, 1); REPEAT: t = t - floor(t); REFLECT: u = t - 2 floor(t / 2), t = u <= 1 ? u : 2 - u
 *   stops        offsets non-decreasing in [0, 1]. In front of the first stop its colour, behind the last stop its colour; between stops i and
 *                i + 1 with o_i < o_i+1: c_i + f (c_i+1 - c_i), f = (t - o_i) / (o_i+1 - o_i), per straight-alpha channel — equal stop colours
 *                give that colour back exactly. Two stops with one offset make a hard edge; at t equal to it the later stop wins.
 *   non-finite   p is not finite where a projective instance divides by W = 0 or a coordinate overflows f32, and t may then be NaN (REPEAT and
 *                REFLECT of an infinite t are NaN as well). PAD's clamp takes NaN as 0; under REPEAT and REFLECT a NaN t compares below every
 *                offset and gives the first stop's colour. Hence equal stop colours give that colour back exactly for every t, NaN included.
 *   source       paint(t) * instance colour per channel (straight alpha), premultiplied as the solid colour is (rgb * a, a), then blended with
 *                the renderer's blend state as crh_renderer_create_blended describes: source clamped to [0, 1], the frame format's rounding of
 *                writes, the write mask. Under the default "over" state a painted pass evaluates "over" in that same form: a painted cover is
 *                always the Rgba8Unorm-attachment model (clamped source and result), never the unclamped float arithmetic of the solid fast path.
 * `instance_paint[i]` is the index into `paints` of instance i's paint, or -1 for its solid colour; instances at index n_instances and beyond are
 * solid. The table is copied and stays with the Scene until the next call; n_paints == 0 clears it. It applies to crh_scene_render,
 * _render_resident (instance i = Shape i) and _render_draws, and to the Color operation only — the other six ignore it. A pass that draws a
 * painted instance runs the general triangle kernel (as a blend state other than "over" does); every other pass is launched as before.
 * Errors: a non-finite field CRH_ERR_NON_FINITE; an unknown kind or spread, n_stops 0 or > CRH_MAX_GRADIENT_STOPS, decreasing offsets or one outside
 * [0, 1], a linear paint with p0 == p1 (precisely: whose dot(p1 - p0, p1 - p0), evaluated in f32, is not a positive finite number — it may
 * underflow or overflow for p0 != p1), a radial one with radius <= 0, a conic one with sweep == 0 or
 * |sweep| greater than the f32 nearest to 2 pi (or so small that k overflows f32), an instance_paint entry >= n_paints or < -1: CRH_ERR_INVALID_ARGUMENT with a
 * crh_last_error text. A failed call leaves the Scene's previous table in place.
 * The table's p1 - p0 and dot(p1 - p0, p1 - p0) are evaluated once, in f32, when the call builds the table; a conic paint's sweep, s and k each
 * once in binary64 from the f32 fields, rounded once to f32. The call settles the frames drawn
 * from the Scene and waits for the renderer's work in flight (kernels read the table): set a table when it changes, not once per frame. */
#define CRH_MAX_GRADIENT_STOPS 8
/* (3 is not a kind and stays refused: an image paint is a type of its own, crh_image_paint below, not a crh_paint of a third kind) */
typedef enum crh_paint_kind { CRH_PAINT_LINEAR = 1, CRH_PAINT_RADIAL = 2, CRH_PAINT_CONIC = 4 } crh_paint_kind;
typedef enum crh_spread { CRH_SPREAD_PAD = 0, CRH_SPREAD_REPEAT = 1, CRH_SPREAD_REFLECT = 2 } crh_spread;
typedef struct crh_gradient_stop {
    float offset;
    float color[4]; /* straight RGBA */
} crh_gradient_stop;
typedef struct crh_paint {
    uint32_t kind, spread; /* crh_paint_kind, crh_spread */
    float p0[2], p1[2];    /* linear: t = 0 at p0, t = 1 at p1; radial: centre p0, radius p1[0] (> 0), p1[1] = 0; conic: centre p0, start angle p1[0], end angle p1[1] */
    uint32_t n_stops;      /* 1..CRH_MAX_GRADIENT_STOPS */
    crh_gradient_stop stops[CRH_MAX_GRADIENT_STOPS];
} crh_paint;
crh_status crh_paint_validate(const crh_paint* paint); /* host only: needs no renderer and no device */
crh_status crh_scene_set_paints(crh_scene* scene, const crh_paint* paints, uint32_t n_paints, const int32_t* instance_paint, uint32_t n_instances);

/* Image paints: the source of a Color cover, per sample, from the texels of an image — a bitmap inside a path, a pattern, a glyph atlas, an
 * earlier frame drawn again as a layer (what a user of the reference does with a cover pipeline that samples a texture). An image paint is a
 * type of its own beside crh_paint; one association names both. The model, which the tests check against float64:
 *   image        width x height texels of premultiplied RGBA8 unorm, row 0 = top: the bytes crh_frame_download hands out. T[j][i] is texel
 *                (column i, row j), its four codes / 255 — on the device the f32 value (float)k / 255.0f. Texel (i, j) covers [i, i+1) x [j, j+1).
 *   coordinates  p is the sample's position in the Shape's path coordinates, exactly as for gradients (crh_scene_set_paints above);
 *                u = m0 p.x + m1 p.y + m2, v = m3 p.x + m4 p.y + m5 (f32: fma(p.y, m1, fma(p.x, m0, m2))), then NaN -> 0 and clamped to +-2^24.
 *   NEAREST      value = T[wrap(floor(v), height, spread_y)][wrap(floor(u), width, spread_x)]
 *   LINEAR       a = u - 0.5, i = floor(a), fx = a - i; b = v - 0.5, j = floor(b), fy = b - j;
 *                top = T[j'][i'] + fx (T[j'][i+1'] - T[j'][i']), bottom the same with (j+1)', value = top + fy (bottom - top) per premultiplied
 *                channel, where ' wraps each of the four indices separately: equal texels give their value back exactly.
 *   wrap(i, n)   PAD: clamp(i, 0, n - 1); REPEAT: i - n floor(i / n); REFLECT: k = i - 2n floor(i / 2n), k < n ? k : 2n - 1 - k.
 *                spread_x is applied with the width, spread_y with the height.
 *   source       (value.rgb * (tint.rgb * tint.a), value.a * tint.a) with tint = the instance colour, premultiplied first as the solid colour
 *                is; then clamped and blended exactly as a gradient's source: the renderer's blend state, the frame format's rounding of
 *                writes, the write mask, always the Rgba8Unorm-attachment model.
 *   reads        every texel address is formed from wrapped indices only: no value of (u, v) reads outside the image.
 *   minified     one level and these two filters alias when the image is drawn much smaller than its texels: generate mipmaps and OR
 *                CRH_FILTER_MIPMAP onto the filter (crh_image_generate_mipmaps below).
 * crh_image_create copies width * height * 4 host bytes to the device before it returns; 1 <= width, height <= 16384, else
 * CRH_ERR_INVALID_ARGUMENT. crh_image_create_from_frame settles the frame and copies its resolved bytes on the device: a snapshot — later
 * passes into the frame do not change the image. It takes CRH_FORMAT_RGBA8 and CRH_FORMAT_RGBA8_ATTACHMENT frames that are not restricted by
 * crh_frame_set_tile_rows, anything else is CRH_ERR_UNSUPPORTED. An image belongs to its renderer.
 * crh_scene_set_paints_with_images is crh_scene_set_paints with image paints behind the gradients: instance_paint[i] in [0, n_paints) names
 * gradient i, in [n_paints, n_paints + n_image_paints) image paint (i - n_paints), -1 the solid colour — one association, so no instance
 * carries both. crh_scene_set_paints(s, p, n, a, m) is this call with no image paints; both tables empty clears. Errors as there, with a
 * crh_last_error text, and a failed call leaves the previous table in force: a null image, an unknown filter or spread CRH_ERR_INVALID_ARGUMENT,
 * a non-finite m CRH_ERR_NON_FINITE, an image of another renderer CRH_ERR_INVALID_ARGUMENT. The table keeps the pixels of its images alive (a
 * shared reference) until it is replaced or the Scene is destroyed: crh_image_destroy while a table names the image is legal. The call settles
 * and waits as crh_scene_set_paints does. A pass that draws an image-painted instance through a Color cover runs k_raster_image, the general
 * triangle kernel with the image block; every other pass — a gradient-only table's included — launches what it launched before. */
typedef struct crh_image crh_image;
enum { CRH_FILTER_NEAREST = 0, CRH_FILTER_LINEAR = 1, CRH_FILTER_MIPMAP = 0x100 /* OR-ed onto one of the two: the valid words are 0, 1, 0x100, 0x101 */ };
crh_status crh_image_create(crh_renderer* renderer, uint32_t width, uint32_t height, const void* rgba8, crh_image** out);
crh_status crh_image_create_from_frame(crh_frame* frame, crh_image** out);
crh_status crh_image_size(const crh_image* image, uint32_t* width, uint32_t* height);
void crh_image_destroy(crh_image* image);
/* Mipmaps: a chain of levels below the image, and a filter flag that blends two of them by the size of a pixel in texels (trilinear minification
 * with LINEAR), so that a minified image paint — an atlas under a zoomed-out transform, a layer under a tilted camera — no longer aliases.
 * crh_image_generate_mipmaps builds levels 1 .. L-1 on the device from level 0 (the image), L = floor(log2(max(width, height))) + 1, on the
 * renderer's stream, and returns when they are complete:
 *   level l+1    size (max(1, w_l >> 1), max(1, h_l >> 1)); channel c of its texel (i, j) = (a + b + c + d + 2) >> 2 over the codes of level l at
 *                columns {min(2i, w_l-1), min(2i+1, w_l-1)} x rows {min(2j, h_l-1), min(2j+1, h_l-1)}: integer, bit-exact. Texels are
 *                premultiplied, so the plain mean is the right one and rgb <= a survives it.
 * The levels belong to the image's pixels: a paint table keeps them alive as it keeps level 0, for images of crh_image_create and of
 * crh_image_create_from_frame alike. A second call changes nothing and returns CRH_OK. A paint table holds the levels its images had when it
 * was set: a table set before the call keeps drawing the one level. crh_image_level_count is 1 until then. crh_image_download_level copies
 * level `level` (0 = the image) to `rgba8`, width * height * 4 bytes of that level, and reports its size; rgba8 == NULL only reports the size
 * (width and height may be NULL); level >= the count is CRH_ERR_INVALID_ARGUMENT.
 * CRH_FILTER_MIPMAP on crh_image_paint::filter, evaluated in f32 on the device and checked against float64 by the tests:
 *   J            the derivative of (u, v) by the sample's position (sx, sy) on the frame, in texels per pixel. With (X, Y, W) = the rows of the
 *                inverse path -> pixel homography h applied to (sx, sy, 1) and p = (X, Y) / W: dp.x/dsx = (h0 - p.x h6) / W, dp.x/dsy =
 *                (h1 - p.x h7) / W, p.y the same with h3, h4 — for an affine instance the constants h0, h1, h3, h4, one J per item — and
 *                du/ds = m0 dp.x/ds + m1 dp.y/ds, dv/ds = m3 dp.x/ds + m4 dp.y/ds.
 *   lod          rho = max(|(du/dsx, dv/dsx)|, |(du/dsy, dv/dsy)|); lod = clamp(log2(rho), 0, L - 1), with NaN -> 0 and rho = 0 -> 0 (on the
 *                device half the hardware log2 of rho^2); l0 = floor(lod), f = lod - l0, l1 = min(l0 + 1, L - 1).
 *   sampling     at level l the coordinates are u_l = u * sx_l, v_l = v * sy_l with sx_l = (float)w_l / (float)w_0 (one f32 division on the host),
 *                so that REPEAT and REFLECT periods agree across levels of sizes that are no powers of two; then the base filter's rule
 *                above (NEAREST or LINEAR, each index wrapped per axis with level l's size), giving s(l).
 *   value        s(l0) + f (s(l1) - s(l0)) per premultiplied channel; then `source` above: tint, clamp, blend, format.
 * Hence: an image of one level, and any magnified placement (rho <= 1), give the base filter's bytes exactly (f = 0; the second level is not
 * even fetched for an affine instance); equal levels give their value back exactly; every address is formed from wrapped indices of its own
 * level, so no (u, v) reads outside a level. A pass that draws, through a Color cover, an instance whose image paint carries the flag and
 * whose image had levels when the table was set runs k_raster_mip; every other pass launches what it launched before.
 * Limits: a level of odd width or height drops its last column or row in the step below it (the 2 x 2 blocks cover 2 (w >> 1) columns), so
 * content there fades from the lower levels and sizes that are no powers of two shift by up to a texel per level; the footprint is isotropic
 * (the longer axis of J picks the level: a strongly anisotropic placement blurs along its short axis); levels are not gamma corrected (the
 * codes are averaged as they are, linear light as the frame's bytes are). */
crh_status crh_image_generate_mipmaps(crh_image* image);
crh_status crh_image_level_count(const crh_image* image, uint32_t* count);
crh_status crh_image_download_level(const crh_image* image, uint32_t level, void* rgba8, uint32_t* width, uint32_t* height);
/* Blur: a separable Gaussian of an image on the device — the soft layer behind a drop shadow, a glow, a soft mask, a blurred backdrop. A
 * blurred snapshot of a frame (crh_image_create_from_frame) drawn as an image paint with the tint (0, 0, 0, a) is a drop shadow: the tint rule
 * of `source` above needs nothing more (as an image, in any colour: crh_image_color_filter with a flood matrix). The model is integer and
 * bit-exact; the tests check every byte against it.
 *   taps         one axis, from the f32 sigma widened to double s: R = (uint32_t)ceil(3.0 * s); w[k] = exp(-(k*k) / (2 s s)), k = 0 .. R;
 *                S = w[0] + 2 w[1] + ... + 2 w[R], summed in that order; q[k] = floor(w[k] / S * 65536 + 0.5); then the rounding's deficit
 *                d = 65536 - (q[0] + 2 sum_{k>=1} q[k]), g = sign(d), m = |d| / 2 (integer division): q[1 .. m] += g, q[0] += d - 2 g m.
 *                Symmetric, non-negative, exactly 65536 over the 2 R + 1 positions; every tap within 1.5 of w[k] / S * 65536 (|d| <= 27 over
 *                (0, 64]). s == 0: R = 0 and the single tap 65536, the identity on that axis.
 *   edge         PAD, REPEAT, REFLECT keep the size (w, h): a tap at source index i reads wrap(i, n) by exactly the rules of the image-paint
 *                block above, |i| any multiple of n beyond it (R = 192 on a 1-texel axis). TRANSPARENT takes texels outside the source as
 *                (0, 0, 0, 0) and grows the result to (w + 2 Rx, h + 2 Ry): its texel (i, j) is centred on source texel (i - Rx, j - Ry), so
 *                nothing of a shadow is cut off. A grown side above 16384 is CRH_ERR_UNSUPPORTED.
 *   horizontal   per channel on the 8-bit codes c: t(i, j) = (sum_k qx[|k|] c(i + k, j) + 128) >> 8, k = -Rx .. Rx: a 16-bit value <= 65280
 *                (the sum is <= 255 * 65536 < 2^24).
 *   vertical     out(i, j) = (sum_k qy[|k|] t(i, j + k) + 2^23) >> 24, k = -Ry .. Ry (the sum is <= 65280 * 65536 < 2^32: unsigned 32 bits).
 * Texels are premultiplied, so the plain weighted mean is the right one. Hence: a constant image comes back exactly under the three same-size
 * edges, and on a texel whose window lies wholly inside the source under TRANSPARENT; rgb <= a survives (both roundings are monotone); sigma 0
 * on both axes is a copy. The codes are averaged as they are, with no gamma handling, as the mip levels are.
 * crh_blur_taps is host only (no renderer, no device): it writes q[0 .. R] to `taps` and R to *radius; taps == NULL only reports the radius;
 * capacity < R + 1 with taps is CRH_ERR_INVALID_ARGUMENT; a non-finite sigma CRH_ERR_NON_FINITE; sigma < 0 or > CRH_MAX_BLUR_SIGMA
 * CRH_ERR_INVALID_ARGUMENT with a crh_last_error text. crh_image_blur validates both sigmas through it before it touches the device.
 * crh_image_blur gives a fresh image of the source's renderer with one level (crh_image_generate_mipmaps works on it). The source is not
 * modified and only its level 0 is read. The call runs k_image_blur_h and k_image_blur_v on the renderer's stream and returns when the result
 * is complete, as crh_image_generate_mipmaps does; the intermediate (8 bytes per texel of the result's width and the source's height) is freed
 * before it returns. A null argument or an edge above 3 is CRH_ERR_INVALID_ARGUMENT; a failed allocation or launch frees everything and returns
 * CRH_ERR_HIP; a refused call leaves *out untouched.
 * Limits: the call is synchronous — a caller that blurs every frame waits once per blur; no in-place variant; radii end at
 * CRH_MAX_BLUR_RADIUS; a true Gaussian, no box or recursive approximation, so the cost grows with sigma; a frame is blurred through a
 * snapshot only; no per-pass backdrop filter. */
#define CRH_MAX_BLUR_SIGMA 64.0f
#define CRH_MAX_BLUR_RADIUS 192u
typedef enum crh_blur_edge {
    CRH_BLUR_EDGE_TRANSPARENT = 0,
    CRH_BLUR_EDGE_PAD = 1,
    CRH_BLUR_EDGE_REPEAT = 2,
    CRH_BLUR_EDGE_REFLECT = 3
} crh_blur_edge;
crh_status crh_blur_taps(float sigma, uint32_t* taps, uint32_t capacity, uint32_t* radius); /* host only: no renderer, no device */
crh_status crh_image_blur(const crh_image* src, float sigma_x, float sigma_y, uint32_t edge, crh_image** out);
/* Compositing: two images into a third, texel by texel on the device — what makes snapshots, mipmaps and blurs LAYERS: a mask applied to a
 * layer (DST_IN, SRC_IN), a blend mode, a group opacity, a shadow placed under its layer (DST_OVER at an offset, with the grown origin of
 * a blurred image; its colour from crh_image_color_filter). The model is integer and bit-exact; the tests check every byte against it. All values are 8-bit codes, all arithmetic
 * is unsigned 32-bit.
 *   size         the result has the backdrop's size. Its texel (i, j) pairs backdrop texel (i, j) with source texel (i - x, j - y); outside
 *                the source that texel is (0, 0, 0, 0). Nothing else is special there: SRC_IN, DST_IN, COPY and CLEAR clear outside the
 *                source, exactly as the formula says.
 *   load         each colour code of both texels is clamped to its alpha, c = min(c, a): every term below stays non-negative, and bytes
 *                that are not premultiplied have a defined result.
 *   opacity      the code o = floor((double)opacity * 255 + 0.5); every source code, alpha included, becomes s = (s o + 127) / 255 (integer
 *                division). o = 255 is the identity; the mapping is monotone, so c <= a survives.
 *   blend term   per colour channel, in units of 1 / 255^2, from the source's colour and alpha sc, sa and the backdrop's bc, ba:
 *                NORMAL T = sc ba; MULTIPLY T = sc bc; SCREEN T = sc ba + bc sa - sc bc; DARKEN T = min(sc ba, bc sa);
 *                LIGHTEN T = max(sc ba, bc sa); DIFFERENCE T = |sc ba - bc sa|; EXCLUSION T = sc ba + bc sa - 2 sc bc;
 *                HARD_LIGHT T = 2 sc <= sa ? 2 sc bc : sa ba - 2 (ba - bc) (sa - sc); OVERLAY the same two branches, chosen by 2 bc <= ba.
 *                0 <= T <= sa ba in every mode. Then X = sc (255 - ba) + T (for NORMAL: 255 sc).
 *   operator     fa = A0 + A1 ba and fb = B0 + B1 sa, each one of 0, 255, the other texel's alpha or its complement. (fa, fb) =
 *                CLEAR (0, 0); COPY (255, 0); DST (0, 255); SRC_OVER (255, 255 - sa); DST_OVER (255 - ba, 255); SRC_IN (ba, 0);
 *                DST_IN (0, sa); SRC_OUT (255 - ba, 0); DST_OUT (0, 255 - sa); SRC_ATOP (ba, 255 - sa); DST_ATOP (255 - ba, sa);
 *                XOR (255 - ba, 255 - sa); PLUS (255, 255).
 *   output       co = min(255, (fa X + 255 fb bc + 32512) / 65025), ao = min(255, (fa sa + fb ba + 127) / 255): ONE rounding of the exact
 *                rational value, half up (65025 and 255 are odd: no ties). The mode does not enter ao. The largest numerator is
 *                33 162 750: 32 bits hold it.
 * Hence: co <= ao; NORMAL + SRC_OVER at o = 255 is sc + round(bc (255 - sa) / 255); DST is a copy of the backdrop and COPY the placed
 * source; a transparent source leaves the backdrop unchanged under SRC_OVER, DST_OVER, DST_OUT, SRC_ATOP, XOR and PLUS; every result is
 * within 0.5 code of the W3C compositing-1 real-valued formula evaluated on the codes after the load and opacity stages.
 * crh_composite_validate and crh_composite_texels are host only (no renderer, no device). validate: a null `how` is
 * CRH_ERR_INVALID_ARGUMENT; an op above 12, a mode above 8 or an opacity outside [0, 1] CRH_ERR_INVALID_ARGUMENT with a crh_last_error
 * text; a non-finite opacity CRH_ERR_NON_FINITE. texels: the rule on n pairs of texels (x and y are ignored), 4 n bytes each in the order
 * r g b a at any alignment; out may be either input.
 * crh_image_composite validates before it touches the device: a null argument or images of different renderers are
 * CRH_ERR_INVALID_ARGUMENT, and a refused call leaves *out untouched. backdrop == source is legal. The result is a fresh image of one level
 * (crh_image_generate_mipmaps works on it), complete when the call returns, as crh_image_blur's; only the inputs' level 0 is read and
 * they are not modified. A failed allocation or launch frees everything and returns CRH_ERR_HIP.
 * Limits: the call is synchronous; images are immutable, so there is no in-place variant; offsets are integers; no color-dodge,
 * color-burn or soft-light (they divide or take a root and need an exactness argument of their own) and no non-separable modes; the codes
 * are combined as they are, with no gamma handling; this is not a per-draw blend mode of the raster path. */
typedef enum crh_composite_op { /* Porter-Duff */
    CRH_COMPOSITE_CLEAR = 0,
    CRH_COMPOSITE_COPY = 1,
    CRH_COMPOSITE_DST = 2,
    CRH_COMPOSITE_SRC_OVER = 3,
    CRH_COMPOSITE_DST_OVER = 4,
    CRH_COMPOSITE_SRC_IN = 5,
    CRH_COMPOSITE_DST_IN = 6,
    CRH_COMPOSITE_SRC_OUT = 7,
    CRH_COMPOSITE_DST_OUT = 8,
    CRH_COMPOSITE_SRC_ATOP = 9,
    CRH_COMPOSITE_DST_ATOP = 10,
    CRH_COMPOSITE_XOR = 11,
    CRH_COMPOSITE_PLUS = 12
} crh_composite_op;
typedef enum crh_blend_mode { /* W3C compositing-1 separable modes with a polynomial premultiplied form */
    CRH_BLEND_NORMAL = 0,
    CRH_BLEND_MULTIPLY = 1,
    CRH_BLEND_SCREEN = 2,
    CRH_BLEND_OVERLAY = 3,
    CRH_BLEND_DARKEN = 4,
    CRH_BLEND_LIGHTEN = 5,
    CRH_BLEND_HARD_LIGHT = 6,
    CRH_BLEND_DIFFERENCE = 7,
    CRH_BLEND_EXCLUSION = 8
} crh_blend_mode;
typedef struct crh_composite {
    uint32_t op, mode;
    float opacity; /* [0, 1]; the code o = floor((double)opacity * 255 + 0.5) */
    int32_t x, y;  /* source texel (0, 0) lies over backdrop texel (x, y); any int32 */
} crh_composite;
crh_status crh_composite_validate(const crh_composite* how); /* host only */
crh_status crh_composite_texels(const crh_composite* how, const void* source_rgba8, const void* backdrop_rgba8, uint64_t n, void* out_rgba8); /* host only */
crh_status crh_image_composite(const crh_image* backdrop, const crh_image* source, const crh_composite* how, crh_image** out);
/* Colour filters: every texel of an image through a 4 x 5 matrix on its unpremultiplied colour (SVG feColorMatrix) and then through a
 * 256-entry table per channel (feComponentTransfer), on the device — the colour of a drop shadow (a flood matrix on the blurred layer),
 * a luminance mask turned into alpha for DST_IN, grayscale, saturate, hue rotation, invert, brightness and contrast, a threshold, a
 * per-layer opacity curve, and the gamma tables that linearise before a blur and re-encode after it. The model is integer and bit-exact;
 * the tests check every byte against it. All values are 8-bit codes, all arithmetic is signed 32-bit.
 *   matrix       20 floats, row-major 4 x 5: rows r', g', b', a', columns r, g, b, a, 1. NULL is the identity.
 *   tables       1024 bytes, r[256] g[256] b[256] a[256]. NULL is the identity. Both NULL is a legal copy (of the loaded texels).
 *   load         each colour code is clamped to its alpha, c = min(c, a), as compositing does.
 *   unpremultiply  u_c = (255 c + a / 2) / a (integer division) for a > 0 and 0 for a = 0; u_a = a. Straight 8-bit codes: u_c <= 255
 *                because c <= a.
 *   coefficients k[i][j] = (int32) floor((double) m[i][j] * 65536 + 0.5). Every m is finite (else CRH_ERR_NON_FINITE) and
 *                |m| <= CRH_COLOR_MATRIX_MAX (else CRH_ERR_INVALID_ARGUMENT with a crh_last_error text), so |k| <= 2^20: a signed 24-bit
 *                operand.
 *   matrix stage n_i = k[i][0] u_r + k[i][1] u_g + k[i][2] u_b + k[i][3] u_a + 255 k[i][4] + 32768;
 *                |n_i| <= 5 * 255 * 2^20 + 32768 = 1 336 967 168 < 2^31. v_i = clamp(floor(n_i / 65536), 0, 255), the floor an arithmetic
 *                shift. The identity's k is exactly 65536 on the diagonal: v = u.
 *   table stage  v_i = tables[256 i + v_i] when tables are given.
 *   premultiply  a' = v_a, c' = (v_c v_a + 127) / 255 (integer division). Hence c' <= a'.
 * Hence: the identity (NULL / NULL, the identity matrix, identity tables) returns every premultiplied texel exactly (|u a / 255 - c| <=
 * a / 510 < 1/2 for a < 255; all 32 896 pairs c <= a are tested); a texel with a = 0 goes in as (0, 0, 0, 0) whatever its colour bytes
 * are; the flood matrix — zero colour columns, the bias (r, g, b), m[3][3] = alpha — gives round(colour * round(alpha a)), a shadow's
 * colour; luminanceToAlpha gives an alpha from the straight colour times alpha; without tables every result lies within
 * e_c + e_a + e_c e_a / 255 + 1/2 codes (colour) and e_a (alpha) of the real-valued formula on the loaded codes, where
 * e_i = (1 + sum_{j<3} |m_ij|) / 2 + 5 * 255 * 2^-17.
 * crh_color_filter_validate and crh_color_filter_texels are host only (no renderer, no device). texels: the rule on n texels, 4 n bytes in
 * the order r g b a at any alignment; out may be rgba8; n == 0 is legal, otherwise a null rgba8 or out is CRH_ERR_INVALID_ARGUMENT; a
 * refused call writes nothing.
 * crh_image_color_filter validates before it touches the device: a null src or out is CRH_ERR_INVALID_ARGUMENT, and a refused call leaves
 * *out untouched. The result is a fresh image of the source's renderer and size with one level (crh_image_generate_mipmaps, blur,
 * composite, image paints and crh_frame_load_image work on it), complete when the call returns: k_image_color_filter runs on the
 * renderer's stream. Only level 0 of the source is read and the source is not modified. A failed allocation or launch frees everything
 * and returns CRH_ERR_HIP.
 * Limits: the call is synchronous, like blur and composite — one wait per filter; images are immutable, so there is no in-place variant;
 * the straight intermediates are 8-bit codes, so two filters in a row round twice (fold matrices on the host instead); tables are
 * applied after the matrix only; this is not a per-draw filter of the raster path. */
#define CRH_COLOR_MATRIX_MAX 16.0f
crh_status crh_color_filter_validate(const float* matrix, const uint8_t* tables); /* host only */
crh_status crh_color_filter_texels(const float* matrix, const uint8_t* tables, const void* rgba8, uint64_t n, void* out); /* host only */
crh_status crh_image_color_filter(const crh_image* src, const float* matrix, const uint8_t* tables, crh_image** out);
/* Morphology: the per-channel min (ERODE) or max (DILATE) of an image over a rectangle, on the device (SVG feMorphology) — an outline round
 * text or artwork (a snapshot dilated by n, flooded with a colour by crh_image_color_filter, DST_OVER under the layer at the grown origin),
 * the spread of a shadow or glow (dilate before the blur; erode for a negative spread or an inner shadow), a mask choked or grown before
 * DST_IN, and open / close (one after the other) to remove specks from a rendered mask. The model is exact by nature, because min and max
 * do not round; the tests check every byte against it.
 *   window       out(i, j), per channel c of r, g, b, a independently, is the min (ERODE) or max (DILATE) of c(i + dx, j + dy) over
 *                |dx| <= radius_x, |dy| <= radius_y. The values are the 8-bit codes as they are: no load clamp and no rounding anywhere.
 *   edge         a crh_blur_edge. PAD, REPEAT and REFLECT keep the size (w, h): an index outside the axis reads wrap(i, n) by exactly the
 *                rules of the image-paint block above, any number of periods out (a radius of 192 on a 1-texel axis). TRANSPARENT reads
 *                (0, 0, 0, 0) outside the source.
 *   grown result under TRANSPARENT, DILATE grows the result to (w + 2 radius_x, h + 2 radius_y): its texel (i, j) is centred on source texel
 *                (i - radius_x, j - radius_y), as crh_image_blur grows, so nothing of an outline is cut off. ERODE keeps (w, h): growing
 *                would add zeros only. A grown side above 16384 is CRH_ERR_UNSUPPORTED.
 * Hence: radius (0, 0) is a byte-for-byte copy; rgb <= a survives both operators (min and max are monotone in every channel); under the
 * three same-size edges dilate >= source >= erode texel by texel (the window holds its centre), and erode(x) == 255 - dilate(255 - x);
 * a window that covers a whole axis gives that row's or column's extreme; two dilations (or two erosions) by r1 and then r2 under one edge
 * equal one by r1 + r2 (for TRANSPARENT dilate the origins add); and the window is a rectangle, so rows-then-columns, columns-then-rows
 * and a 2-D pass give the same bytes: the model does not bind the kernels' order.
 * crh_morphology_size and crh_morphology_texels are host only (no renderer, no device) and take 1 <= width, height <= 16384. size:
 * validates and reports the size of the result. texels: the rule on a whole image in host memory, width * height * 4 bytes in the order
 * r g b a at any alignment, row 0 first, into out_rgba8, which holds the result's size; out_rgba8 == rgba8 is refused.
 * Every error is found before the device is touched, and a refused call leaves *out (or the out buffers) untouched and writes nothing: a
 * null argument, op > 1, edge > 3, a radius above CRH_MAX_MORPHOLOGY_RADIUS or a size outside [1, 16384] is CRH_ERR_INVALID_ARGUMENT with a
 * crh_last_error text.
 * crh_image_morphology gives a fresh image of the source's renderer with one level (crh_image_generate_mipmaps, blur, composite, colour
 * filter, image paints and crh_frame_load_image work on it), complete when the call returns: k_image_morph_h (source -> intermediate) and
 * k_image_morph_v (intermediate -> result) run on the renderer's stream, at a cost per texel that does not grow linearly with the radius. Only level 0
 * of the source is read and the source is not modified. The intermediate (packed RGBA8, the result's width and the source's height) is
 * freed before the call returns; a zero radius on an axis skips that axis's pass. A failed allocation or launch frees everything and
 * returns CRH_ERR_HIP.
 * Limits: the call is synchronous, like its siblings — one wait per call; the structuring element is a rectangle: no disc (a round outline or
 * spread is crh_image_distance_field under a table of crh_image_color_filter); the radii are
 * integers; the operator acts per channel on premultiplied codes, as SVG does; images are immutable, so there is no in-place variant. */
#define CRH_MAX_MORPHOLOGY_RADIUS 192u
typedef enum crh_morphology_op {
    CRH_MORPHOLOGY_ERODE = 0,
    CRH_MORPHOLOGY_DILATE = 1
} crh_morphology_op;
crh_status crh_morphology_size(uint32_t width, uint32_t height, uint32_t op, uint32_t radius_x, uint32_t radius_y, uint32_t edge, uint32_t* out_width,
                               uint32_t* out_height); /* host only: validates, and reports the size of the result */
crh_status crh_morphology_texels(uint32_t width, uint32_t height, const void* rgba8, uint32_t op, uint32_t radius_x, uint32_t radius_y, uint32_t edge,
                                 void* out_rgba8); /* host only: the rule on a whole image in host memory */
crh_status crh_image_morphology(const crh_image* src, uint32_t op, uint32_t radius_x, uint32_t radius_y, uint32_t edge, crh_image** out);
/* Convolution: an image through a kernel matrix of up to 15 x 15 entries, on the device (SVG feConvolveMatrix) — sharpen and unsharp,
 * emboss, Sobel, Prewitt and Laplacian edge detection, small box and tent filters, any 3 x 3 or 5 x 5 kernel of an image-processing text.
 * The model is integer and bit-exact: all values are 8-bit codes, all arithmetic is signed 32-bit, and the tests check every byte.
 *   coefficients k[r][c] = (int32) floor((double) kernel[r][c] / (double) divisor * 65536 + 0.5), bias_k = floor((double) bias * 65536 + 0.5).
 *                The double quotient is compared with CRH_CONVOLVE_MAX_GAIN before the conversion, and sum |k[r][c]| <= 64 * 65536 = 2^22,
 *                otherwise the call is refused (the gain limit). Hence |sum k c| <= 2^22 * 255 = 1 069 547 520; with 255 * 65536 of bias
 *                and 32768 of rounding the largest magnitude is 1 086 291 968 < 2^31, and every |k| <= 2^22 is a signed 24-bit operand.
 *   load         each colour code is clamped to its alpha, c = min(c, a), as compositing and the colour filter do.
 *   window       n_ch(i, j) = sum_r sum_c k[r][c] * s_ch(i - target_x + (order_x - 1 - c), j - target_y + (order_y - 1 - r))
 *                             + 255 * bias_k + 32768,
 *                v_ch = clamp(n_ch >> 16, 0, 255) with an arithmetic shift: one rounding of the exact value. The kernel is rotated by
 *                180 degrees, as SVG's is (a true convolution), so SVG kernels carry over unchanged; (target_x, target_y) is the kernel
 *                cell that lies on the output texel (SVG targetX / targetY).
 *   edge         a crh_blur_edge. PAD, REPEAT and REFLECT read wrap(i, n) by exactly the rules of the image-paint block above, any
 *                number of periods out (an order of 15 on a 1-texel axis is legal); TRANSPARENT reads (0, 0, 0, 0) outside the source.
 *   preserve_alpha == 0   s is the loaded premultiplied texel, all four channels; a' = v_a, c' = min(v_c, v_a).
 *   preserve_alpha == 1   the alpha is not convolved: a' = a(i, j). The colour channels of s are the straight codes u_c of the colour
 *                filter's unpremultiply, u_c = (255 c + a / 2) / a (0 for a = 0), and c' = (v_c * a' + 127) / 255, its premultiply.
 * Hence: the 1 x 1 kernel [1] with divisor 1 and bias 0 returns every loaded texel exactly in both modes (under preserve_alpha by the
 * colour filter's identity argument); a kernel with a single 1 at (r, c) is a translation, and under TRANSPARENT equals crh_image_composite
 * COPY onto a transparent backdrop of the same size at the offset (c + target_x - (order_x - 1), r + target_y - (order_y - 1)), byte for
 * byte; a kernel whose quantised entries sum to 65536 + e returns a constant image exactly under the three same-size edges when |e| <= 128
 * (and |e| <= 112 always when the real entries sum to the divisor: each of at most 225 taps rounds by 1/2); c' <= a' always; and with
 * preserve_alpha == 0 every result is within 1/2 + 255 (order_x order_y + 1) / 2^17 codes of the real-valued formula on the loaded codes.
 * crh_convolve_validate, crh_convolve_coefficients and crh_convolve_texels are host only (no renderer, no device). coefficients: the
 * quantised kernel, order_x * order_y entries row-major into k (k == NULL: validate only) and bias_k (may be NULL), as crh_blur_taps
 * hands out taps. texels: the rule on a whole image in host memory, 1 <= width, height <= 16384, width * height * 4 bytes in the order
 * r g b a at any alignment, row 0 first, into out_rgba8 of the same size; out_rgba8 == rgba8 is refused.
 * Every error is found before the device is touched, and a refused call writes nothing and leaves *out untouched: a null argument or
 * kernel is CRH_ERR_INVALID_ARGUMENT; a non-finite kernel entry, divisor or bias is CRH_ERR_NON_FINITE; an order of 0 or above
 * CRH_MAX_CONVOLVE_ORDER, a target >= its order, divisor 0, |bias| > 1, edge > 3, preserve_alpha > 1, the gain limit, a size outside
 * [1, 16384], out_rgba8 == rgba8, and a capacity below order_x * order_y given together with k are CRH_ERR_INVALID_ARGUMENT with a
 * crh_last_error text. The source must belong to a renderer.
 * crh_image_convolve gives a fresh image of the source's renderer and size with one level (crh_image_generate_mipmaps, blur, composite,
 * colour filter, morphology, image paints and crh_frame_load_image work on it), complete when the call returns: k_image_convolve runs on
 * the renderer's stream, a 2-D stencil that stages a tile and its halo in LDS with the edge and the load applied, the coefficients in
 * scalar registers. Only level 0 of the source is read and the source is not modified. A failed allocation or launch frees everything
 * and returns CRH_ERR_HIP.
 * Limits: the call is synchronous, like its siblings — one wait per call; kernels are at most 15 x 15; the result has the source's size
 * under every edge — unlike blur and dilate nothing grows, and a caller who wants a wide kernel's spill takes a larger
 * crh_image_crop of the source first; there is no kernelUnitLength; codes are taken as they are, with no gamma handling. */
#define CRH_MAX_CONVOLVE_ORDER 15u
#define CRH_CONVOLVE_MAX_GAIN 64.0f
typedef struct crh_convolve {
    uint32_t order_x, order_y;   /* 1 .. CRH_MAX_CONVOLVE_ORDER columns and rows of the kernel */
    uint32_t target_x, target_y; /* < order: the kernel cell that lies on the output texel (SVG targetX / targetY) */
    const float* kernel;         /* [order_y][order_x], row-major */
    float divisor;               /* finite, not 0 */
    float bias;                  /* |bias| <= 1 */
    uint32_t edge;               /* crh_blur_edge */
    uint32_t preserve_alpha;     /* 0 / 1 */
} crh_convolve;
crh_status crh_convolve_validate(const crh_convolve* how); /* host only */
crh_status crh_convolve_coefficients(const crh_convolve* how, int32_t* k, uint32_t capacity, int32_t* bias_k); /* host only: the quantised kernel */
crh_status crh_convolve_texels(uint32_t width, uint32_t height, const void* rgba8, const crh_convolve* how, void* out_rgba8); /* host only */
crh_status crh_image_convolve(const crh_image* src, const crh_convolve* how, crh_image** out);
/* Lighting: an image's alpha as a height field, lit by one light, on the device (SVG feDiffuseLighting / feSpecularLighting with
 * feDistantLight / fePointLight / feSpotLight) — bevels, embossed text, raised buttons, glossy highlights, spotlit panels. A frame's
 * snapshot, blurred, is the bump map; CRH_COMPOSITE_SRC_IN masks the lit result to the shape, CRH_BLEND_MULTIPLY applies a diffuse term
 * and CRH_COMPOSITE_PLUS adds a specular one. The result is integer in, integer out and the tests check every byte: all real arithmetic
 * below is IEEE binary64 in exactly the written order and parenthesisation, with only + - * / sqrt and the functions of crh_fmath.h
 * (pow = crh_d_pow, sincos = crh_d_sincos), never contracted, every float field widened to double first, and one rounding to a code at
 * the end. rad(d) = d * (CRH_PI / 180.0); s = surface_scale.
 *   height       A(i, j) = the alpha code of source texel (column i, row j). Outside the image (edge, a crh_blur_edge): TRANSPARENT
 *                gives 0; PAD, REPEAT and REFLECT read wrap(i, n) by exactly the rules of the image-paint block above.
 *   gradient     gx = (A(i+1,j-1) + 2 A(i+1,j) + A(i+1,j+1)) - (A(i-1,j-1) + 2 A(i-1,j) + A(i-1,j+1)), gy the same with rows and
 *                columns exchanged: integers in [-1020, 1020].
 *   normal       nx = (s * (double)(-gx)) / 1020.0, ny = (s * (double)(-gy)) / 1020.0, nz = 1; nlen = sqrt((nx nx + ny ny) + 1.0) >= 1.
 *   light vector DISTANT, once per call: (sa, ca) = sincos(rad(azimuth)), (se, ce) = sincos(rad(elevation)), L = (ca ce, sa ce, se).
 *                POINT, SPOT, per texel: d = (px - (i + 0.5), py - (j + 0.5), pz - (s * A(i,j)) / 255.0), len = sqrt((dx dx + dy dy) + dz dz),
 *                L = d / len per component; len == 0 gives L = (0, 0, 0).
 *   light colour DISTANT, POINT: C = color. SPOT, once per call: S = (points_at - position) / its length (the same sum and square root),
 *                cc = cos(rad(cone_angle)) when cone_angle != 0; per texel m = -((Lx Sx + Ly Sy) + Lz Sz); m <= 0, or a cone with m < cc,
 *                gives C = 0, otherwise C = color * pow(m, spot_exponent) per channel. The cut-off is hard: there is no smoothing band.
 *   DIFFUSE      v = kd * max(((nx Lx + ny Ly) + Lz) / nlen, 0); each colour channel is code(v * C_c), alpha is 255.
 *   SPECULAR     h = (Lx, Ly, Lz + 1.0), hlen = sqrt((hx hx + hy hy) + hz hz); hlen == 0 gives v = 0, otherwise
 *                v = ks * pow(max(((nx hx + ny hy) + hz) / (nlen * hlen), 0), specular_exponent); each colour channel is code(v * C_c) and
 *                alpha is the largest of the three colour codes.
 *   code(t)      t >= 1 ? 255 : floor(t * 255.0 + 0.5). With validated inputs t is finite and not negative.
 * Hence: a constant alpha under the three same-size edges, or s == 0, gives a constant image under a distant light, for DIFFUSE
 * code(kd * max(Lz, 0) * C); an elevation of 90 on a flat field gives code(kd C) for DIFFUSE and code(ks C) for SPECULAR; constant == 0
 * gives (0, 0, 0, 255) for DIFFUSE and (0, 0, 0, 0) for SPECULAR; the source's colour channels never enter the result; a SPECULAR colour
 * never exceeds its alpha, so the texel is a valid premultiplied one; a point light at (w - px, py, pz) over the horizontally mirrored
 * image gives the mirrored bytes exactly (every coordinate involved is exact in binary64); and every code is within 0.5 + 10^-6 of the
 * real-valued SVG formula on the same inputs (at most 12 binary64 operations and one crh_d_pow, whose |y| <= 745 keeps its relative error
 * below 10^-13, stand between the inputs and t: a few 10^-11 of a code).
 * Fields that the chosen op / light does not use are not read and not validated. crh_lighting_validate and crh_lighting_texels are host
 * only (no renderer, no device). texels: the rule on a whole image in host memory, 1 <= width, height <= 16384, width * height * 4 bytes
 * in the order r g b a at any alignment, row 0 first, into out_rgba8 of the same size; out_rgba8 == rgba8 is refused.
 * Every error is found before the device is touched, and a refused call writes nothing and leaves *out untouched: a null argument, an
 * op above CRH_LIGHTING_SPECULAR, a light above CRH_LIGHT_SPOT, an edge above CRH_BLUR_EDGE_REFLECT are CRH_ERR_INVALID_ARGUMENT; then a
 * non-finite used field is CRH_ERR_NON_FINITE; then a used value outside its range (below), points_at == position, a size outside
 * [1, 16384] and out_rgba8 == rgba8 are CRH_ERR_INVALID_ARGUMENT, each with a crh_last_error text. The source must belong to a renderer.
 * crh_image_lighting gives a fresh image of the source's renderer, size and origin with one level (mipmaps, blur, composite, colour
 * filter, morphology, convolution, image paints and crh_frame_load_image work on it), complete when the call returns: k_image_lighting
 * runs on the renderer's stream, a 3 x 3 stencil on alpha codes staged in LDS with the edge applied, specialised on (op, light). Only
 * the alpha of level 0 of the source is read and the source is not modified. A failed allocation or launch frees everything and
 * returns CRH_ERR_HIP.
 * Limits: the edges are the library's four, not SVG's one-sided border kernels (PAD halves the border slope compared with SVG); one
 * light per call — several lights are several calls joined by CRH_COMPOSITE_PLUS; there is no kernelUnitLength; the call is
 * synchronous, like its siblings; light coordinates are in the image's own texel space (x right, y down, z towards the viewer) — a
 * grown blur's origin is the caller's to add. */
typedef enum crh_lighting_op { CRH_LIGHTING_DIFFUSE = 0, CRH_LIGHTING_SPECULAR = 1 } crh_lighting_op;
typedef enum crh_light_kind { CRH_LIGHT_DISTANT = 0, CRH_LIGHT_POINT = 1, CRH_LIGHT_SPOT = 2 } crh_light_kind;
typedef struct crh_lighting {
    uint32_t op, light, edge;      /* edge: crh_blur_edge, what the height field is outside the image */
    float surface_scale;           /* s: height of alpha 255 in texels; finite, |s| <= 256 */
    float constant;                /* kd or ks; [0, 256] */
    float specular_exponent;       /* SPECULAR: [1, 128]; DIFFUSE: ignored */
    float color[3];                /* the light's colour, each in [0, 1] */
    float azimuth, elevation;      /* DISTANT: degrees, |.| <= 3600 */
    float position[3];             /* POINT, SPOT: texel coordinates (x right, y down, z towards the viewer), |.| <= 2^20 */
    float points_at[3];            /* SPOT: |.| <= 2^20, must differ from position */
    float spot_exponent;           /* SPOT: [0, 128] */
    float cone_angle;              /* SPOT: degrees; 0 = no cone, otherwise in (0, 90] */
} crh_lighting;
crh_status crh_lighting_validate(const crh_lighting* how); /* host only */
crh_status crh_lighting_texels(uint32_t width, uint32_t height, const void* rgba8, const crh_lighting* how, void* out_rgba8); /* host only */
crh_status crh_image_lighting(const crh_image* src, const crh_lighting* how, crh_image** out);
/* Turbulence: an image made of procedural noise on the device (SVG feTurbulence, Perlin's fractalNoise and turbulence) — paper grain,
 * clouds, marble, wood, the bump map of rough metal under crh_image_lighting, a dissolve mask for CRH_COMPOSITE_DST_IN, film grain with
 * CRH_BLEND_OVERLAY. The only image call that makes pixels instead of changing them. Integer tables in, one rounding to a code out, and
 * the tests check every byte: all real arithmetic below is IEEE binary64 in exactly the written order and parenthesisation, with only
 * + - * /, sqrt and crh_floor_d, never contracted, every float field widened to double first; ceil(x) = -floor(-x).
 *   seed         in 64-bit integers: s = seed; s <= 0 gives s = (|s| mod 2147483646) + 1; s > 2147483646 gives s = 2147483646.
 *   random step  rnd(s) = 16807 * (s mod 127773) - 2836 * (s div 127773), plus 2147483647 when that is <= 0. Every draw below first does
 *                s = rnd(s) and then uses s.
 *   gradients    for k = 0..3 (r, g, b, a) outermost and i = 0..255 inside, two draws: gx = (double)((s mod 512) - 256) / 256.0, then gy
 *                the same way; n = sqrt(gx gx + gy gy); G[k][i] = (gx / n, gy / n), and (0, 0) when n == 0 (seed 346: k = 1, i = 164).
 *   lattice      after all gradients: lat[i] = i for 0..255; then for i = 255 down to 1: a draw, j = s mod 256, swap lat[i] and lat[j].
 *   frequency    per axis, n = width or height, f = the widened base frequency. stitch == 0 or f == 0: the frequency is f and the period
 *                P = 0. Otherwise lo = floor(n f) / n, hi = ceil(n f) / n, f' = (f / lo < hi / f) ? lo : hi (lo == 0: the quotient is
 *                +inf, so hi), P = (int)floor(n f' + 0.5) >= 1. Octave o uses the period P << o.
 *   point        texel (column i, row j): vx = ((double)offset[0] + (double)i) * fx, vy likewise with j and fy; after each octave
 *                vx = vx * 2.0 and vy = vy * 2.0.
 *   noise(k, vx, vy, Px, Py)
 *                flx = floor(vx), ix = (int)flx, rx0 = vx - flx, rx1 = rx0 - 1.0; the y axis the same. wrap(i, P) = (P == 0 ? i : i mod P,
 *                taken non-negative) & 255, applied to ix, ix + 1, iy and iy + 1 separately: bx0, bx1, by0, by1. a0 = lat[bx0],
 *                a1 = lat[bx1]; b00 = lat[(a0 + by0) & 255], b10 = lat[(a1 + by0) & 255], b01 = lat[(a0 + by1) & 255],
 *                b11 = lat[(a1 + by1) & 255]. sx = (rx0 rx0) * (3.0 - (2.0 rx0)), sy likewise. With q = G[k][b]:
 *                u = (rx0 q00.x) + (ry0 q00.y), v = (rx1 q10.x) + (ry0 q10.y), a = u + (sx * (v - u));
 *                u = (rx0 q01.x) + (ry1 q01.y), v = (rx1 q11.x) + (ry1 q11.y), b = u + (sx * (v - u)); the noise is a + (sy * (b - a)).
 *   sum          sum = 0, ratio = 1; per octave sum = sum + (N / ratio), N = the noise for FRACTAL_NOISE and its absolute value for
 *                TURBULENCE; then ratio = ratio * 2.0.
 *   code         t = (sum + 1.0) * 0.5 for FRACTAL_NOISE, t = sum for TURBULENCE; code = t >= 1 ? 255 : t > 0 ? (int)floor(t * 255.0 + 0.5) : 0.
 *   texel        premultiplied, as every image here: A = opaque ? 255 : code_a (with opaque, channel 3 is not evaluated); each colour
 *                byte is (code_c * A + 127) / 255 in integers; the alpha byte is A.
 * With the validated ranges |vx| <= (65536 + 16384) * 4 * 2^11 < 2^31: lattice coordinates and periods fit 32 bits and crh_floor_d's
 * precondition holds.
 * Hence: rgb <= a in every texel; octaves == 0, or both frequencies 0, or integer-valued offsets with integer frequencies (every point
 * is a lattice point) give a constant image — FRACTAL_NOISE (64, 64, 64, 128), with opaque (128, 128, 128, 255); TURBULENCE
 * (0, 0, 0, 0), with opaque (0, 0, 0, 255); seeds 0 and 1 give the same image, seed -1 that of seed 2; window: with stitch == 0 an image
 * of any size at offset (x + dx, y + dy) equals the window at (dx, dy) of the image at offset (x, y) for integer dx, dy and
 * float-representable sums, so a large texture can be made in pieces; period: with stitch == 1, a power-of-two width and height and
 * integer offsets, the image at offset (x + w, y + h) is byte-equal to the one at (x, y) (all products are then exact; without stitch it
 * is not); base_frequency[1] does not enter when height == 1 and offset[1] makes vy an integer, and likewise for x.
 * crh_turbulence_validate, crh_turbulence_tables (the seeded tables, gradient[(k * 256 + i) * 2 + c]) and crh_turbulence_texels (the rule
 * on a whole image in host memory, width * height * 4 bytes in the order r g b a at any alignment, row 0 first) are host only: no
 * renderer, no device.
 * Every error is found before the device is touched, and a refused call writes nothing and leaves *out untouched: first a null
 * argument, a kind above CRH_TURBULENCE_TURBULENCE, stitch or opaque above 1 and octaves above CRH_MAX_TURBULENCE_OCTAVES are
 * CRH_ERR_INVALID_ARGUMENT; then a non-finite frequency or offset is CRH_ERR_NON_FINITE; then a frequency outside
 * [0, CRH_TURBULENCE_MAX_FREQUENCY], an offset outside +-CRH_TURBULENCE_MAX_OFFSET and a size outside [1, 16384] are
 * CRH_ERR_INVALID_ARGUMENT, each with a crh_last_error text "crh_turbulence_validate: ...".
 * crh_image_turbulence gives a fresh image of the renderer with one level and origin (0, 0) (mipmaps, blur, composite, colour filter,
 * morphology, convolution, lighting, image paints and crh_frame_load_image work on it), complete when the call returns: the tables are
 * built on the host and uploaded once per call, and k_image_turbulence runs on the renderer's stream, specialised on (kind, opaque,
 * stitched), the tables in LDS. A failed allocation or launch frees everything and returns CRH_ERR_HIP.
 * Limits: lattice coordinates are taken with floor and stitching is a true modulo, so values differ from a browser's, which follows the
 * SVG sample code's +4096 offset and its wrap bookkeeping — the statistics and the look are the same; the stitch tile is the image
 * itself; the output is linear codes with no colour-space handling; the call is synchronous, like its siblings. */
#define CRH_MAX_TURBULENCE_OCTAVES 12u
#define CRH_TURBULENCE_MAX_FREQUENCY 4.0f
#define CRH_TURBULENCE_MAX_OFFSET 65536.0f
typedef enum crh_turbulence_kind { CRH_TURBULENCE_FRACTAL_NOISE = 0, CRH_TURBULENCE_TURBULENCE = 1 } crh_turbulence_kind;
typedef struct crh_turbulence {
    uint32_t kind;              /* crh_turbulence_kind */
    uint32_t octaves;           /* 0 .. CRH_MAX_TURBULENCE_OCTAVES */
    int32_t  seed;              /* any */
    uint32_t stitch;            /* 0 or 1: the image tiles seamlessly with itself */
    uint32_t opaque;            /* 0: alpha is the fourth noise channel (SVG); 1: alpha = 255, three channels of noise */
    float base_frequency[2];    /* lattice cells per texel, x and y; each in [0, CRH_TURBULENCE_MAX_FREQUENCY] */
    float offset[2];            /* noise-space position of texel (0, 0); each |.| <= CRH_TURBULENCE_MAX_OFFSET */
} crh_turbulence;
crh_status crh_turbulence_validate(const crh_turbulence* how);                                        /* host only */
crh_status crh_turbulence_tables(int32_t seed, uint8_t lattice[256], double gradient[4 * 256 * 2]);   /* host only: gradient[(k*256 + i)*2 + c] */
crh_status crh_turbulence_texels(uint32_t width, uint32_t height, const crh_turbulence* how, void* out_rgba8); /* host only */
crh_status crh_image_turbulence(crh_renderer* renderer, uint32_t width, uint32_t height, const crh_turbulence* how, crh_image** out);
/* Displacement: a new image that reads `src` through a per-texel offset taken from a second image, the map (SVG feDisplacementMap) —
 * water, heat haze, torn edges, wobbly text, a frosted backdrop from a blurred snapshot; crh_image_turbulence makes the usual map. All
 * values are 8-bit codes, everything is integer and bit-exact, and the tests check every byte.
 *   size      src and map have one size (w, h); the result has that size, one level, origin (0, 0), and belongs to the source's renderer.
 *             Neither image is modified, and the map may be the source itself: map == src is legal.
 *   map code  the map texel (i, j) is loaded as the colour filter loads a texel: c = min(c, a). A colour channel gives the straight code
 *             u = (255 c + a / 2) / a, and 0 for a = 0; CRH_CHANNEL_A gives u = a. ux comes from x_channel, uy from y_channel.
 *   offset    per axis, in units of 1/256 texel: K = (int32) floor((double) scale * 256 + 0.5), so |K| <= 2^18; n = K (2 u - 255), so
 *             |n| < 2^26; q = floor((n + 255) / 510), a true floor, also for negative n: scale (u / 255 - 1/2) rounded half up,
 *             |q| <= 2^17.
 *   position  X = 256 i + 128 + qx and Y = 256 j + 128 + qy, both below 2^23 in magnitude.
 *   NEAREST   the value is S(X >> 8, Y >> 8), with arithmetic shifts.
 *   LINEAR    ax = X - 128, i0 = ax >> 8, fx = ax & 255, the y axis the same. Per channel top = S(i0, j0) (256 - fx) + S(i0 + 1, j0) fx,
 *             bottom the same with j0 + 1; value = (top (256 - fy) + bottom fy + 32768) >> 16: one rounding, the largest numerator is
 *             16 744 448 < 2^24.
 *   S(i, j)   the source's codes as they are, with no load clamp, as morphology reads them. Under PAD, REPEAT and REFLECT each index
 *             goes separately through the image-paint block's wrap(i, n); the index may lie any number of periods out: 513 texels
 *             beyond a 1-texel axis. Under TRANSPARENT the value is (0, 0, 0, 0) when either index is outside. Every address is formed
 *             from wrapped or tested indices only: no map value reads outside the source.
 * Hence: scales (0, 0) give a byte-for-byte copy under both filters and every edge, and a zero scale on one axis leaves that axis
 * exactly unmoved; equal texels come back exactly; rgb <= a survives (the weights are shared and the rounding is monotone); scale 510
 * gives q = 256 (2 u - 255) exactly, so each texel reads the source 2 u - 255 whole texels away, both filters agree and the result is
 * S(i + 2 ux - 255, j + 2 uy - 255); a constant map whose q is a multiple of 256 is a translation, under TRANSPARENT byte for byte
 * crh_image_composite's COPY of the source onto a transparent backdrop of the same size at offset (-qx / 256, -qy / 256); as in SVG no
 * code gives a zero offset: u = 127 gives -scale / 510, u = 128 gives +scale / 510, and a transparent map texel has u = 0 and moves by
 * -scale / 2; q is within 3/4 of a 1/256 texel of the real scale (u / 255 - 1/2) * 256: 1/2 from the rounding plus 1/4 from K.
 * crh_displace_validate, crh_displace_offset (the q of two straight codes <= 255, as crh_blur_taps hands out taps; a code above 255 is
 * CRH_ERR_INVALID_ARGUMENT) and crh_displace_texels (the rule on whole images in host memory, width * height * 4 bytes each in the
 * order r g b a at any alignment, row 0 first) are host only: no renderer, no device.
 * Every error is found before the device is touched, and a refused call writes nothing and leaves *out untouched: first a null argument
 * is CRH_ERR_INVALID_ARGUMENT; then a channel above CRH_CHANNEL_A, a filter other than CRH_FILTER_NEAREST or CRH_FILTER_LINEAR (the
 * MIPMAP flag is refused) and an edge above CRH_BLUR_EDGE_REFLECT are CRH_ERR_INVALID_ARGUMENT; then a non-finite scale is
 * CRH_ERR_NON_FINITE; then, in this order, a |scale| above CRH_MAX_DISPLACE_SCALE, a size outside [1, 16384], a map of another size,
 * images of different renderers, and in crh_displace_texels an out_rgba8 equal to either input are CRH_ERR_INVALID_ARGUMENT, each with a
 * crh_last_error text "crh_displace_validate: ...".
 * crh_image_displace runs k_image_displace on the renderer's stream, specialised on the filter and on TRANSPARENT against the wrapping
 * edges; it allocates nothing but the result. A failed allocation or launch frees everything and returns CRH_ERR_HIP.
 * Limits: the call is synchronous, like its siblings; map and source must have one size — crh_image_crop brings one to the other's if
 * they do not; the footprint is a point or a 2 x 2 bilinear one, so strong local compression of the map aliases; the map is used in its own
 * codes, with no colour-space handling; this is not a per-draw effect of the raster path. */
typedef enum crh_channel { CRH_CHANNEL_R = 0, CRH_CHANNEL_G = 1, CRH_CHANNEL_B = 2, CRH_CHANNEL_A = 3 } crh_channel;
#define CRH_MAX_DISPLACE_SCALE 1024.0f
typedef struct crh_displace {
    float scale[2];                 /* x and y; finite, |.| <= CRH_MAX_DISPLACE_SCALE (SVG has one scale: give it twice) */
    uint32_t x_channel, y_channel;  /* crh_channel of the map that moves x, and y */
    uint32_t filter;                /* CRH_FILTER_NEAREST or CRH_FILTER_LINEAR (the MIPMAP flag is refused) */
    uint32_t edge;                  /* crh_blur_edge: what the SOURCE is outside itself */
} crh_displace;
crh_status crh_displace_validate(const crh_displace* how);                                             /* host only */
crh_status crh_displace_offset(const crh_displace* how, uint32_t code_x, uint32_t code_y, int32_t q[2]); /* host only: q of two straight codes <= 255 */
crh_status crh_displace_texels(uint32_t width, uint32_t height, const void* rgba8, const void* map_rgba8, const crh_displace* how, void* out_rgba8); /* host only */
crh_status crh_image_displace(const crh_image* src, const crh_image* map, const crh_displace* how, crh_image** out);
/* Distance fields: a new image that holds, for every texel, the exact Euclidean distance to a shape, coded into 8 bits over a chosen
 * spread — the round outline, glow and spread that crh_image_morphology's rectangle cannot make, and the chiselled bevel that a blurred
 * height field cannot: a 256-entry table of crh_image_color_filter turns the distance into an outline of any width or a falloff of any
 * profile, CRH_COMPOSITE_DST_OVER puts it under the layer at the grown origin, crh_image_lighting lights the INSIDE distance as a
 * chisel, an image paint's tint colours it. Squared distances between texel centres are integers and the code is one rounding with an
 * integer statement, so every byte is defined and the tests check every byte.
 *   inside(x, y)  for any integer position: under PAD, REPEAT and REFLECT code(wrap(x, w), wrap(y, h)) >= threshold, code the stored
 *             (premultiplied) code of `channel` as it is and wrap the image-paint block's, any number of periods out; under
 *             TRANSPARENT a position outside the source is not inside.
 *   D2(p)     OUTSIDE: 0 if inside(p), otherwise the least |p - q|^2 over the positions q with inside(q), or "none" if there is no
 *             such q. INSIDE: 0 if not inside(p), otherwise the least |p - q|^2 over the q with not inside(q). Texel centres sit at
 *             integer coordinates, so D2 is an integer.
 *   c(D2)     min(255, floor(255 sqrt(D2) / spread + 1/2)), in integers: c(0) = 0, otherwise the largest c in [0, 255] with
 *             (2 c - 1)^2 spread^2 <= 260100 D2 (64-bit arithmetic; a tie rounds up); "none" gives 255. Every D2 >= spread^2 gives 255,
 *             so no q farther than `spread` from p can change a byte: this is what bounds the kernels' windows.
 *   result    v = 255 - c (OUTSIDE: 255 on the shape, falling to 0 at `spread` — glow, outline, spread) or c (INSIDE: 0 off the
 *             shape, rising into it — chisel, inner glow); the texel is (v, v, v, v): premultiplied-valid, a mask, a table's input,
 *             a tint's, a height field.
 *   size      OUTSIDE under TRANSPARENT grows the result to (w + 2 spread, h + 2 spread), texel (i, j) centred on the source's
 *             (i - spread, j - spread), as blur and dilate grow; a grown side above 16384 is CRH_ERR_UNSUPPORTED. INSIDE keeps (w, h)
 *             under every edge (growing would add zeros only), and so do the other edges. One level; the mirrors carry the origin.
 * Hence: with spread 4, OUTSIDE and one inside texel, D2 = 1, 2, 4, 5, 9, 16 give c = 64, 90, 128, 143, 191, 255 (D2 = 4 is a tie:
 * 255 * 4 = 510 * 2) and the bytes 191, 165, 127, 112, 64, 0; an inside texel is 255 (OUTSIDE) and at least c(1) (INSIDE); INSIDE of an
 * image is 255 - OUTSIDE of its complement (code -> 255 - code, threshold t -> 256 - t) under the three same-size edges; the transpose
 * of the result is the result of the transpose; under REPEAT a roll of the source rolls the result; neighbouring bytes differ by at most
 * c(1) + 1; on a binarised image under PAD {v >= 255 - c(r^2)} lies within crh_image_morphology's dilate(r, r) and contains
 * dilate(k, k) for 2 k^2 <= r^2.
 * crh_distance_validate, crh_distance_code (the result byte v of one D2 under how's mode and spread, as crh_blur_taps hands out taps), crh_distance_size and crh_distance_texels
 * (the rule on a whole image in host memory, width * height * 4 bytes in, the result's size out, r g b a at any alignment, row 0
 * first; not quadratic in the spread) are host only: no renderer, no device.
 * Every error is found before the device is touched, and a refused call writes nothing and leaves *out and the out buffers untouched:
 * first a null argument; then a mode above CRH_DISTANCE_INSIDE, a channel above CRH_CHANNEL_A, a threshold outside [1, 255], a spread
 * outside [1, CRH_MAX_DISTANCE_SPREAD] and an edge above CRH_BLUR_EDGE_REFLECT; then a size outside [1, 16384] and, in
 * crh_distance_texels, an out_rgba8 equal to rgba8 are CRH_ERR_INVALID_ARGUMENT; then a grown side above 16384 is
 * CRH_ERR_UNSUPPORTED; each with a crh_last_error text "crh_distance_validate: ...".
 * crh_image_distance_field runs two kernels on the renderer's stream with one scratch allocation (the thresholds of c and one byte per
 * texel of the result): k_image_distance_v takes the source to g, the distance along the column (0 .. spread - 1, or "nothing within
 * reach"), k_image_distance_h takes g to the result by D2(x, y) = min over dx of dx^2 + g(x + dx, y)^2, which is exact. Only level 0
 * of the source is read and the source is not modified. A failed allocation or launch frees everything and returns CRH_ERR_HIP.
 * Limits: the call is synchronous, like its siblings; the source is binarised, so there is no sub-texel refinement from antialiased
 * coverage; distances are between texel centres, not to the boundary between texels; there is no signed mode: INSIDE and OUTSIDE are
 * two calls; the spread is an integer and at most 255. */
#define CRH_MAX_DISTANCE_SPREAD 255u
typedef enum crh_distance_mode { CRH_DISTANCE_OUTSIDE = 0, CRH_DISTANCE_INSIDE = 1 } crh_distance_mode;
typedef struct crh_distance {
    uint32_t mode;      /* crh_distance_mode */
    uint32_t channel;   /* crh_channel; the stored (premultiplied) code as it is */
    uint32_t threshold; /* 1..255: a texel is inside iff code >= threshold */
    uint32_t spread;    /* 1..CRH_MAX_DISTANCE_SPREAD, in texels */
    uint32_t edge;      /* crh_blur_edge */
} crh_distance;
crh_status crh_distance_validate(const crh_distance* how);                                               /* host only */
crh_status crh_distance_code(const crh_distance* how, uint64_t squared_distance, uint32_t* code);        /* host only: the result byte of one D2 */
crh_status crh_distance_size(uint32_t width, uint32_t height, const crh_distance* how, uint32_t* out_width, uint32_t* out_height); /* host only */
crh_status crh_distance_texels(uint32_t width, uint32_t height, const void* rgba8, const crh_distance* how, void* out_rgba8);      /* host only */
crh_status crh_image_distance_field(const crh_image* src, const crh_distance* how, crh_image** out);
/* Resize: a new image of any size in [1, 16384]^2 that holds the whole source, resampled — "this layer at 37 % size", a 2x supersampled
 * frame down to the display's size, a thumbnail, the half-resolution blur (down, blur, up). The filter widens with the ratio when it
 * minifies, so it does not alias at any ratio, and it is separable: one table of integer taps per axis, which differ per output texel.
 * Integer on the texels and bit-exact, so every byte is defined and the tests check every byte.
 * An axis of n source texels and m result texels, both in [1, 16384]; per output index o, all real arithmetic in binary64 exactly in the
 * order and parenthesisation written, never contracted, floor and / the IEEE operations:
 *   s         max(1.0, (double)n / m): the filter widens when minifying and not when magnifying.
 *   c         ((o + 0.5) * n) / m: the whole source maps onto the whole result, texel centres at half-integers.
 *   f, r      the filter and its support; a = |x|, f = 0 where no case applies:
 *               BOX          r = 0.5   1 for -0.5 <= x < 0.5 (nearest when magnifying, the area mean at integer ratios)
 *               TRIANGLE     r = 1     1 - a for a < 1 (bilinear when magnifying)
 *               CATMULL_ROM  r = 2     ((1.5 a - 2.5) a) a + 1 for a < 1; ((-0.5 a + 2.5) a - 4) a + 2 for a < 2
 *               MITCHELL     r = 2     (((21 a - 36) a) a + 16) / 18 for a < 1; (((-7 a + 36) a - 60) a + 32) / 18 for a < 2
 *                                      (Mitchell-Netravali with B = C = 1/3; Catmull-Rom is B = 0, C = 1/2)
 *               LANCZOS3     r = 3     1 at a = 0; ((3 s1) s3) / (p p) for a < 3 with p = CRH_PI a, s1 = sin p, s3 = sin(p / 3),
 *                                      both sines from crh_d_sincos of include/crh_fmath.h
 *   window    lo = max(0, (int)floor(c - r s)), hi = min(n - 1, (int)floor(c + r s)), count = hi - lo + 1 >= 1. Taps that fall outside
 *             the source are dropped and the rest renormalised: this is the edge rule. There are no edge modes and nothing outside the
 *             image is ever read.
 *   weights   w[t] = f((((lo + t) + 0.5) - c) / s), t = 0 .. count - 1; S = the sum of w in ascending t, from 0.0;
 *             q[t] = (int)floor(w[t] / S * 16384 + 0.5), signed.
 *   deficit   d = 16384 - sum q. The |d| taps nearest the centre each take sign(d): nearest is ascending |((lo + t) + 0.5) - c|, ties to
 *             the lower t. So sum q = 16384 exactly.
 *   checked   count <= CRH_MAX_RESIZE_TAPS, else the axis is CRH_ERR_UNSUPPORTED; and |d| <= count and sum |q| <= 32768 (the largest seen is
 *             25748: LANCZOS3, 4 to 5, output 2), else CRH_ERR_UNSUPPORTED as well, which no pair of sizes is known to meet.
 * Texels, per channel on the stored 8-bit codes as they are (premultiplied; no gamma), in signed 32-bit arithmetic, >> arithmetic (floor):
 *   horizontal  t(o, j) = clamp((sum_t qx[t] c(lo + t, j) + 32) >> 6, 0, 65280): units of 1/256 code in 16 bits; |sum| <= 255 * 32768 < 2^23.
 *               The intermediate has the result's width and the source's height.
 *   vertical    v(o, i) = clamp((sum_t qy[t] t(o, lo + t) + 2^21) >> 22, 0, 255); |sum| + 2^21 <= 65280 * 32768 + 2^21 < 2^31, which is what
 *               the bound on sum |q| is for.
 *   result      alpha = v_a; each colour = min(v, alpha): negative lobes do not keep rgb <= a on their own.
 * Hence: a constant image comes back exactly at every size and filter; n == m on both axes is a copy, byte for byte, under every filter
 * but MITCHELL, which is not interpolating (its taps there are 1/18, 8/9, 1/18: 910, 14564, 910); BOX at an integer ratio is within 0.51
 * code of the real mean of its n/m x n/m texels; rgb <= a always holds; under BOX and TRIANGLE no tap is negative and no clamp binds.
 * crh_resize_taps (the taps of one axis: first[m], count[m], and sum of count signed taps back to back in `taps`, whose number goes to
 * *total if total is not null; with all three arrays null it only reports *total; capacity is the room in `taps`) and crh_resize_texels
 * (the rule on a whole image in host memory, width * height * 4 bytes in, out_width * out_height * 4 out, r g b a at any alignment, row 0
 * first) are host only: no renderer, no device.
 * Every error is found before the device is touched, and a refused call writes nothing and leaves *out and the out buffers untouched:
 * first a null argument (crh_resize_taps: some but not all of the arrays null, or no array and no total); then a side of 0 or above
 * 16384, a filter above CRH_RESIZE_LANCZOS3, in crh_resize_texels an out_rgba8 equal to rgba8 and in crh_resize_taps a capacity below
 * the total are CRH_ERR_INVALID_ARGUMENT; then an axis over the tap cap is CRH_ERR_UNSUPPORTED; each with a crh_last_error text
 * "crh_resize_taps: ...".
 * crh_image_resize runs two kernels on the renderer's stream with one scratch allocation (both axes' tables in one upload at its head,
 * then the intermediate, 8 bytes per texel): k_image_resize_h and k_image_resize_v. The result is a fresh one-level image of the
 * source's renderer, complete on return, with origin (0, 0); only level 0 of the source is read and the source is not modified. A
 * failed allocation or launch frees everything and returns CRH_ERR_HIP.
 * Limits: the call is synchronous, like its siblings; one call minifies an axis by at most the ratio whose window holds 512 texels,
 * about 500 (BOX), 250 (TRIANGLE), 127 (CATMULL_ROM, MITCHELL) and 85 (LANCZOS3): beyond it chain two calls or take a mip level first;
 * the codes are filtered as they are, with no gamma handling; the scale is axis-aligned: rotation and perspective stay with image paints. */
#define CRH_MAX_RESIZE_TAPS 512u
typedef enum crh_resize_filter { CRH_RESIZE_BOX = 0, CRH_RESIZE_TRIANGLE = 1, CRH_RESIZE_CATMULL_ROM = 2, CRH_RESIZE_MITCHELL = 3, CRH_RESIZE_LANCZOS3 = 4 } crh_resize_filter;
crh_status crh_resize_taps(uint32_t n, uint32_t m, uint32_t filter, int32_t* first, uint16_t* count, int16_t* taps, uint64_t capacity, uint64_t* total); /* host only */
crh_status crh_resize_texels(uint32_t width, uint32_t height, const void* rgba8, uint32_t out_width, uint32_t out_height, uint32_t filter, void* out_rgba8); /* host only */
crh_status crh_image_resize(const crh_image* src, uint32_t width, uint32_t height, uint32_t filter, crh_image** out);
/* Regions and statistics: part of an image or of a frame as a new image, and where an image's content is — so that the drop shadow of a
 * 300 x 200 button in a 4096 x 4096 frame filters 300 x 200 texels, not 64 MB four times, and nothing goes through the host to find the
 * button. A crop is a copy and the statistics are counts: every byte and every counter is defined, and the tests check each.
 *   crop        the result is width x height, each in [1, 16384], one level; its texel (i, j) is the source's texel (x + i, y + j), the
 *               bytes exactly as stored (a copy: nothing is clamped to alpha), and (0, 0, 0, 0) where that lies outside the source. x and
 *               y are any int32. A rectangle that misses the source entirely is legal and gives a transparent image: this is how an
 *               empty canvas is made, and a rectangle larger than the source is the larger transparent backdrop that a filter's spill
 *               or a map of another size needs. The mirrors give the result the origin (origin.x - x, origin.y - y), which may be negative.
 *   frame region  crh_image_create_from_frame_region is, byte for byte, crh_image_crop of what crh_image_create_from_frame would return,
 *               without the full-size copy: one kernel reads the frame's resolved bytes. It settles the frame as that call does and
 *               refuses what it refuses (a format other than CRH_FORMAT_RGBA8 and CRH_FORMAT_RGBA8_ATTACHMENT, a frame restricted by
 *               crh_frame_set_tile_rows: CRH_ERR_UNSUPPORTED); a cleared frame gives zeros. The size limit is the region's, not the
 *               frame's: a frame of more than 16384 texels on a side is snapshotted in regions.
 *   inside      a texel is inside iff its stored (premultiplied) code of `channel`, a crh_channel, is >= `threshold`, 1..255:
 *               crh_distance's definition.
 *   statistics  histogram[256 * c + v], c = 0..3 for r, g, b, a, is the number of texels whose stored code of channel c is v, over all
 *               texels, whatever the channel and the threshold: [r, g, b, a][code] as one array of 1024, and each channel's 256 counts sum
 *               to width * height (16384^2 < 2^32: 32 bits hold every count). [x0, x1) x [y0, y1) is the smallest rectangle that holds
 *               every texel inside, 0, 0, 0, 0 if none is; count is the number of texels inside, which is also the sum of the channel's
 *               histogram from `threshold` up.
 * Hence: the statistics of a crop to the bounds have the bounds (0, 0, x1 - x0, y1 - y0) and the same count; a crop at (a, b) of a crop
 * at (x, y) whose rectangle lies inside the first result is the crop at (x + a, y + b); the statistics of a crop that misses the source
 * are width * height in bin 0 of each channel and no bounds.
 * crh_crop_texels and crh_statistics_texels (the rules on whole images in host memory, width * height * 4 bytes in the order r g b a at
 * any alignment, row 0 first; the crop writes out_width * out_height * 4) are host only: no renderer, no device.
 * Every error is found before the device is touched, and a refused call writes nothing and leaves *out and the out buffers untouched:
 * first a null argument; then a channel above CRH_CHANNEL_A; then a threshold outside [1, 255]; then a size (the source's, the result's,
 * the region's) outside [1, 16384]; then, in crh_crop_texels, an out_rgba8 equal to rgba8 are CRH_ERR_INVALID_ARGUMENT, each with a
 * crh_last_error text "crh_crop_texels: ..." (the three crops) or "crh_statistics_texels: ..." (the two statistics); then what
 * crh_image_create_from_frame refuses of a frame is CRH_ERR_UNSUPPORTED.
 * crh_image_crop and crh_image_create_from_frame_region run k_image_crop on the renderer's stream, which writes every texel of the result
 * once, zeros included, and allocate nothing but the result. crh_image_statistics runs k_image_stats, which leaves a partial result
 * per workgroup in the call's one scratch allocation (no workgroup waits for another), and k_image_stats_merge, which sums them; the 4116
 * bytes are then copied to the host. All three are synchronous, like their siblings; only level 0 of the source is read and the source
 * is not modified. A failed allocation or launch frees everything, writes nothing to *out and returns CRH_ERR_HIP.
 * Limits: the calls are synchronous and none works in place; the statistics of a frame need a snapshot first; the bounds are one
 * rectangle, not one per connected component; the histogram is of the stored codes, premultiplied as they are. */
typedef struct crh_image_stats {
    uint32_t histogram[1024];   /* [r, g, b, a][code] as uint32_t[4][256]: entry 256 * c + v = how many texels store code v in channel c */
    uint32_t x0, y0, x1, y1;    /* half-open: the smallest rectangle that holds every texel inside; 0, 0, 0, 0 if none is */
    uint32_t count;             /* texels inside */
} crh_image_stats;
crh_status crh_crop_texels(uint32_t width, uint32_t height, const void* rgba8, int32_t x, int32_t y, uint32_t out_width, uint32_t out_height, void* out_rgba8); /* host only */
crh_status crh_statistics_texels(uint32_t width, uint32_t height, const void* rgba8, uint32_t channel, uint32_t threshold, crh_image_stats* out);                /* host only */
crh_status crh_image_crop(const crh_image* src, int32_t x, int32_t y, uint32_t width, uint32_t height, crh_image** out);
crh_status crh_image_create_from_frame_region(crh_frame* frame, int32_t x, int32_t y, uint32_t width, uint32_t height, crh_image** out);
crh_status crh_image_statistics(const crh_image* src, uint32_t channel, uint32_t threshold, crh_image_stats* out);
/* Variable blur: crh_image_blur with a strength that changes across the image — a progressive backdrop blur under a bar, tilt-shift,
 * depth of field from a depth layer, a soft vignette, focus on one widget. A second image of the source's size, the mask, gives every
 * texel a level, and the level chooses the texel's own taps. Integer and bit-exact like the blur, of which it is the general case.
 *   level        u(i, j) = the stored code of how->channel (a crh_channel) of mask texel (i, j), 0 <= u <= 255, as it is: no
 *                unpremultiply, as crh_image_distance_field reads its channel. The mask has the source's size and is read at the
 *                output's own (i, j); no edge rule applies to it.
 *   sigma        per axis, with s0 = sigma[0] (at code 0) and s1 = sigma[1] (at code 255), each in [0, CRH_MAX_BLUR_SIGMA]: u == 0 gives
 *                s0 and u == 255 gives s1, the caller's floats exactly; any other u gives
 *                (float)((double)s0 + ((double)s1 - (double)s0) * (double)u / 255.0), evaluated in that order. s0 > s1 is legal.
 *   taps         exactly crh_blur_taps(sigma of the level): R_u, q_u[0 .. R_u]. There is no second tap rule.
 *   horizontal   with u = u(i, j): t(i, j) = (sum_{k = -Rx_u .. Rx_u} qx_u[|k|] c(i + k, j) + 128) >> 8 per channel, c the source under `edge`.
 *   vertical     with u = u(i, j): out(i, j) = (sum_{k = -Ry_u .. Ry_u} qy_u[|k|] t(i, j + k) + 2^23) >> 24. t <= 65280, the sum < 2^32.
 *   edge         a crh_blur_edge: what the SOURCE is outside itself. PAD, REPEAT and REFLECT wrap a source index in the horizontal pass
 *                and a row index of t in the vertical pass by exactly the blur's wrap(i, n); TRANSPARENT takes what lies outside as
 *                zero. The result has the source's size under EVERY edge, origin (0, 0), as crh_image_convolve keeps it: with growth
 *                the mask would need an edge rule of its own. A caller who wants the spill takes a larger crh_image_crop of the
 *                source and of the mask first, which pads with zeros.
 * Hence: (1) a mask whose chosen channel is one value u everywhere gives, byte for byte, crh_image_blur(src, sigma_x(u), sigma_y(u), edge)
 * under PAD, REPEAT and REFLECT, and under TRANSPARENT that blur's result cropped to (Rx, Ry, w, h); (2) a texel whose level has sigma 0
 * on both axes comes back exactly, whatever its neighbours' levels are (t = 256 c, then (65536 * 256 c + 2^23) >> 24 = c); (3) a constant
 * image comes back exactly under the three same-size edges, because every tap set sums to 65536; (4) rgb <= a survives, because one
 * texel's four channels share its weights and both roundings are monotone; (5) the result does not depend on which of sigma[0] and
 * sigma[1] is the larger beyond what the formula says: a descending ramp over the inverted mask is the ascending one wherever the two
 * formulas give one float.
 * crh_variable_blur_validate, crh_variable_blur_sigma (the two sigmas of one code <= 255, as crh_blur_taps hands out taps; a code above
 * 255 is CRH_ERR_INVALID_ARGUMENT) and crh_variable_blur_texels (the rule on whole images in host memory, width * height * 4 bytes each in
 * the order r g b a at any alignment, row 0 first) are host only: no renderer, no device.
 * Every error is found before the device is touched, and a refused call writes nothing and leaves *out and the out buffer untouched:
 * first a null argument; then a sigma that is not finite (CRH_ERR_NON_FINITE); then a sigma that is negative or above
 * CRH_MAX_BLUR_SIGMA; then a channel above CRH_CHANNEL_A; then an edge above CRH_BLUR_EDGE_REFLECT; then a size outside [1, 16384];
 * then, in crh_variable_blur_texels, an out_rgba8 equal to either input; then, in crh_image_variable_blur, a mask of another size than
 * the source, then images of different renderers: CRH_ERR_INVALID_ARGUMENT but for the one named, each with a crh_last_error text
 * "crh_variable_blur_validate: ...". mask == src is legal.
 * crh_image_variable_blur builds the 256 tap sets of each axis on the host (consecutive levels of one sigma share a set), uploads them
 * with a 256-entry table of (offset, radius) per axis at the head of the one scratch allocation that also holds the 16-bit intermediate,
 * and runs k_image_variable_blur_h and k_image_variable_blur_v on the renderer's stream: the blur's geometry, an apron of the call's
 * largest radius, every lane summing over its own level's taps; a wave whose lanes share one level reads its taps as the blur does.
 * The result has one level (crh_image_generate_mipmaps works on it); only level 0 of the source and of the mask is read and neither is
 * modified. A failed allocation or launch frees everything, writes nothing to *out and returns CRH_ERR_HIP.
 * Limits: this is a gather — each output picks its own kernel, the form every UI toolkit ships — not the scatter a physical lens gives;
 * the profile between the two sigmas is linear in the code: any other profile is a crh_image_color_filter table on the mask first; the
 * call is synchronous, like its siblings. */
typedef struct crh_variable_blur {
    float sigma_x[2];   /* the x sigma at mask code 0 and at mask code 255, each in [0, CRH_MAX_BLUR_SIGMA] */
    float sigma_y[2];   /* the same for y */
    uint32_t channel;   /* crh_channel: which STORED code of the mask's texel is the level */
    uint32_t edge;      /* crh_blur_edge: what the SOURCE is outside itself */
} crh_variable_blur;
crh_status crh_variable_blur_validate(const crh_variable_blur* how);                                                          /* host only */
crh_status crh_variable_blur_sigma(const crh_variable_blur* how, uint32_t code, float* sigma_x, float* sigma_y);              /* host only */
crh_status crh_variable_blur_texels(uint32_t width, uint32_t height, const void* rgba8, const void* mask_rgba8, const crh_variable_blur* how, void* out_rgba8); /* host only: the rule */
crh_status crh_image_variable_blur(const crh_image* src, const crh_image* mask, const crh_variable_blur* how, crh_image** out);
/* Transform: a new image that is `src` seen through a 3 x 3 matrix — rotate, skew or tilt a layer (CSS transform, Canvas drawImage under a
 * matrix, a card flip) in one call, with a result of any size, three filters and the four edges. The matrix maps RESULT coordinates to
 * SOURCE coordinates (no inverse is taken; a singular matrix is legal), texel (i, j) covering [i, i + 1) x [j, j + 1).
 * All real arithmetic below is IEEE binary64, exactly in the written order and parenthesisation, with no contraction, and uses only
 * + * /, comparisons and floor; everything behind X and Y is integer. The tests check every byte.
 *   position  of result texel (i, j): u = i + 0.5, v = j + 0.5; xs = (m0 u + m1 v) + m2, ys = (m3 u + m4 v) + m5, ws = (m6 u + m7 v) + m8.
 *             The call is AFFINE when m6 == 0 && m7 == 0 && m8 == 1: then px = xs, py = ys. Otherwise a texel with !(ws > 0) is NOT
 *             VISIBLE — its result is (0, 0, 0, 0) under every edge (it lies behind the horizon) — and for the others px = xs / ws,
 *             py = ys / ws. Clamp by comparisons: p = p < -2097152 ? -2097152 : p > 2097152 ? 2097152 : p. With |m| <= 2^40 and
 *             u, v < 2^15 every sum is finite, so no NaN can arise, and an infinite quotient clamps. X = (int32) floor(px * 256 + 0.5),
 *             Y likewise: |X|, |Y| <= 2^29, in units of 1/256 texel. crh_transform_position hands out exactly these (visible 0 or 1;
 *             the position of an invisible texel is (0, 0)).
 *   NEAREST   and LINEAR: the value is crh_image_displace's NEAREST and LINEAR of the position (X, Y): S(X >> 8, Y >> 8), or the
 *             2 x 2 blend around (X - 128, Y - 128) with one rounding. One function serves both calls.
 *   CUBIC     Catmull-Rom over 4 x 4 texels. ax = X - 128, i0 = ax >> 8, F = ax & 255, the y axis the same. Exact integer weights over
 *             2^25: W0 = -F^3 + 512 F^2 - 65536 F, W2 = -3 F^3 + 1024 F^2 + 65536 F, W3 = F^3 - 256 F^2, W1 = 2^25 - W0 - W2 - W3;
 *             c_k = (W_k + 1024) >> 11 (arithmetic) for k = 0, 2, 3 and c_1 = 16384 - c_0 - c_2 - c_3, a 256 x 4 table that is a
 *             constant of the library. Per channel and footprint row r = j0 - 1 .. j0 + 2:
 *             h_r = (sum_k c_k(Fx) S(i0 - 1 + k, r) + 32) >> 6, then value = clamp((sum_r c_r(Fy) h_r + 2^21) >> 22, 0, 255), and at
 *             the end rgb = min(rgb, a), as crh_image_resize does, because negative lobes do not keep rgb <= a. Over all 256 phases:
 *             -1214 <= c_k <= 16384; the positive weights of a phase sum to at most 18432 and the negative ones to at most 2048 in
 *             magnitude; -8161 <= h <= 73440; the second numerator is at most 1 372 456 960 < 2^31 in magnitude; a constant image
 *             comes back exactly at every phase pair.
 *   S(i, j)   crh_image_displace's S: the source's codes as they are, with no load clamp. Under PAD, REPEAT and REFLECT each index goes
 *             separately through the image-paint block's wrap(i, n), any number of periods out; under TRANSPARENT the value is
 *             (0, 0, 0, 0) when either index is outside. Every address is formed from a wrapped or tested index only.
 * Hence: the identity at the source's size is a byte-for-byte copy under NEAREST and LINEAR and every edge, and under CUBIC a copy of a
 * premultiplied source (F = 0 gives c = (0, 16384, 0, 0), and only min(rgb, a) can change a texel); an integer translation under
 * TRANSPARENT is crh_image_crop's bytes; a quarter turn (entries 0 and +-1 and an integer offset) is an exact permutation of the texels
 * under all three filters; rgb <= a survives every filter for a premultiplied source; an all-zero linear part reads one point.
 * crh_transform_fit is the call for "rotate this layer by 30 degrees and keep all of it": `forward` maps SOURCE coordinates to the caller's
 * target space, and the call writes to *out the result size and the result -> source matrix of the smallest result that holds the
 * whole source, and to `origin` where the target space's (0, 0) lies in that result (blur's and crop's convention). In binary64, in
 * this order, with (a b c; d e f; g h i) = forward: each corner (x, y) of (0, 0), (w, 0), (0, h), (w, h) gives X = (a x + b y) + c,
 * Y = (d x + e y) + f, W = (g x + h y) + i; an affine forward (g == 0 && h == 0 && i == 1) takes (X, Y), any other refuses
 * "a corner is behind the horizon" when !(W > 0) and takes (X / W, Y / W). x0 = floor(min x), x1 = ceil(max x), y likewise; the size is
 * max(1, x1 - x0) by max(1, y1 - y0), refused as "the result is outside [1, 16384]" when it exceeds 16384 or is not finite, and
 * "the origin is beyond 2^30" when |x0| or |y0| is; origin = (-x0, -y0). The adjugate, entry by entry:
 *   A0 = e i - f h   A1 = c h - b i   A2 = b f - c e
 *   A3 = f g - d i   A4 = a i - c g   A5 = c d - a f
 *   A6 = d h - e g   A7 = b g - a h   A8 = a e - b d          det = (a A0 + b A3) + c A6
 * "forward is singular" when det == 0 or a quotient n_k = A_k / det is not finite. The matrix is n composed with the translation by
 * (x0, y0): entries 0, 1, 3, 4, 6, 7 are n's, and m2 = (n0 x0 + n1 y0) + n2, m5 = (n3 x0 + n4 y0) + n5, m8 = (n6 x0 + n7 y0) + n8; it
 * is then validated like any other. An affine forward gives A6 = A7 = 0 and A8 = det, so the last row is exactly (0, 0, 1) and the
 * call takes the affine path.
 * crh_transform_validate, _fit, _position and crh_transform_texels (the rule on whole images in host memory: width * height * 4 bytes
 * of the source in the order r g b a at any alignment, row 0 first, to how->width * how->height * 4 bytes) are host only: no renderer,
 * no device.
 * Every error is found before the device is touched, and a refused call writes nothing and leaves *out untouched, in this order: a null
 * argument is CRH_ERR_INVALID_ARGUMENT; then a filter above CRH_TRANSFORM_CUBIC or an edge above CRH_BLUR_EDGE_REFLECT; then a non-finite
 * entry is CRH_ERR_NON_FINITE; then an entry above CRH_MAX_TRANSFORM_ENTRY in magnitude, a result size (and the source's) outside
 * [1, 16384], a texel outside the result in crh_transform_position, and out_rgba8 equal to the input in crh_transform_texels are
 * CRH_ERR_INVALID_ARGUMENT, each with a crh_last_error text "crh_transform_validate: ...". crh_transform_fit checks `forward` by the same
 * rows before its own refusals.
 * crh_image_transform runs k_image_transform on the renderer's stream, specialised on the filter, on TRANSPARENT against the wrapping
 * edges and on affine against projective; it allocates nothing but the result, which has one level (crh_image_generate_mipmaps works on
 * it) and origin (0, 0); only level 0 of the source is read and it is not modified. A failed allocation or launch frees everything and
 * returns CRH_ERR_HIP.
 * Limits: no prefilter — a minification beyond about 2 x aliases: crh_image_resize or crh_image_generate_mipmaps first; the call is
 * synchronous, like its siblings; the codes are used as they are, with no gamma handling; this is not a per-draw effect of the raster
 * path. */
typedef enum crh_transform_filter { CRH_TRANSFORM_NEAREST = 0, CRH_TRANSFORM_LINEAR = 1, CRH_TRANSFORM_CUBIC = 2 } crh_transform_filter;
#define CRH_MAX_TRANSFORM_ENTRY 1099511627776.0 /* 2^40 */
typedef struct crh_transform {
    double matrix[9];       /* row-major 3 x 3: RESULT coordinates (x, y, 1) -> SOURCE coordinates; finite, |.| <= 2^40 */
    uint32_t width, height; /* of the result, each in [1, 16384] */
    uint32_t filter;        /* crh_transform_filter */
    uint32_t edge;          /* crh_blur_edge: what the source is outside itself */
} crh_transform;
crh_status crh_transform_validate(const crh_transform* how);                                   /* host only */
crh_status crh_transform_fit(uint32_t width, uint32_t height, const double forward[9], uint32_t filter, uint32_t edge,
                             crh_transform* out, int32_t origin[2]);                          /* host only */
crh_status crh_transform_position(const crh_transform* how, uint32_t i, uint32_t j, int32_t position[2], uint32_t* visible); /* host only */
crh_status crh_transform_texels(uint32_t width, uint32_t height, const void* rgba8, const crh_transform* how, void* out_rgba8); /* host only */
crh_status crh_image_transform(const crh_image* src, const crh_transform* how, crh_image** out);
typedef struct crh_image_paint {
    const crh_image* image;
    uint32_t filter;             /* CRH_FILTER_NEAREST or _LINEAR, optionally | CRH_FILTER_MIPMAP */
    uint32_t spread_x, spread_y; /* crh_spread, per axis */
    float m[6];                  /* path -> texel: u = m0 x + m1 y + m2, v = m3 x + m4 y + m5 */
} crh_image_paint;
crh_status crh_image_paint_validate(const crh_image_paint* paint); /* host only: needs no renderer and no device */
crh_status crh_scene_set_paints_with_images(crh_scene* scene, const crh_paint* paints, uint32_t n_paints, const crh_image_paint* image_paints,
                                            uint32_t n_image_paints, const int32_t* instance_paint, uint32_t n_instances);

/* LoadOp::Load of caller content: `rgba8` = width*height*4 bytes of premultiplied RGBA8, row 0 = top, replace the frame's pixels; every
 * sample of a pixel starts from its value. The stencil attachment, the saved alpha layers and the pass state are reset as by
 * crh_frame_clear, the depth attachment is left alone. The frame is NOT cleared afterwards: the next pass loads these pixels. Ordered
 * behind the last pass into the frame; the host bytes are copied before the call returns. CRH_ERR_INVALID_ARGUMENT for a
 * CRH_FORMAT_RGBA16F frame and for a frame restricted by crh_frame_set_tile_rows. */
crh_status crh_frame_upload(crh_frame* frame, const void* rgba8);
/* LoadOp::Load of an image: crh_frame_upload with the bytes taken from level 0 of `image` on the device — how a composed layer comes back
 * into a frame without a round trip through the host. The same ordering, the same reset of stencil, alpha layers and pass state, the same
 * frames refused; the call returns when the copy is done, so the image may be destroyed afterwards. An image of another size or of another
 * renderer is CRH_ERR_INVALID_ARGUMENT. */
crh_status crh_frame_load_image(crh_frame* frame, const crh_image* image);
/* MSAA resolve (box average, examples/showcase/main.rs:215) + copy to host, `rgba8` = width*height*4 bytes, row 0 = top. */
crh_status crh_frame_download(crh_frame* frame, void* rgba8);
/* The same for a CRH_FORMAT_RGBA16F frame: width*height*8 bytes (four IEEE binary16 per pixel). Each entry point refuses the other format. */
crh_status crh_frame_download_f16(crh_frame* frame, void* rgba16f);
/* Device pointer of the resolved RGBA8 image (for the RCCL tile exchange); valid until the frame is destroyed. */
crh_status crh_frame_device_pointer(crh_frame* frame, void** rgba8_dev);
/* Ordered premultiplied "over" of n_layers RGBA8 images that live in HBM: dst = layers[0] under layers[1] ....
 * Runs on a stream of its own and returns when dst is complete, without waiting for renders in flight. */
crh_status crh_composite_over(crh_renderer* renderer, const void* const* layers_dev, uint32_t n_layers, uint64_t n_pixels, void* dst_dev);

/* ---- stream plumbing ------------------------------------------------------------------------------- */
crh_status crh_renderer_synchronize(crh_renderer* renderer);
/* Blocks the host until the last render INTO THIS FRAME has finished; work queued afterwards (the next frame of a double-buffered
 * loop) keeps running. The resolved image behind crh_frame_device_pointer is then complete (a frame whose tile lists turned out too
 * small is rendered again here, which waits for everything in flight — once, while the capacities are being learned). */
crh_status crh_frame_synchronize(crh_frame* frame);
/* hipStream_t of the renderer, as void* (for HIP events in bench.py). */
void* crh_renderer_stream(crh_renderer* renderer);
/* Milliseconds spent by the last crh_scene_tessellate / crh_scene_render* on the GPU, per kernel,
 * measured with HIP events on the renderer's streams when timing is enabled. enabled = 1: every kernel of a step (a dozen events per
 * step: they cost a pipelined loop about 4 % of its rate); 2: the kernels of the raster lane only (two events per step); 0: off. */
crh_status crh_renderer_enable_timing(crh_renderer* renderer, int enabled);
typedef struct crh_kernel_time {
    char name[48];
    float ms;
    uint64_t algorithmic_bytes;
} crh_kernel_time;
crh_status crh_renderer_kernel_times(crh_renderer* renderer, crh_kernel_time* out, uint32_t capacity, uint32_t* count);
/* Self-test tap: evaluates include/crh_fmath.h ON THE GPU (fn 0 atan2(a,b), 1 acos(a), 2 sin(a), 3 cos(a), 4 pow(a,b), 5 wgsl_mod(a,b)),
 * and fn 10 csrc/paint_angle.hpp paint_turns(a,b), so that tests can check device results bit for bit against the host evaluation of the same header. Host pointers. */
crh_status crh_selftest_fmath(crh_renderer* renderer, int fn, const float* a, const float* b, float* out, uint64_t n);
/* Self-test tap of the sRGB codec of the *_SRGB formats, run ON THE GPU by the functions the raster kernels use: codes[i] = encode(x[i]) for
 * i < n, decoded[c] = decode(c) for the 256 codes (both as defined at CRH_FORMAT_RGBA8_SRGB above). Host pointers. */
crh_status crh_selftest_srgb(crh_renderer* renderer, const float* x, uint8_t* codes, uint64_t n, float* decoded);
/* ---- glyph producer: text.rs (config 3 input) ----------------------------------------------------
 * Host-side code (the reference's is host-side too). The TrueType reading is done by the crate
 * ttf-parser 0.14.0 in the reference (Cargo.toml:20, not vendored); src/csrc/text.cpp restates the
 * published TrueType `glyf` outline walk and the tables text.rs queries. */
typedef struct crh_font crh_font;           /* Font, text.rs:11-38 (ttf_parser::Face over owned bytes) */
typedef struct crh_path_list crh_path_list; /* Vec<Path>, as returned by text.rs:97 and :236 */

/* Font::new, text.rs:19-27. The bytes are copied. CRH_ERR_INVALID_ARGUMENT when the face cannot be parsed (the reference unwrap()s). */
crh_status crh_font_create(const void* ttf_bytes, size_t n_bytes, crh_font** out);
void crh_font_destroy(crh_font* font);

/* The Face getters text.rs calls (text.rs:156-158, :209-211, :238); font units. */
typedef struct crh_font_metrics {
    uint32_t units_per_em;
    uint32_t number_of_glyphs;
    int32_t ascender, descender, line_gap, height; /* height = ascender - descender (Face::height) */
    int32_t has_x_height, x_height;                /* Face::x_height() -> Option */
    int32_t has_vertical_metrics, vertical_height, vertical_line_gap; /* Face::vertical_height() / vertical_line_gap() -> Option */
    int32_t has_kerning;                           /* first subtable of `kern` usable (text.rs:148) */
} crh_font_metrics;
crh_status crh_font_get_metrics(const crh_font* font, crh_font_metrics* out);
/* Face::glyph_index (text.rs:147,181): *found = 0 when no Unicode cmap subtable maps the code point. */
crh_status crh_font_glyph_index(const crh_font* font, uint32_t code_point, uint16_t* glyph_id, uint32_t* found);
/* Face::glyph_hor_advance / glyph_ver_advance (text.rs:189-191) */
crh_status crh_font_glyph_advance(const crh_font* font, uint16_t glyph_id, uint32_t vertical, uint16_t* advance, uint32_t* found);
/* Face::glyph_bounding_box (text.rs:244): x_min y_min x_max y_max */
crh_status crh_font_glyph_bounding_box(const crh_font* font, uint16_t glyph_id, int16_t box[4], uint32_t* found);
/* kerning_table.glyphs_kerning(left, right) (text.rs:183) */
crh_status crh_font_glyphs_kerning(const crh_font* font, uint16_t left, uint16_t right, int16_t* kerning, uint32_t* found);

/* Orientation text.rs:106-117, Alignment :119-131 (declaration order) */
enum { CRH_ORIENTATION_RIGHT_TO_LEFT = 0, CRH_ORIENTATION_LEFT_TO_RIGHT = 1, CRH_ORIENTATION_TOP_TO_BOTTOM = 2, CRH_ORIENTATION_BOTTOM_TO_TOP = 3 };
enum { CRH_ALIGNMENT_BEGIN = 0, CRH_ALIGNMENT_BASELINE = 1, CRH_ALIGNMENT_CENTER = 2, CRH_ALIGNMENT_END = 3 };
/* Layout, text.rs:133-143 */
typedef struct crh_text_layout {
    float size;
    uint32_t orientation;     /* CRH_ORIENTATION_* */
    uint32_t major_alignment; /* CRH_ALIGNMENT_* */
    uint32_t minor_alignment; /* CRH_ALIGNMENT_* */
} crh_text_layout;

/* paths_of_glyph, text.rs:97-104: one Path per contour, no stroke options; an empty list for glyphs without outline. */
crh_status crh_paths_of_glyph(const crh_font* font, uint16_t glyph_id, crh_path_list** out);
/* paths_of_text, text.rs:236-263. `text` = Unicode scalar values (Rust chars); `clipping_area` = n_clip (x, y) pairs of a convex
 * polygon in clockwise order (utils.rs:83-98) or NULL. */
crh_status crh_paths_of_text(const crh_font* font, const crh_text_layout* layout, const uint32_t* text, size_t n_chars, const float* clipping_area,
                             size_t n_clip, crh_path_list** out);
/* calculate_aligned_positions!, text.rs:145-230 (integer font units): `positions` receives, line by line, one (x, y, glyph_id) triple of
 * int64 per character plus one terminating entry per line (the '\n' or the end of the text, glyph id 0), i.e. n_chars + 1 triples in
 * total; line_ends[l] = the reference's `line_range_end` (text.rs:169,199). Pass NULL pointers to query *n_lines only. */
crh_status crh_text_aligned_positions(const crh_font* font, const crh_text_layout* layout, const uint32_t* text, size_t n_chars, int64_t extent[2],
                                      int64_t offset[2], int64_t* positions /* [n_chars + 1][3] */, uint64_t* line_ends, uint64_t* line_lengths,
                                      uint64_t* n_lines);
/* Path::push_elliptical_arc, path.rs:639-708 (the SVG "arc to" command): the rational quadratic segments that continue a path whose
 * current end point is `from`. `records` receives n_segments x {weight, tangent_crossing.xy, vertex.xy} (the record layout of
 * CRH_SEGMENT_RATIONAL_QUADRATIC); *is_line = 1 when a radius is zero and the reference pushes a plain line to `to` instead.
 * Call with records == NULL to query *n_segments (at most 3). Host code. */
crh_status crh_path_elliptical_arc(const float from[2], const float half_extent[2], float rotation, uint32_t large_arc, uint32_t sweep, const float to[2],
                                   float* records, uint32_t capacity, uint32_t* n_segments, uint32_t* is_line);
/* Path::transform(scale, &motor), path.rs:387-439, on every path of the list. motor = ppga2d::Motor [scalar, e12, e01, e02]
 * (utils.rs:122-129: rotate2d, translate2d). */
crh_status crh_path_list_transform(crh_path_list* list, float scale, const float motor[4]);
/* Views the list as one Shape, all paths filled, in crh_path_batch form; the pointers stay valid until the list is changed or destroyed. */
crh_status crh_path_list_view(const crh_path_list* list, crh_path_batch* out);
void crh_path_list_destroy(crh_path_list* list);

/* ---- multi-GPU: path-index sharding + the framebuffer exchange ---------------------------------------
 * The reference is single-GPU (no such component upstream); this group is the exchange step of SURVEY.md §8(e) behind
 * the C ABI, so that a host in any language can shard: one process per GPU, rank g renders Shapes crh_comm_shard(n, g, world) into a
 * private full-size layer (a crh_frame), crh_frame_exchange composites the layers in rank order — premultiplied "over", lower rank
 * underneath — and leaves the image in rank 0's `result` frame. Only 16x16 tiles that hold something travel (occupancy bitmaps are
 * all-gathered first); transfers are grouped ncclSend / ncclRecv of row slabs over RCCL (the librccl the process has already mapped —
 * e.g. the one bundled with torch — or librccl.so, opened on first use).
 * Layers may be RGBA8 frames (<= 2/255 per channel against a single-GPU render of the whole scene) or CRH_FORMAT_RGBA16F frames
 * (<= 1/255: one RGBA8 quantisation, in the composite); all ranks use the same format, the result frame is RGBA8.
 * A rank whose layer cannot be read (a failed pass) still takes part in the collective and every rank returns an error together. */
typedef struct crh_comm crh_comm;
#define CRH_COMM_ID_BYTES 128 /* ncclUniqueId */
/* contiguous, order-preserving split of [0, n_items): sizes differ by at most one */
crh_status crh_comm_shard(uint32_t n_items, uint32_t rank, uint32_t world, uint32_t* begin, uint32_t* end);
/* the pixel rows of rank `rank`'s slab of a frame `height` pixels high (whole 16-pixel tile rows) */
crh_status crh_comm_slab_rows(uint32_t height, uint32_t rank, uint32_t world, uint32_t* row_begin, uint32_t* row_end);
/* rank 0 calls this and hands the 128 bytes to the other ranks by any means (ncclGetUniqueId) */
crh_status crh_comm_unique_id(void* id128);
/* collective over all ranks (ncclCommInitRank); the renderer names the device. CRH_ERR_UNSUPPORTED when RCCL cannot be loaded. */
crh_status crh_comm_create(crh_renderer* renderer, uint32_t rank, uint32_t world, const void* id128, crh_comm** out);
void crh_comm_destroy(crh_comm* comm);
/* collective: `layer` = this rank's frame; `result` = the frame that receives the image on rank 0, NULL on every other rank.
 * Waits for the last pass into `layer` only; runs on a stream of its own, so the renderer may already be drawing the next step.
 * `result` may be one of the layers (here and in crh_comm_local_exchange, at any rank): the image is the composite of the layers as they
 * were when the call was made, and the frame shows it afterwards. */
crh_status crh_frame_exchange(crh_comm* comm, crh_frame* layer, crh_frame* result);
/* The other split of SURVEY.md §8(e) — shard by TILE instead of by path index (no such component upstream either; it mirrors what a wgpu
 * scissor rectangle on renderer.rs:267-355's passes would do): the passes into `frame` draw the tile rows that cover the pixel rows
 * [row_begin, row_end) only (multiples of 16, or the frame's height; crh_comm_slab_rows gives rank g's), the rest of the frame is and stays
 * transparent. Every rank uploads, tessellates and bins ALL paths and draws 1 / world of the tiles; crh_frame_exchange of such layers
 * moves nothing in its all-to-all, composites nothing, and gathers an image that is bit-equal to a single GPU's (path sharding with RGBA8
 * layers: <= 2/255). (0, height) gives the whole frame back. Waits for the frame's last pass. A LoadOp::Clear of the pixels, the stencil
 * attachment and the alpha layers: the frame keeps no pass state afterwards (as after crh_frame_clear); the depth attachment is left alone. */
crh_status crh_frame_set_tile_rows(crh_frame* frame, uint32_t row_begin, uint32_t row_end);
/* collective, the tile split's own exchange: every rank's `layer` holds its slab of rows (crh_frame_set_tile_rows with crh_comm_slab_rows' rows)
 * and the slabs travel straight from the layers' pixel rows into rank 0's `result` frame (NULL elsewhere): one grouped ncclSend / ncclRecv
 * per rank, no bitmaps, packing, plan, composite or unpacking. RGBA8 storage on both sides, frames of one size on every rank (checked).
 * crh_comm_last_timing then reports the transfer under [4], crh_comm_last_traffic the slab's bytes. */
crh_status crh_frame_gather_slabs(crh_comm* comm, crh_frame* layer, crh_frame* result);
/* bytes this rank sent in the last exchange, and what dense slabs (no empty-tile suppression) would have been */
crh_status crh_comm_last_traffic(const crh_comm* comm, uint64_t* bytes_sent, uint64_t* bytes_dense);
/* GPU time of the phases of this rank's last exchange, in milliseconds (HIP events on the communicator's stream; waits for the exchange):
 * [0] occupancy bitmap + packing of the non-empty tiles, [1] all-gather of the bitmaps + their prefix sums, [2] all-to-all of the slab
 * tiles, [3] ordered composite of the slab, [4] gather of the composited tiles on rank 0, [5] unpacking into the result frame (rank 0). */
#define CRH_COMM_PHASES 6
crh_status crh_comm_last_timing(crh_comm* comm, float ms[CRH_COMM_PHASES]);
/* bytes this rank sent to every peer in the all-to-all of the last exchange: per_peer[world] (its own entry is 0) */
crh_status crh_comm_last_peer_bytes(const crh_comm* comm, uint64_t* per_peer);
/* What the transport says about this communicator: *nranks = ncclCommCount of an RCCL communicator (the size of the loopback group for a
 * local one), *rccl_version = ncclGetVersion's code (major * 10000 + minor * 100 + patch; 0 for a local communicator). A line of a
 * multi-GPU measurement carries both, so that "did RCCL see N ranks" is answered by RCCL. */
crh_status crh_comm_info(const crh_comm* comm, uint32_t* nranks, int32_t* rccl_version);
/* The same exchange without RCCL, for several communicators on ONE device driven by one thread (tests, single-GPU validation):
 * rank 0's communicator founds the group (rank0 = NULL), ranks 1.. join it; crh_comm_local_exchange(rank 0's comm, layers[world],
 * result) then runs every rank's part with device-to-device copies in place of the transfers. */
crh_status crh_comm_create_local(crh_renderer* renderer, uint32_t rank, uint32_t world, crh_comm* rank0, crh_comm** out);
crh_status crh_comm_local_exchange(crh_comm* rank0, crh_frame* const* layers, crh_frame* result);
crh_status crh_comm_local_gather_slabs(crh_comm* rank0, crh_frame* const* layers, crh_frame* result); /* crh_frame_gather_slabs over the loopback group */

const char* crh_last_error(void);
const char* crh_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CONTRAST_HIP_H */
