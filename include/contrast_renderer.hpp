// contrast_renderer.hpp — header-only C++17 host mirror of the reference's public API for the hot path, over the C ABI of
// contrast_hip.h: the same type and function names, argument order, ownership and error behaviour as the Rust crate
// (Lichtso/contrast_renderer v0.1.4, citations relative to its tree), so that code written against
//     contrast_renderer::path::{Path, StrokeOptions, DynamicStrokeOptions, ...}          (src/path.rs)
//     contrast_renderer::renderer::{Configuration, Renderer, Shape, RenderOperation}     (src/renderer.rs)
//     contrast_renderer::text::{Font, Layout, paths_of_glyph, paths_of_text}             (src/text.rs)
// reads the same here. wgpu's Device / Queue / RenderPass become HIP-backed handles (a device ordinal, a Frame and a recorded
// RenderPass). Errors: Result<_, Error> becomes `throw Error` with the reference's variants (error.rs:5-16) in `Error::status`; the
// reference's panics (non-finite input, degenerate cubic) surface as status 6 / 7 instead of aborting the process.
//
// The Rust toolchain is absent from the build image, so this C++ mirror (and the ctypes one in contrast_renderer_amd/) is what the
// tests drive; INTEGRATION.md shows the equivalent Rust shim.
#pragma once
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "contrast_hip.h"

namespace contrast_renderer {

// ---------------------------------------------------------------------------------------------- error.rs
struct Error : std::runtime_error {
    crh_status status;
    explicit Error(crh_status s) : std::runtime_error(describe(s)), status(s) {}
    static std::string describe(crh_status s) {
        static const char* names[] = {"Ok", "NumberOfStencilBitsIsUnsupported", "ClipStackOverflow", "TooManyNestedOpacityGroups", "TooManyDashIntervals",
                                      "DynamicStrokeOptionsIndexOutOfBounds", "NonFinite (the reference panics: safe_float.rs:46)",
                                      "DegenerateCubic (the reference panics: fill.rs:174,178)", "Unsupported", "Hip", "InvalidArgument"};
        std::string text = s <= CRH_ERR_INVALID_ARGUMENT ? names[s] : "unknown";
        const char* detail = crh_last_error();
        if ((s == CRH_ERR_HIP || s == CRH_ERR_INVALID_ARGUMENT) && detail && *detail) text += std::string(": ") + detail;
        return text;
    }
};
inline void check(crh_status s) {
    if (s != CRH_OK) throw Error(s);
}

// ---------------------------------------------------------------------------------------------- safe_float.rs
// SafeFloat::from (safe_float.rs:44-52): finite or panic, -0.0 -> +0.0
inline float safe_float(float v) {
    if (!std::isfinite(v)) throw Error(CRH_ERR_NON_FINITE);
    return v == 0.0f ? 0.0f : v;
}
using Vec2 = std::pair<float, float>;

// ---------------------------------------------------------------------------------------------- path.rs
enum class SegmentType : uint8_t { Line = 0, IntegralQuadraticCurve = 1, IntegralCubicCurve = 2, RationalQuadraticCurve = 3, RationalCubicCurve = 4 }; // :56-67
enum class Join : uint32_t { Miter = 0, Bevel = 1, Round = 2 };                                                                                     // :71-82
enum class Cap : uint32_t { Square = 0, Round = 1, Out = 2, In = 3, Right = 4, Left = 5, Butt = 6 };                                               // :86-101

struct DashInterval { // path.rs:105-118
    float gap_start, gap_end;
    Cap dash_start, dash_end;
};

struct DynamicStrokeOptions { // path.rs:127-149: Dashed { join, pattern, phase } | Solid { join, start, end }
    bool dashed = false;
    Join join = Join::Miter;
    std::vector<DashInterval> pattern;
    float phase = 0.0f;
    Cap start = Cap::Butt, end = Cap::Butt;
    static DynamicStrokeOptions Dashed(Join join, std::vector<DashInterval> pattern, float phase) {
        DynamicStrokeOptions o;
        o.dashed = true;
        o.join = join;
        o.pattern = std::move(pattern);
        o.phase = safe_float(phase);
        return o;
    }
    static DynamicStrokeOptions Solid(Join join, Cap start, Cap end) {
        DynamicStrokeOptions o;
        o.join = join;
        o.start = start;
        o.end = end;
        return o;
    }
    crh_dynamic_stroke_options to_c() const {
        crh_dynamic_stroke_options c = {};
        c.dashed = dashed ? 1u : 0u;
        c.join = (uint32_t)join;
        c.pattern_len = (uint32_t)pattern.size(); // > 4 is reported by the library as TooManyDashIntervals, like renderer.rs:32-34
        for (size_t i = 0; i < pattern.size() && i < CRH_MAX_DASH_INTERVALS; ++i)
            c.pattern[i] = crh_dash_interval{safe_float(pattern[i].gap_start), safe_float(pattern[i].gap_end), (uint32_t)pattern[i].dash_start, (uint32_t)pattern[i].dash_end};
        c.phase = phase;
        c.start = (uint32_t)start;
        c.end = (uint32_t)end;
        return c;
    }
};

struct CurveApproximation { // path.rs:153-167
    bool uniform_tangent_angle = false;
    uint32_t steps = 1;
    float angle = 0.0f;
    static CurveApproximation UniformlySpacedParameters(uint32_t steps) { return CurveApproximation{false, steps, 0.0f}; }
    static CurveApproximation UniformTangentAngle(float angle) { return CurveApproximation{true, 0u, safe_float(angle)}; }
};

struct StrokeOptions { // path.rs:171-192
    float width = 1.0f, offset = 0.0f, miter_clip = 1.0f;
    bool closed = false;
    uint32_t dynamic_stroke_options_group = 0;
    CurveApproximation curve_approximation = CurveApproximation::UniformlySpacedParameters(1);
    void legalize() { // path.rs:196-200
        width = std::fabs(width);
        offset = std::fmin(std::fmax(offset, -0.5f), 0.5f);
        miter_clip = std::fabs(miter_clip);
    }
    crh_stroke_options to_c() const {
        crh_stroke_options c = {};
        c.width = safe_float(width);
        c.offset = safe_float(offset);
        c.miter_clip = safe_float(miter_clip);
        c.closed = closed ? 1u : 0u;
        c.dynamic_stroke_options_group = dynamic_stroke_options_group;
        c.curve_approximation = curve_approximation.uniform_tangent_angle ? CRH_CURVE_UNIFORM_TANGENT_ANGLE : CRH_CURVE_UNIFORMLY_SPACED_PARAMETERS;
        c.steps = curve_approximation.steps;
        c.angle_step = curve_approximation.angle;
        return c;
    }
};

// Path (path.rs:213-230). The five typed segment Vecs + segment_types of the reference are kept as one interleaved record list in
// segment order, which is what the SoA batch of the C ABI wants.
class Path {
  public:
    Vec2 start{0.0f, 0.0f};
    std::optional<StrokeOptions> stroke_options;
    std::vector<SegmentType> segment_types;
    std::vector<float> control; // per segment {2, 4, 6, 5, 10} floats, layouts of path.rs:15-52

    void push_line(Vec2 p) { // path.rs:234-237
        segment_types.push_back(SegmentType::Line);
        put(p);
    }
    void push_integral_quadratic_curve(Vec2 c0, Vec2 c1) { // path.rs:240-243
        segment_types.push_back(SegmentType::IntegralQuadraticCurve);
        put(c0), put(c1);
    }
    void push_integral_cubic_curve(Vec2 c0, Vec2 c1, Vec2 c2) { // path.rs:246-249
        segment_types.push_back(SegmentType::IntegralCubicCurve);
        put(c0), put(c1), put(c2);
    }
    void push_rational_quadratic_curve(float weight, Vec2 c0, Vec2 c1) { // path.rs:252-255
        segment_types.push_back(SegmentType::RationalQuadraticCurve);
        control.push_back(safe_float(weight));
        put(c0), put(c1);
    }
    void push_rational_cubic_curve(const float (&weights)[4], Vec2 c0, Vec2 c1, Vec2 c2) { // path.rs:258-261
        segment_types.push_back(SegmentType::RationalCubicCurve);
        for (float w : weights) control.push_back(safe_float(w));
        put(c0), put(c1), put(c2);
    }
    Vec2 get_end() const { return control.empty() ? start : Vec2{control[control.size() - 2], control[control.size() - 1]}; } // path.rs:266-290

    // ---- tangents (path.rs:296-372); Plane = (c, nx, ny)
    struct Plane {
        float c, nx, ny;
    };
    Plane get_start_tangent() const { // path.rs:296-322 — looks at segment_types.last() and the last segment of that type, as written there
        if (segment_types.empty()) return Plane{0.0f, 0.0f, 0.0f};
        const SegmentType last_type = segment_types.back();
        size_t at = 0, found = 0;
        for (size_t i = 0; i < segment_types.size(); ++i) {
            if (segment_types[i] == last_type) found = at;
            at += floats(segment_types[i]);
        }
        const size_t first_point = found + (last_type == SegmentType::RationalQuadraticCurve ? 1 : (last_type == SegmentType::RationalCubicCurve ? 4 : 0));
        return signum(tangent_from_points(start, Vec2{control[first_point], control[first_point + 1]}));
    }
    Plane get_end_tangent() const { // path.rs:326-372
        if (segment_types.empty()) return Plane{0.0f, 0.0f, 0.0f};
        const size_t n = control.size();
        if (segment_types.back() == SegmentType::Line) {
            const Vec2 previous = segment_types.size() > 1 ? Vec2{control[n - 4], control[n - 3]} : start;
            return signum(tangent_from_points(previous, Vec2{control[n - 2], control[n - 1]}));
        }
        return signum(tangent_from_points(Vec2{control[n - 4], control[n - 3]}, Vec2{control[n - 2], control[n - 1]}));
    }
    // path.rs:376-384 moves the typed segment Vecs of `other` but not its segment_types: nothing reachable is added (reproduced)
    void append(Path& other) {
        other.segment_types.clear();
        other.control.clear();
    }
    void reverse() { // path.rs:445-488
        std::vector<SegmentType> types;
        std::vector<std::vector<float>> records;
        Vec2 previous = start;
        size_t at = 0;
        for (SegmentType t : segment_types) {
            std::vector<float> rec(control.begin() + (long)at, control.begin() + (long)(at + floats(t)));
            at += floats(t);
            if (t == SegmentType::IntegralCubicCurve) {
                std::swap(rec[0], rec[2]);
                std::swap(rec[1], rec[3]);
            } else if (t == SegmentType::RationalCubicCurve) {
                std::swap(rec[0], rec[3]);
                std::swap(rec[1], rec[2]);
                std::swap(rec[4], rec[6]);
                std::swap(rec[5], rec[7]);
            }
            const Vec2 end{rec[rec.size() - 2], rec[rec.size() - 1]};
            rec[rec.size() - 2] = previous.first;
            rec[rec.size() - 1] = previous.second;
            previous = end;
            types.push_back(t);
            records.push_back(std::move(rec));
        }
        start = previous;
        segment_types.assign(types.rbegin(), types.rend());
        control.clear();
        for (auto it = records.rbegin(); it != records.rend(); ++it) control.insert(control.end(), it->begin(), it->end());
    }
    void convert_integral_curves_to_rational_curves() { // path.rs:492-534
        std::vector<float> out;
        size_t at = 0;
        for (SegmentType& t : segment_types) {
            const size_t n = floats(t);
            if (t == SegmentType::IntegralQuadraticCurve) {
                out.push_back(1.0f);
                t = SegmentType::RationalQuadraticCurve;
            } else if (t == SegmentType::IntegralCubicCurve) {
                out.insert(out.end(), 4, 1.0f);
                t = SegmentType::RationalCubicCurve;
            }
            out.insert(out.end(), control.begin() + (long)at, control.begin() + (long)(at + n));
            at += n;
        }
        control = std::move(out);
    }
    void convert_quadratic_curves_to_cubic_curves() { // path.rs:538-615
        std::vector<float> out;
        size_t at = 0;
        Vec2 previous = start;
        for (SegmentType& t : segment_types) {
            const size_t n = floats(t);
            const float* r = control.data() + at;
            at += n;
            if (t == SegmentType::IntegralQuadraticCurve) {
                const float c0x = previous.first + (r[0] - previous.first) * 2.0f / 3.0f, c0y = previous.second + (r[1] - previous.second) * 2.0f / 3.0f;
                const float c1x = r[2] + (r[0] - r[2]) * 2.0f / 3.0f, c1y = r[3] + (r[1] - r[3]) * 2.0f / 3.0f;
                for (float v : {c0x, c0y, c1x, c1y, r[2], r[3]}) out.push_back(safe_float(v));
                t = SegmentType::IntegralCubicCurve;
            } else if (t == SegmentType::RationalQuadraticCurve) {
                const float w = r[0];
                const float p0[3] = {1.0f, previous.first, previous.second}, p1[3] = {w, r[1] * w, r[2] * w}, p2[3] = {1.0f, r[3], r[4]};
                const float two_thirds = 2.0f / 3.0f;
                float n0[3], n1[3];
                for (int k = 0; k < 3; ++k) {
                    n0[k] = p0[k] + (p1[k] - p0[k]) * two_thirds;
                    n1[k] = p2[k] + (p1[k] - p2[k]) * two_thirds;
                }
                for (float v : {1.0f, n0[0], n1[0], 1.0f, n0[1] / n0[0], n0[2] / n0[0], n1[1] / n1[0], n1[2] / n1[0], r[3], r[4]}) out.push_back(safe_float(v));
                t = SegmentType::RationalCubicCurve;
            } else {
                out.insert(out.end(), r, r + n);
            }
            previous = Vec2{out[out.size() - 2], out[out.size() - 1]};
        }
        control = std::move(out);
    }
    void close() { // path.rs:621-628
        const Plane t = tangent_from_points(start, get_end());
        if (t.nx * t.nx + t.ny * t.ny <= 1e-4f) return;
        push_line(start);
    }
    void push_quarter_ellipse(Vec2 tangent_crossing, Vec2 to) { push_rational_quadratic_curve(0.70710678118654752440f, tangent_crossing, to); } // path.rs:631-636
    void push_elliptical_arc(Vec2 half_extent, float rotation, bool large_arc, bool sweep, Vec2 to) { // path.rs:639-708 (native: csrc/path.cpp)
        const Vec2 end = get_end();
        const float from[2] = {end.first, end.second}, half[2] = {half_extent.first, half_extent.second}, target[2] = {to.first, to.second};
        float records[20];
        uint32_t n = 0, is_line = 0;
        check(crh_path_elliptical_arc(from, half, rotation, large_arc, sweep, target, records, 4, &n, &is_line));
        if (is_line) {
            push_line(to);
            return;
        }
        for (uint32_t i = 0; i < n; ++i) push_rational_quadratic_curve(records[5 * i], {records[5 * i + 1], records[5 * i + 2]}, {records[5 * i + 3], records[5 * i + 4]});
    }

    static Path from_polygon(const std::vector<Vec2>& vertices) { // path.rs:711-724
        Path path;
        path.start = Vec2{safe_float(vertices.at(0).first), safe_float(vertices.at(0).second)};
        for (size_t i = 1; i < vertices.size(); ++i) path.push_line(vertices[i]);
        return path;
    }
    static Path from_regular_polygon(Vec2 center, float radius, float rotation, size_t vertex_count) { // path.rs:727-734
        std::vector<Vec2> vertices;
        for (size_t i = 0; i < vertex_count; ++i) {
            const float angle = rotation + (float)i / (float)vertex_count * 3.14159265358979323846f * 2.0f;
            vertices.push_back(Vec2{center.first + radius * std::cos(angle), center.second + radius * std::sin(angle)});
        }
        return from_polygon(vertices);
    }
    static Path from_rect(Vec2 center, Vec2 half_extent) { // path.rs:736-743
        const float cx = center.first, cy = center.second, hx = half_extent.first, hy = half_extent.second;
        return from_polygon({{cx - hx, cy - hy}, {cx - hx, cy + hy}, {cx + hx, cy + hy}, {cx + hx, cy - hy}});
    }

    static Path from_rounded_rect(Vec2 center, Vec2 half_extent, float radius) { // path.rs:746-780
        const float cx = center.first, cy = center.second, hx = half_extent.first, hy = half_extent.second, r = radius;
        const Vec2 v[4][3] = {{{cx - hx + r, cy - hy}, {cx - hx, cy - hy}, {cx - hx, cy - hy + r}},
                              {{cx - hx, cy + hy - r}, {cx - hx, cy + hy}, {cx - hx + r, cy + hy}},
                              {{cx + hx - r, cy + hy}, {cx + hx, cy + hy}, {cx + hx, cy + hy - r}},
                              {{cx + hx, cy - hy + r}, {cx + hx, cy - hy}, {cx + hx - r, cy - hy}}};
        Path path;
        path.start = Vec2{safe_float(v[3][2].first), safe_float(v[3][2].second)};
        for (const auto& corner : v) {
            path.push_line(corner[0]);
            path.push_quarter_ellipse(corner[1], corner[2]);
        }
        return path;
    }
    static Path from_ellipse(Vec2 center, Vec2 half_extent) { // path.rs:783-810
        const float cx = center.first, cy = center.second, hx = half_extent.first, hy = half_extent.second;
        const Vec2 v[4][2] = {{{cx - hx, cy - hy}, {cx - hx, cy}}, {{cx - hx, cy + hy}, {cx, cy + hy}}, {{cx + hx, cy + hy}, {cx + hx, cy}}, {{cx + hx, cy - hy}, {cx, cy - hy}}};
        Path path;
        path.start = Vec2{safe_float(v[3][1].first), safe_float(v[3][1].second)};
        for (const auto& corner : v) path.push_quarter_ellipse(corner[0], corner[1]);
        return path;
    }
    static Path from_circle(Vec2 center, float radius) { return from_ellipse(center, {radius, radius}); } // path.rs:813-815

  private:
    static size_t floats(SegmentType t) {
        static const size_t n[5] = {2, 4, 6, 5, 10};
        return n[(size_t)t];
    }
    static Plane tangent_from_points(Vec2 a, Vec2 b) { // path.rs:203-205: a v b
        return Plane{a.second * b.first - a.first * b.second, b.second - a.second, a.first - b.first};
    }
    static Plane signum(Plane p) {
        const float inv = 1.0f / std::sqrt(p.nx * p.nx + p.ny * p.ny);
        return Plane{p.c * inv, p.nx * inv, p.ny * inv};
    }
    void put(Vec2 p) {
        control.push_back(safe_float(p.first));
        control.push_back(safe_float(p.second));
    }
};

// Flattens the argument lists of Shape::from_paths (renderer.rs:177-183), one per Shape, into the SoA crh_path_batch.
class PathBatch {
  public:
    void add_shape(const std::vector<DynamicStrokeOptions>& dynamic_stroke_options, const std::vector<Path>& paths) {
        for (const Path& path : paths) {
            path_start_.push_back(path.start.first);
            path_start_.push_back(path.start.second);
            if (path.stroke_options) {
                path_stroke_.push_back((int32_t)stroke_options_.size());
                stroke_options_.push_back(path.stroke_options->to_c());
            } else {
                path_stroke_.push_back(-1);
            }
            for (SegmentType t : path.segment_types) types_.push_back((uint8_t)t);
            control_.insert(control_.end(), path.control.begin(), path.control.end());
            path_segment_begin_.push_back((uint32_t)types_.size());
        }
        shape_path_begin_.push_back((uint32_t)path_stroke_.size());
        for (const DynamicStrokeOptions& o : dynamic_stroke_options) dynamic_.push_back(o.to_c());
        shape_dynamic_begin_.push_back((uint32_t)dynamic_.size());
    }
    uint32_t n_shapes() const { return (uint32_t)shape_path_begin_.size() - 1u; }
    crh_path_batch view() const {
        crh_path_batch b = {};
        b.n_shapes = n_shapes();
        b.shape_path_begin = shape_path_begin_.data();
        b.n_paths = (uint32_t)path_stroke_.size();
        b.path_segment_begin = path_segment_begin_.data();
        b.path_start = path_start_.data();
        b.path_stroke_options = path_stroke_.data();
        b.n_segments = (uint32_t)types_.size();
        b.segment_types = types_.data();
        b.control_data = control_.data();
        b.n_control_floats = (uint32_t)control_.size();
        b.n_stroke_options = (uint32_t)stroke_options_.size();
        b.stroke_options = stroke_options_.data();
        b.shape_dynamic_begin = shape_dynamic_begin_.data();
        b.n_dynamic_stroke_options = (uint32_t)dynamic_.size();
        b.dynamic_stroke_options = dynamic_.data();
        return b;
    }

  private:
    std::vector<uint32_t> shape_path_begin_{0u}, path_segment_begin_{0u}, shape_dynamic_begin_{0u};
    std::vector<float> path_start_, control_;
    std::vector<int32_t> path_stroke_;
    std::vector<uint8_t> types_;
    std::vector<crh_stroke_options> stroke_options_;
    std::vector<crh_dynamic_stroke_options> dynamic_;
};

// ---------------------------------------------------------------------------------------------- renderer.rs
enum class RenderOperation : uint32_t { Stencil = 0, Clip = 1, UnClip = 2, Color = 3, SaveAlphaContext = 4, ScaleAlphaContext = 5, RestoreAlphaContext = 6 }; // :145-160

// Configuration::blending (renderer.rs:380-382): wgpu's blend types, as the C ABI's crh_color_target_state carries them
enum class BlendFactor : uint32_t { // wgpu::BlendFactor, same order; 13-16 (dual source) are refused: the colour cover has one output
    Zero = 0, One = 1, Src = 2, OneMinusSrc = 3, SrcAlpha = 4, OneMinusSrcAlpha = 5, Dst = 6, OneMinusDst = 7, DstAlpha = 8, OneMinusDstAlpha = 9,
    SrcAlphaSaturated = 10, Constant = 11, OneMinusConstant = 12, Src1 = 13, OneMinusSrc1 = 14, Src1Alpha = 15, OneMinusSrc1Alpha = 16
};
enum class BlendOperation : uint32_t { Add = 0, Subtract = 1, ReverseSubtract = 2, Min = 3, Max = 4 }; // wgpu::BlendOperation
struct BlendComponent { // wgpu::BlendComponent (the default is REPLACE)
    BlendFactor src_factor = BlendFactor::One;
    BlendFactor dst_factor = BlendFactor::Zero;
    BlendOperation operation = BlendOperation::Add;
    static const BlendComponent REPLACE, OVER;
    crh_blend_component to_c() const { return crh_blend_component{(uint32_t)src_factor, (uint32_t)dst_factor, (uint32_t)operation}; }
    static BlendComponent from_c(const crh_blend_component& c) { return BlendComponent{(BlendFactor)c.src_factor, (BlendFactor)c.dst_factor, (BlendOperation)c.operation}; }
};
inline const BlendComponent BlendComponent::REPLACE{BlendFactor::One, BlendFactor::Zero, BlendOperation::Add};
inline const BlendComponent BlendComponent::OVER{BlendFactor::One, BlendFactor::OneMinusSrcAlpha, BlendOperation::Add};
struct BlendState { // wgpu::BlendState
    BlendComponent color, alpha;
    static const BlendState REPLACE, ALPHA_BLENDING, PREMULTIPLIED_ALPHA_BLENDING;
};
inline const BlendState BlendState::REPLACE{BlendComponent::REPLACE, BlendComponent::REPLACE};
inline const BlendState BlendState::ALPHA_BLENDING{BlendComponent{BlendFactor::SrcAlpha, BlendFactor::OneMinusSrcAlpha, BlendOperation::Add}, BlendComponent::OVER};
inline const BlendState BlendState::PREMULTIPLIED_ALPHA_BLENDING{BlendComponent::OVER, BlendComponent::OVER};
namespace ColorWrites { // wgpu::ColorWrites
constexpr uint32_t RED = CRH_COLOR_WRITE_RED, GREEN = CRH_COLOR_WRITE_GREEN, BLUE = CRH_COLOR_WRITE_BLUE, ALPHA = CRH_COLOR_WRITE_ALPHA, COLOR = 7, ALL = CRH_COLOR_WRITE_ALL;
}
// wgpu::TextureFormat of the colour target. The value is the frame format that keeps f32 colours within a pass; attachment_format() the one
// that rounds every write, as a hardware blender does
enum class TextureFormat : uint32_t {
    Rgba8Unorm = CRH_FORMAT_RGBA8,
    Bgra8Unorm = CRH_FORMAT_BGRA8,
    Rgba8UnormSrgb = CRH_FORMAT_RGBA8_SRGB,
    Bgra8UnormSrgb = CRH_FORMAT_BGRA8_SRGB
};
inline uint32_t attachment_format(TextureFormat f) { return f == TextureFormat::Rgba8Unorm ? (uint32_t)CRH_FORMAT_RGBA8_ATTACHMENT : (uint32_t)f + 1u; }
// wgpu::ColorTargetState; `constant` stands for RenderPass::set_blend_constant, kept with the renderer here. `format` is kept host-side: the
// format a Frame created without one gets (the C ABI names a frame's format at crh_frame_create_format)
struct ColorTargetState {
    std::optional<BlendState> blend = std::nullopt; // None: the source replaces the target
    uint32_t write_mask = ColorWrites::ALL;
    std::array<float, 4> constant = {0.0f, 0.0f, 0.0f, 0.0f};
    TextureFormat format = TextureFormat::Rgba8Unorm;
    crh_color_target_state to_c() const {
        const BlendState b = blend.value_or(BlendState::REPLACE);
        return crh_color_target_state{blend ? 1u : 0u, b.color.to_c(), b.alpha.to_c(), write_mask, {constant[0], constant[1], constant[2], constant[3]}};
    }
    static ColorTargetState from_c(const crh_color_target_state& c) {
        ColorTargetState out;
        if (c.blend_enabled) out.blend = BlendState{BlendComponent::from_c(c.color), BlendComponent::from_c(c.alpha)};
        out.write_mask = c.write_mask;
        for (int i = 0; i < 4; ++i) out.constant[(size_t)i] = c.constant[i];
        return out;
    }
};

struct Configuration { // renderer.rs:380-405, the fields that change results on this path
    // msaa_sample_count: 1, 2, 4 or 8 with the standard sample locations (contrast_hip.h crh_config); any other count: CRH_ERR_UNSUPPORTED
    uint32_t msaa_sample_count = 1, clip_nesting_counter_bits = 4, winding_counter_bits = 4, alpha_layer_count = 0;
    // of the colour cover only, as in the reference (renderer.rs:743-745)
    crh_cull cull_mode = CRH_CULL_NONE;              // Option<wgpu::Face>
    crh_compare depth_compare = CRH_COMPARE_ALWAYS;  // wgpu::CompareFunction
    bool depth_write_enabled = false;
    std::optional<ColorTargetState> blending = std::nullopt; // the colour cover's blend state (renderer.rs:380-382); nullopt = the showcase's premultiplied "over"
};

class Renderer { // renderer.rs:408-435
  public:
    Renderer(int device, const Configuration& config) { // Renderer::new(&device, config) -> Result<Renderer, Error>
        const crh_config c = {config.msaa_sample_count, config.clip_nesting_counter_bits, config.winding_counter_bits, config.alpha_layer_count,
                              (uint32_t)config.cull_mode,  (uint32_t)config.depth_compare,      config.depth_write_enabled ? 1u : 0u};
        const std::optional<crh_color_target_state> blending = config.blending ? std::optional<crh_color_target_state>(config.blending->to_c()) : std::nullopt;
        check(crh_renderer_create_blended(&c, blending ? &*blending : nullptr, device, &handle_));
        samples_ = config.msaa_sample_count;
        format_ = config.blending ? config.blending->format : TextureFormat::Rgba8Unorm;
    }
    ~Renderer() { crh_renderer_destroy(handle_); }
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;
    Configuration get_config() const { // renderer.rs:887
        crh_config c;
        check(crh_renderer_get_config(handle_, &c));
        return Configuration{c.msaa_sample_count, c.clip_nesting_counter_bits, c.winding_counter_bits, c.alpha_layer_count,
                             (crh_cull)c.cull_mode, (crh_compare)c.depth_compare, c.depth_write_enabled != 0, get_blending()};
    }
    ColorTargetState get_blending() const { // the state the renderer was created with (the "over" state for a Configuration without one)
        crh_color_target_state b;
        check(crh_renderer_get_blending(handle_, &b));
        ColorTargetState out = ColorTargetState::from_c(b);
        out.format = format_;
        return out;
    }
    void synchronize() { check(crh_renderer_synchronize(handle_)); }
    crh_renderer* raw() const { return handle_; }
    uint32_t msaa_sample_count() const { return samples_; }
    TextureFormat format() const { return format_; } // Configuration::blending's format (Rgba8Unorm without one)

  private:
    crh_renderer* handle_ = nullptr;
    uint32_t samples_ = 1;
    TextureFormat format_ = TextureFormat::Rgba8Unorm;
};

// The caller-owned colour + depth/stencil attachments of the render pass (examples/showcase/main.rs:217-230).
class Frame {
  public:
    // `format`: CRH_FORMAT_RGBA8 (f32 colours during a pass, one rounding at the end) or CRH_FORMAT_RGBA8_ATTACHMENT (every blend rounded to 8 bits, as
    // the wgpu Rgba8Unorm attachment of main.rs:205-215 would), or one of the BGRA / sRGB formats (include/contrast_hip.h)
    Frame(Renderer& renderer, uint32_t width, uint32_t height, uint32_t format) : width_(width), height_(height), samples_(renderer.msaa_sample_count()) {
        check(crh_frame_create_format(renderer.raw(), width, height, format, &handle_));
    }
    // ... in the format of the renderer's Configuration::blending (CRH_FORMAT_RGBA8 without one)
    Frame(Renderer& renderer, uint32_t width, uint32_t height) : Frame(renderer, width, height, (uint32_t)renderer.format()) {}
    ~Frame() { crh_frame_destroy(handle_); }
    Frame(const Frame&) = delete;
    Frame& operator=(const Frame&) = delete;
    void clear() { check(crh_frame_clear(handle_)); } // LoadOp::Clear(TRANSPARENT) + depth clear 1.0 + stencil clear
    void keep_pass_state() { check(crh_frame_keep_pass_state(handle_)); } // stencil, alpha layers and sample colours stay with the frame between passes, until clear()
    void set_tile_rows(uint32_t row_begin, uint32_t row_end) { check(crh_frame_set_tile_rows(handle_, row_begin, row_end)); } // the tile split of the multi-GPU path: draw these pixel rows only
    // the depth attachment (present when the Configuration tests or writes depth): LoadOp::Clear(value), the depth of the 3-D scene
    // the Shapes are decals in ([height][width], replicated to the samples), and read back of every sample
    void clear_depth(float value) { check(crh_frame_clear_depth(handle_, value)); }
    void upload_depth(const std::vector<float>& depth) {
        if (depth.size() != (size_t)width_ * height_) throw Error(CRH_ERR_INVALID_ARGUMENT);
        check(crh_frame_upload_depth(handle_, depth.data()));
    }
    std::vector<float> download_depth() {
        std::vector<float> out((size_t)width_ * height_ * samples_);
        check(crh_frame_download_depth(handle_, out.data()));
        return out;
    }
    // LoadOp::Load of caller content: premultiplied 8-bit pixels in the frame's storage order (B G R A for a BGRA format, sRGB rgb for an sRGB one),
    // row 0 = top; stencil, alpha layers and pass state reset as by clear(), depth kept
    void upload(const std::vector<uint8_t>& rgba8) {
        if (rgba8.size() != (size_t)width_ * height_ * 4) throw Error(CRH_ERR_INVALID_ARGUMENT);
        check(crh_frame_upload(handle_, rgba8.data()));
    }
    // crh_frame_load_image: upload() with the bytes taken from level 0 of an Image on the device (the same size, the same renderer); complete on
    // return, so the image may be destroyed afterwards
    inline void load_image(const class Image& image);
    std::vector<uint8_t> download() {                 // MSAA resolve + read back: premultiplied 8-bit pixels in the frame's storage order, row 0 = top
        std::vector<uint8_t> out((size_t)width_ * height_ * 4);
        check(crh_frame_download(handle_, out.data()));
        return out;
    }
    uint32_t width() const { return width_; }
    uint32_t height() const { return height_; }
    crh_frame* raw() const { return handle_; }

  private:
    crh_frame* handle_ = nullptr;
    uint32_t width_, height_, samples_;
};

struct ShapeBuffers { // the byte image Shape::from_paths uploads (renderer.rs:198-209)
    uint64_t vertex_offsets[8], index_offsets[3];
    std::vector<uint8_t> vertex_bytes, index_bytes;
};

class RenderPass;

// Gradient paints: the source of a Color cover in place of the instance's one colour (include/contrast_hip.h crh_scene_set_paints states the model)
enum class Spread : uint32_t { Pad = CRH_SPREAD_PAD, Repeat = CRH_SPREAD_REPEAT, Reflect = CRH_SPREAD_REFLECT };
struct GradientStop {
    float offset;               // in [0, 1], non-decreasing along the stops
    std::array<float, 4> color; // straight RGBA
};
class Paint {
  public:
    // t = 0 at p0, t = 1 at p1
    static Paint linear(const std::array<float, 2>& p0, const std::array<float, 2>& p1, const std::vector<GradientStop>& stops, Spread spread = Spread::Pad) {
        return Paint(CRH_PAINT_LINEAR, spread, p0, p1, stops);
    }
    // t = distance from `center` / radius
    static Paint radial(const std::array<float, 2>& center, float radius, const std::vector<GradientStop>& stops, Spread spread = Spread::Pad) {
        return Paint(CRH_PAINT_RADIAL, spread, center, {radius, 0.0f}, stops);
    }
    // t = 0 on the ray from `center` at the angle `start`, t = 1 at `end`: radians, from +x towards +y, 0 < |end - start| <= 2 pi; end < start reads the stops clockwise
    static Paint conic(const std::array<float, 2>& center, float start, float end, const std::vector<GradientStop>& stops, Spread spread = Spread::Pad) {
        return Paint(CRH_PAINT_CONIC, spread, center, {start, end}, stops);
    }
    void validate() const { check(crh_paint_validate(&c_)); } // host only: throws what Scene::set_paints would
    const crh_paint& to_c() const { return c_; }

  private:
    Paint(uint32_t kind, Spread spread, const std::array<float, 2>& p0, const std::array<float, 2>& p1, const std::vector<GradientStop>& stops) {
        if (stops.empty() || stops.size() > CRH_MAX_GRADIENT_STOPS) throw Error(CRH_ERR_INVALID_ARGUMENT);
        c_ = crh_paint{};
        c_.kind = kind, c_.spread = (uint32_t)spread, c_.n_stops = (uint32_t)stops.size();
        c_.p0[0] = p0[0], c_.p0[1] = p0[1], c_.p1[0] = p1[0], c_.p1[1] = p1[1];
        for (size_t i = 0; i < stops.size(); ++i) {
            c_.stops[i].offset = stops[i].offset;
            for (int ch = 0; ch < 4; ++ch) c_.stops[i].color[ch] = stops[i].color[(size_t)ch];
        }
    }
    crh_paint c_;
};

// Image paints: the texels of an Image as the source of a Color cover (include/contrast_hip.h crh_scene_set_paints_with_images states the model)
enum class Filter : uint32_t { Nearest = CRH_FILTER_NEAREST, Linear = CRH_FILTER_LINEAR, NearestMipmap = CRH_FILTER_NEAREST | CRH_FILTER_MIPMAP, LinearMipmap = CRH_FILTER_LINEAR | CRH_FILTER_MIPMAP };
// what Image::blur reads outside the image (crh_blur_edge); Transparent grows the result by the radius on every side
enum class BlurEdge : uint32_t { Transparent = CRH_BLUR_EDGE_TRANSPARENT, Pad = CRH_BLUR_EDGE_PAD, Repeat = CRH_BLUR_EDGE_REPEAT, Reflect = CRH_BLUR_EDGE_REFLECT };
// crh_blur_taps (host only) -> the integer taps q[0 .. radius] of one axis of Image::blur, radius = ceil(3 sigma) = size() - 1; they sum to
// exactly 65536 over the 2 radius + 1 positions (include/contrast_hip.h crh_image_blur states the rule)
inline std::vector<uint32_t> blur_taps(float sigma) {
    uint32_t radius = 0;
    check(crh_blur_taps(sigma, nullptr, 0, &radius));
    std::vector<uint32_t> taps(radius + 1u);
    check(crh_blur_taps(sigma, taps.data(), (uint32_t)taps.size(), &radius));
    return taps;
}
// Compositing (include/contrast_hip.h crh_image_composite states the rule): the Porter-Duff operator, the blend mode, and the rule on texel pairs
enum class CompositeOp : uint32_t {
    Clear = CRH_COMPOSITE_CLEAR, Copy = CRH_COMPOSITE_COPY, Dst = CRH_COMPOSITE_DST, SrcOver = CRH_COMPOSITE_SRC_OVER, DstOver = CRH_COMPOSITE_DST_OVER, SrcIn = CRH_COMPOSITE_SRC_IN,
    DstIn = CRH_COMPOSITE_DST_IN, SrcOut = CRH_COMPOSITE_SRC_OUT, DstOut = CRH_COMPOSITE_DST_OUT, SrcAtop = CRH_COMPOSITE_SRC_ATOP, DstAtop = CRH_COMPOSITE_DST_ATOP, Xor = CRH_COMPOSITE_XOR,
    Plus = CRH_COMPOSITE_PLUS
};
enum class BlendMode : uint32_t {
    Normal = CRH_BLEND_NORMAL, Multiply = CRH_BLEND_MULTIPLY, Screen = CRH_BLEND_SCREEN, Overlay = CRH_BLEND_OVERLAY, Darken = CRH_BLEND_DARKEN, Lighten = CRH_BLEND_LIGHTEN,
    HardLight = CRH_BLEND_HARD_LIGHT, Difference = CRH_BLEND_DIFFERENCE, Exclusion = CRH_BLEND_EXCLUSION
};
// crh_composite_texels (host only): the rule on source.size() / 4 texel pairs of premultiplied RGBA8 -> as many bytes
inline std::vector<uint8_t> composite_texels(const std::vector<uint8_t>& source, const std::vector<uint8_t>& backdrop, CompositeOp op = CompositeOp::SrcOver, BlendMode mode = BlendMode::Normal,
                                             float opacity = 1.0f) {
    if (source.size() != backdrop.size() || source.size() % 4u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    const crh_composite how = {(uint32_t)op, (uint32_t)mode, opacity, 0, 0};
    std::vector<uint8_t> out(source.size());
    check(crh_composite_texels(&how, source.data(), backdrop.data(), source.size() / 4u, out.data()));
    return out;
}
// Colour filters (include/contrast_hip.h crh_image_color_filter states the rule): a 4 x 5 matrix on unpremultiplied colours, rows r', g', b', a',
// columns r, g, b, a, 1, and one 256-entry table per channel. The constructors use the SVG filter-effects coefficients, computed in double and
// rounded to float once.
using ColorMatrixValues = std::array<float, 20>;
using ColorTables = std::array<uint8_t, 1024>; // r[256] g[256] b[256] a[256]
struct ColorMatrix {
    static ColorMatrixValues from_rows(const double (&m)[20]) {
        ColorMatrixValues out;
        for (size_t n = 0; n < 20; ++n) out[n] = (float)m[n];
        return out;
    }
    static ColorMatrixValues identity() { return opacity(1.0); }
    static ColorMatrixValues saturate(double s) {
        const double m[20] = {0.213 + 0.787 * s, 0.715 - 0.715 * s, 0.072 - 0.072 * s, 0, 0, 0.213 - 0.213 * s, 0.715 + 0.285 * s, 0.072 - 0.072 * s, 0, 0,
                              0.213 - 0.213 * s, 0.715 - 0.715 * s, 0.072 + 0.928 * s, 0, 0, 0, 0, 0, 1, 0};
        return from_rows(m);
    }
    static ColorMatrixValues hue_rotate(double degrees) {
        const double angle = degrees * 3.14159265358979323846 / 180.0, c = std::cos(angle), s = std::sin(angle);
        const double m[20] = {0.213 + c * 0.787 - s * 0.213, 0.715 - c * 0.715 - s * 0.715, 0.072 - c * 0.072 + s * 0.928, 0, 0,
                              0.213 - c * 0.213 + s * 0.143, 0.715 + c * 0.285 + s * 0.140, 0.072 - c * 0.072 - s * 0.283, 0, 0,
                              0.213 - c * 0.213 - s * 0.787, 0.715 - c * 0.715 + s * 0.715, 0.072 + c * 0.928 + s * 0.072, 0, 0, 0, 0, 0, 1, 0};
        return from_rows(m);
    }
    static ColorMatrixValues luminance_to_alpha() {
        const double m[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.2125, 0.7154, 0.0721, 0, 0};
        return from_rows(m);
    }
    // every texel takes the straight colour (r, g, b) and a times its alpha: the colour of a drop shadow
    static ColorMatrixValues flood(double r, double g, double b, double a) {
        const double m[20] = {0, 0, 0, 0, r, 0, 0, 0, 0, g, 0, 0, 0, 0, b, 0, 0, 0, a, 0};
        return from_rows(m);
    }
    static ColorMatrixValues opacity(double a) {
        const double m[20] = {1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, a, 0};
        return from_rows(m);
    }
};
// crh_color_filter_texels (host only): the rule on texels.size() / 4 texels of premultiplied RGBA8 -> as many bytes; a null matrix or tables is the identity
inline std::vector<uint8_t> color_filter_texels(const std::vector<uint8_t>& texels, const ColorMatrixValues* matrix = nullptr, const ColorTables* tables = nullptr) {
    if (texels.size() % 4u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    std::vector<uint8_t> out(texels.size());
    check(crh_color_filter_texels(matrix ? matrix->data() : nullptr, tables ? tables->data() : nullptr, texels.data(), texels.size() / 4u, out.data()));
    return out;
}
// Morphology (include/contrast_hip.h crh_image_morphology states the rule): per channel the min (Erode) or max (Dilate) over a rectangle
enum class MorphologyOp : uint32_t { Erode = CRH_MORPHOLOGY_ERODE, Dilate = CRH_MORPHOLOGY_DILATE };
// crh_morphology_size (host only) -> the size of Image::morphology's result on a width x height image; throws what it would refuse
inline std::array<uint32_t, 2> morphology_size(uint32_t width, uint32_t height, MorphologyOp op, uint32_t radius_x, uint32_t radius_y, BlurEdge edge = BlurEdge::Transparent) {
    std::array<uint32_t, 2> out = {0u, 0u};
    check(crh_morphology_size(width, height, (uint32_t)op, radius_x, radius_y, (uint32_t)edge, &out[0], &out[1]));
    return out;
}
// crh_morphology_texels (host only): the rule on a width x height image of RGBA8 in host memory -> the bytes of the result, of morphology_size's size
inline std::vector<uint8_t> morphology_texels(uint32_t width, uint32_t height, const std::vector<uint8_t>& texels, MorphologyOp op, uint32_t radius_x, uint32_t radius_y,
                                              BlurEdge edge = BlurEdge::Transparent) {
    if (texels.size() != (size_t)width * height * 4u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    const std::array<uint32_t, 2> size = morphology_size(width, height, op, radius_x, radius_y, edge);
    std::vector<uint8_t> out((size_t)size[0] * size[1] * 4u);
    check(crh_morphology_texels(width, height, texels.data(), (uint32_t)op, radius_x, radius_y, (uint32_t)edge, out.data()));
    return out;
}
// Convolution (include/contrast_hip.h crh_image_convolve states the rule): a kernel matrix of order_x columns and order_y rows, row-major, in
// SVG's orientation. The presets divide by 1 unless they say otherwise; target = the kernel cell on the output texel, the centre by default.
struct ConvolveKernel {
    uint32_t order_x = 1, order_y = 1;
    std::vector<float> values = {1.0f};
    float divisor = 1.0f, bias = 0.0f;
    uint32_t target_x = 0, target_y = 0;
    ConvolveKernel() = default;
    ConvolveKernel(uint32_t ox, uint32_t oy, std::vector<float> v, float d = 1.0f, float b = 0.0f) : order_x(ox), order_y(oy), values(std::move(v)), divisor(d), bias(b), target_x(ox / 2u), target_y(oy / 2u) {}
    static ConvolveKernel identity() { return ConvolveKernel(); }
    static ConvolveKernel sharpen(float amount = 1.0f) { return ConvolveKernel(3, 3, {0, -amount, 0, -amount, 1.0f + 4.0f * amount, -amount, 0, -amount, 0}); }
    static ConvolveKernel box(uint32_t n) { return ConvolveKernel(n, n, std::vector<float>((size_t)n * n, 1.0f), (float)(n * n)); } // the mean of n x n texels
    static ConvolveKernel emboss() { return ConvolveKernel(3, 3, {-2, -1, 0, -1, 1, 1, 0, 1, 2}); }
    static ConvolveKernel laplacian() { return ConvolveKernel(3, 3, {0, 1, 0, 1, -4, 1, 0, 1, 0}); }
    static ConvolveKernel sobel_x() { return ConvolveKernel(3, 3, {-1, 0, 1, -2, 0, 2, -1, 0, 1}); }
    static ConvolveKernel sobel_y() { return ConvolveKernel(3, 3, {-1, -2, -1, 0, 0, 0, 1, 2, 1}); }
    // the C struct; it points into `values`, so it lives no longer than this kernel
    crh_convolve to_c(BlurEdge edge, bool preserve_alpha) const {
        if (values.size() != (size_t)order_x * order_y) throw Error(CRH_ERR_INVALID_ARGUMENT);
        return crh_convolve{order_x, order_y, target_x, target_y, values.data(), divisor, bias, (uint32_t)edge, preserve_alpha ? 1u : 0u};
    }
};
// crh_convolve_coefficients (host only) -> the quantised kernel, order_x * order_y entries row-major, and bias_k behind them
inline std::vector<int32_t> convolve_coefficients(const ConvolveKernel& kernel) {
    const crh_convolve how = kernel.to_c(BlurEdge::Pad, false);
    std::vector<int32_t> out((size_t)kernel.order_x * kernel.order_y + 1u);
    check(crh_convolve_coefficients(&how, out.data(), (uint32_t)out.size() - 1u, &out.back()));
    return out;
}
// crh_convolve_texels (host only): the rule on a width x height image of RGBA8 in host memory -> the bytes of the result, of the same size
inline std::vector<uint8_t> convolve_texels(uint32_t width, uint32_t height, const std::vector<uint8_t>& texels, const ConvolveKernel& kernel, BlurEdge edge = BlurEdge::Pad,
                                            bool preserve_alpha = false) {
    if (texels.size() != (size_t)width * height * 4u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    const crh_convolve how = kernel.to_c(edge, preserve_alpha);
    std::vector<uint8_t> out(texels.size());
    check(crh_convolve_texels(width, height, texels.data(), &how, out.data()));
    return out;
}
// Lighting (include/contrast_hip.h crh_image_lighting states the rule): an image's alpha as a height field under one light.
enum class LightingOp : uint32_t { Diffuse = CRH_LIGHTING_DIFFUSE, Specular = CRH_LIGHTING_SPECULAR };
// A light infinitely far away (SVG feDistantLight): azimuth in the image plane from the x axis towards y (down), elevation above it, in degrees
struct DistantLight {
    float azimuth = 0.0f, elevation = 0.0f;
};
// A light at (x, y, z) in the image's texel space, x right, y down, z towards the viewer (SVG fePointLight)
struct PointLight {
    float x = 0.0f, y = 0.0f, z = 0.0f;
};
// A light at `position` that shines towards `points_at` (SVG feSpotLight); cone_angle in degrees, 0 = no cone
struct SpotLight {
    std::array<float, 3> position = {0.0f, 0.0f, 1.0f}, points_at = {0.0f, 0.0f, 0.0f};
    float exponent = 1.0f, cone_angle = 0.0f;
};
// What is lit and how: the fields of crh_lighting that do not describe the light
struct Lighting {
    LightingOp op = LightingOp::Diffuse;
    float surface_scale = 1.0f, constant = 1.0f, specular_exponent = 1.0f;
    std::array<float, 3> color = {1.0f, 1.0f, 1.0f};
    BlurEdge edge = BlurEdge::Pad;
    crh_lighting to_c(const DistantLight& light) const {
        crh_lighting how = base(CRH_LIGHT_DISTANT);
        how.azimuth = light.azimuth, how.elevation = light.elevation;
        return how;
    }
    crh_lighting to_c(const PointLight& light) const {
        crh_lighting how = base(CRH_LIGHT_POINT);
        how.position[0] = light.x, how.position[1] = light.y, how.position[2] = light.z;
        return how;
    }
    crh_lighting to_c(const SpotLight& light) const {
        crh_lighting how = base(CRH_LIGHT_SPOT);
        for (int c = 0; c < 3; ++c) how.position[c] = light.position[(size_t)c], how.points_at[c] = light.points_at[(size_t)c];
        how.spot_exponent = light.exponent, how.cone_angle = light.cone_angle;
        return how;
    }

  private:
    crh_lighting base(uint32_t light) const {
        crh_lighting how = {};
        how.op = (uint32_t)op, how.light = light, how.edge = (uint32_t)edge;
        how.surface_scale = surface_scale, how.constant = constant, how.specular_exponent = specular_exponent;
        for (int c = 0; c < 3; ++c) how.color[c] = color[(size_t)c];
        return how;
    }
};
// crh_lighting_texels (host only): the rule on a width x height image of RGBA8 in host memory -> the bytes of the result, of the same size
template <class Light>
inline std::vector<uint8_t> lighting_texels(uint32_t width, uint32_t height, const std::vector<uint8_t>& texels, const Light& light, const Lighting& lighting = Lighting()) {
    if (texels.size() != (size_t)width * height * 4u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    const crh_lighting how = lighting.to_c(light);
    std::vector<uint8_t> out(texels.size());
    check(crh_lighting_texels(width, height, texels.data(), &how, out.data()));
    return out;
}
// Turbulence (include/contrast_hip.h crh_image_turbulence states the rule): an image of procedural noise, SVG feTurbulence.
enum class TurbulenceKind : uint32_t { FractalNoise = CRH_TURBULENCE_FRACTAL_NOISE, Turbulence = CRH_TURBULENCE_TURBULENCE };
// The fields of crh_turbulence: lattice cells per texel on each axis, octaves of twice the frequency and half the weight each, the seed of
// the tables, whether the image tiles with itself, whether alpha is 255 instead of a fourth channel of noise, and the noise-space position of texel (0, 0).
struct Turbulence {
    std::array<float, 2> base_frequency = {0.0f, 0.0f};
    uint32_t octaves = 1;
    int32_t seed = 0;
    TurbulenceKind kind = TurbulenceKind::Turbulence;
    bool stitch = false, opaque = false;
    std::array<float, 2> offset = {0.0f, 0.0f};
    crh_turbulence to_c() const {
        crh_turbulence how = {};
        how.kind = (uint32_t)kind, how.octaves = octaves, how.seed = seed, how.stitch = stitch ? 1u : 0u, how.opaque = opaque ? 1u : 0u;
        for (int c = 0; c < 2; ++c) how.base_frequency[c] = base_frequency[(size_t)c], how.offset[c] = offset[(size_t)c];
        return how;
    }
};
// crh_turbulence_texels (host only): the rule -> the width * height * 4 bytes of the image
inline std::vector<uint8_t> turbulence_texels(uint32_t width, uint32_t height, const Turbulence& turbulence) {
    const crh_turbulence how = turbulence.to_c();
    check(crh_turbulence_validate(&how));
    if (width == 0u || height == 0u || width > 16384u || height > 16384u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    std::vector<uint8_t> out((size_t)width * height * 4u);
    check(crh_turbulence_texels(width, height, &how, out.data()));
    return out;
}
// crh_turbulence_tables (host only): the permutation of 0..255 and the unit gradients, gradient[(k * 256 + i) * 2 + c], that `seed` gives
struct TurbulenceTables {
    std::array<uint8_t, 256> lattice;
    std::array<double, 4 * 256 * 2> gradient;
};
inline TurbulenceTables turbulence_tables(int32_t seed) {
    TurbulenceTables tables;
    check(crh_turbulence_tables(seed, tables.lattice.data(), tables.gradient.data()));
    return tables;
}
// Displacement (include/contrast_hip.h crh_image_displace states the rule): an image read through the per-texel offsets of a second one, SVG feDisplacementMap.
enum class Channel : uint32_t { R = CRH_CHANNEL_R, G = CRH_CHANNEL_G, B = CRH_CHANNEL_B, A = CRH_CHANNEL_A };
// The fields of crh_displace: the scale of each axis in texels (SVG has one: give it twice), the map's channels that move x and y, the
// filter (Nearest or Linear) and what the SOURCE is outside itself. The defaults are SVG's.
struct Displace {
    std::array<float, 2> scale = {0.0f, 0.0f};
    Channel x_channel = Channel::A, y_channel = Channel::A;
    Filter filter = Filter::Linear;
    BlurEdge edge = BlurEdge::Transparent;
    crh_displace to_c() const {
        crh_displace how = {};
        how.scale[0] = scale[0], how.scale[1] = scale[1];
        how.x_channel = (uint32_t)x_channel, how.y_channel = (uint32_t)y_channel, how.filter = (uint32_t)filter, how.edge = (uint32_t)edge;
        return how;
    }
};
// crh_displace_texels (host only): the rule on two width * height * 4 byte arrays, the source and the map -> the bytes of the result
inline std::vector<uint8_t> displace_texels(uint32_t width, uint32_t height, const std::vector<uint8_t>& texels, const std::vector<uint8_t>& map, const Displace& displace) {
    if (texels.size() != (size_t)width * height * 4u || map.size() != texels.size()) throw Error(CRH_ERR_INVALID_ARGUMENT);
    const crh_displace how = displace.to_c();
    std::vector<uint8_t> out(texels.size());
    check(crh_displace_texels(width, height, texels.data(), map.data(), &how, out.data()));
    return out;
}
// crh_displace_offset (host only): the offsets (qx, qy), in 1/256 texel, of two straight map codes <= 255
inline std::array<int32_t, 2> displace_offset(const Displace& displace, uint32_t code_x, uint32_t code_y) {
    const crh_displace how = displace.to_c();
    std::array<int32_t, 2> q = {0, 0};
    check(crh_displace_offset(&how, code_x, code_y, q.data()));
    return q;
}
// Variable blur (include/contrast_hip.h crh_image_variable_blur states the rule): a blur whose sigma a mask sets per texel.
// The fields of crh_variable_blur: per axis the sigma at mask code 0 and at code 255 (linear in the code between; either may be the
// larger), the mask's channel whose STORED code is the level, and what the SOURCE is outside itself. The edge's default is Pad because
// the call keeps the size and a backdrop should not darken at its rim.
struct VariableBlur {
    std::array<float, 2> sigma_x = {0.0f, 0.0f}, sigma_y = {0.0f, 0.0f};
    Channel channel = Channel::A;
    BlurEdge edge = BlurEdge::Pad;
    crh_variable_blur to_c() const {
        crh_variable_blur how = {};
        how.sigma_x[0] = sigma_x[0], how.sigma_x[1] = sigma_x[1], how.sigma_y[0] = sigma_y[0], how.sigma_y[1] = sigma_y[1];
        how.channel = (uint32_t)channel, how.edge = (uint32_t)edge;
        return how;
    }
};
// crh_variable_blur_texels (host only): the rule on two width * height * 4 byte arrays, the source and the mask -> the bytes of the result
inline std::vector<uint8_t> variable_blur_texels(uint32_t width, uint32_t height, const std::vector<uint8_t>& texels, const std::vector<uint8_t>& mask, const VariableBlur& blur) {
    if (texels.size() != (size_t)width * height * 4u || mask.size() != texels.size()) throw Error(CRH_ERR_INVALID_ARGUMENT);
    const crh_variable_blur how = blur.to_c();
    std::vector<uint8_t> out(texels.size());
    check(crh_variable_blur_texels(width, height, texels.data(), mask.data(), &how, out.data()));
    return out;
}
// crh_variable_blur_sigma (host only): the sigmas (x, y) of one mask code <= 255
inline std::array<float, 2> variable_blur_sigma(const VariableBlur& blur, uint32_t code) {
    const crh_variable_blur how = blur.to_c();
    std::array<float, 2> sigma = {0.0f, 0.0f};
    check(crh_variable_blur_sigma(&how, code, &sigma[0], &sigma[1]));
    return sigma;
}
// crh_variable_blur_validate (host only): throws what Image::variable_blur would refuse of the fields
inline void variable_blur_validate(const VariableBlur& blur) {
    const crh_variable_blur how = blur.to_c();
    check(crh_variable_blur_validate(&how));
}
// Transform (include/contrast_hip.h crh_image_transform states the rule): an image seen through a 3 x 3 matrix, in a result of any size.
enum class TransformFilter : uint32_t { Nearest = CRH_TRANSFORM_NEAREST, Linear = CRH_TRANSFORM_LINEAR, Cubic = CRH_TRANSFORM_CUBIC };
// The fields of crh_transform: the matrix that maps RESULT coordinates (x, y, 1) to SOURCE coordinates, row-major (the identity by
// default), the result's size, the filter and what the SOURCE is outside itself.
struct Transform {
    std::array<double, 9> matrix = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    uint32_t width = 1, height = 1;
    TransformFilter filter = TransformFilter::Linear;
    BlurEdge edge = BlurEdge::Transparent;
    crh_transform to_c() const {
        crh_transform how = {};
        for (size_t k = 0; k < 9; ++k) how.matrix[k] = matrix[k];
        how.width = width, how.height = height, how.filter = (uint32_t)filter, how.edge = (uint32_t)edge;
        return how;
    }
};
// What crh_transform_fit gives: the call that holds the whole source moved by `forward`, and where the target space's (0, 0) lies in its result
struct TransformFit {
    Transform transform;
    std::array<int32_t, 2> origin = {0, 0};
};
// crh_transform_validate (host only): throws what Image::resample would refuse of the fields
inline void transform_validate(const Transform& transform) {
    const crh_transform how = transform.to_c();
    check(crh_transform_validate(&how));
}
// crh_transform_fit (host only): `forward` maps the coordinates of a width x height source to the caller's target space
inline TransformFit transform_fit(uint32_t width, uint32_t height, const std::array<double, 9>& forward, TransformFilter filter = TransformFilter::Linear, BlurEdge edge = BlurEdge::Transparent) {
    crh_transform how = {};
    TransformFit fit;
    check(crh_transform_fit(width, height, forward.data(), (uint32_t)filter, (uint32_t)edge, &how, fit.origin.data()));
    for (size_t k = 0; k < 9; ++k) fit.transform.matrix[k] = how.matrix[k];
    fit.transform.width = how.width, fit.transform.height = how.height, fit.transform.filter = filter, fit.transform.edge = edge;
    return fit;
}
// crh_transform_position (host only): where result texel (i, j) reads the source, in 1/256 texel, and whether it is visible
struct TransformPosition {
    std::array<int32_t, 2> position = {0, 0};
    bool visible = false;
};
inline TransformPosition transform_position(const Transform& transform, uint32_t i, uint32_t j) {
    const crh_transform how = transform.to_c();
    TransformPosition at;
    uint32_t visible = 0;
    check(crh_transform_position(&how, i, j, at.position.data(), &visible));
    at.visible = visible != 0u;
    return at;
}
// crh_transform_texels (host only): the rule on the width * height * 4 bytes of a source -> the transform.width * transform.height * 4 bytes of the result
inline std::vector<uint8_t> transform_texels(uint32_t width, uint32_t height, const std::vector<uint8_t>& texels, const Transform& transform) {
    if (texels.size() != (size_t)width * height * 4u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    const crh_transform how = transform.to_c();
    transform_validate(transform); // (the result's size before its room is taken)
    std::vector<uint8_t> out((size_t)how.width * how.height * 4u);
    check(crh_transform_texels(width, height, texels.data(), &how, out.data()));
    return out;
}
// Distance fields (include/contrast_hip.h crh_image_distance_field states the rule): the exact Euclidean distance to a shape in 8 bits over a spread.
enum class DistanceMode : uint32_t { Outside = CRH_DISTANCE_OUTSIDE, Inside = CRH_DISTANCE_INSIDE };
// The fields of crh_distance: what the distance is measured to (Outside: the shape, 255 on it and 0 at the spread; Inside: what is not the
// shape, 0 off it and rising into it), the channel whose stored code against the threshold makes the shape, the spread in texels
// (1..CRH_MAX_DISTANCE_SPREAD) and what the source is outside itself.
struct Distance {
    uint32_t spread = 1;
    DistanceMode mode = DistanceMode::Outside;
    Channel channel = Channel::A;
    uint32_t threshold = 128;
    BlurEdge edge = BlurEdge::Transparent;
    crh_distance to_c() const {
        crh_distance how = {};
        how.mode = (uint32_t)mode, how.channel = (uint32_t)channel, how.threshold = threshold, how.spread = spread, how.edge = (uint32_t)edge;
        return how;
    }
};
// crh_distance_code (host only): the result byte of one squared distance between texel centres
inline uint32_t distance_code(const Distance& distance, uint64_t squared_distance) {
    const crh_distance how = distance.to_c();
    uint32_t code = 0;
    check(crh_distance_code(&how, squared_distance, &code));
    return code;
}
// crh_distance_size (host only) -> the size of Image::distance_field's result on a width x height image; throws what it would refuse
inline std::array<uint32_t, 2> distance_size(uint32_t width, uint32_t height, const Distance& distance) {
    const crh_distance how = distance.to_c();
    std::array<uint32_t, 2> out = {0, 0};
    check(crh_distance_size(width, height, &how, &out[0], &out[1]));
    return out;
}
// crh_distance_texels (host only): the rule on a width x height image of RGBA8 in host memory -> the bytes of the result, of distance_size's size
inline std::vector<uint8_t> distance_texels(uint32_t width, uint32_t height, const std::vector<uint8_t>& texels, const Distance& distance) {
    if (texels.size() != (size_t)width * height * 4u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    const std::array<uint32_t, 2> size = distance_size(width, height, distance);
    const crh_distance how = distance.to_c();
    std::vector<uint8_t> out((size_t)size[0] * size[1] * 4u);
    check(crh_distance_texels(width, height, texels.data(), &how, out.data()));
    return out;
}
// Resize (include/contrast_hip.h crh_image_resize states the rule): the reconstruction filter, widened by the ratio on an axis that shrinks.
enum class ResizeFilter : uint32_t { Box = CRH_RESIZE_BOX, Triangle = CRH_RESIZE_TRIANGLE, CatmullRom = CRH_RESIZE_CATMULL_ROM, Mitchell = CRH_RESIZE_MITCHELL, Lanczos3 = CRH_RESIZE_LANCZOS3 };
// crh_resize_taps (host only): the taps of one axis from n source texels to m; output o reads first[o] .. first[o] + count[o] - 1 with the
// signed taps that follow each other in `taps`, and an output's taps sum to 16384
struct ResizeTaps {
    std::vector<int32_t> first;
    std::vector<uint16_t> count;
    std::vector<int16_t> taps;
};
inline ResizeTaps resize_taps(uint32_t n, uint32_t m, ResizeFilter filter = ResizeFilter::Lanczos3) {
    uint64_t total = 0;
    check(crh_resize_taps(n, m, (uint32_t)filter, nullptr, nullptr, nullptr, 0, &total));
    ResizeTaps out;
    out.first.resize(m), out.count.resize(m), out.taps.resize((size_t)total + 1u); // (+ 1: data() of an empty vector may be null)
    check(crh_resize_taps(n, m, (uint32_t)filter, out.first.data(), out.count.data(), out.taps.data(), total, nullptr));
    out.taps.resize((size_t)total);
    return out;
}
// crh_resize_texels (host only): the rule on a width x height image of RGBA8 in host memory -> the out_width x out_height result's bytes
inline std::vector<uint8_t> resize_texels(uint32_t width, uint32_t height, const std::vector<uint8_t>& texels, uint32_t out_width, uint32_t out_height, ResizeFilter filter = ResizeFilter::Lanczos3) {
    if (texels.size() != (size_t)width * height * 4u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    const bool legal = out_width >= 1u && out_width <= 16384u && out_height >= 1u && out_height <= 16384u; // (what the library refuses gets a texel's room and the library's status)
    std::vector<uint8_t> out(legal ? (size_t)out_width * out_height * 4u : 4u);
    check(crh_resize_texels(width, height, texels.data(), out_width, out_height, (uint32_t)filter, out.data()));
    return out;
}
// crh_image_stats as it is: histogram[256 * c + v] = how many texels store code v in channel c (r, g, b, a), [x0, x1) x [y0, y1) around the
// texels inside (all 0 if none is), count = their number
typedef crh_image_stats ImageStatistics;
// crh_crop_texels (host only): the rule of Image::crop on a width x height image of RGBA8 in host memory -> the out_width x out_height result's bytes
inline std::vector<uint8_t> crop_texels(uint32_t width, uint32_t height, const std::vector<uint8_t>& texels, int32_t x, int32_t y, uint32_t out_width, uint32_t out_height) {
    if (texels.size() != (size_t)width * height * 4u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    const bool legal = out_width >= 1u && out_width <= 16384u && out_height >= 1u && out_height <= 16384u; // (what the library refuses gets a texel's room and the library's status)
    std::vector<uint8_t> out(legal ? (size_t)out_width * out_height * 4u : 4u);
    check(crh_crop_texels(width, height, texels.data(), x, y, out_width, out_height, out.data()));
    return out;
}
// crh_statistics_texels (host only): the rule of Image::statistics on a width x height image of RGBA8 in host memory
inline ImageStatistics statistics_texels(uint32_t width, uint32_t height, const std::vector<uint8_t>& texels, Channel channel = Channel::A, uint32_t threshold = 1u) {
    if (texels.size() != (size_t)width * height * 4u) throw Error(CRH_ERR_INVALID_ARGUMENT);
    ImageStatistics out;
    check(crh_statistics_texels(width, height, texels.data(), (uint32_t)channel, threshold, &out));
    return out;
}
// crh_image: width x height texels of premultiplied RGBA8 on the device, row 0 = top — the bytes Frame::download hands out. One level until
// generate_mipmaps(); a minified image wants its mipmaps and Filter::NearestMipmap / LinearMipmap (include/contrast_hip.h crh_image_generate_mipmaps).
// Destroying it while a Scene's paint table names it is legal: the table keeps the pixels.
class Image {
  public:
    Image(const Renderer& renderer, uint32_t width, uint32_t height, const uint8_t* rgba8) : width_(width), height_(height) { check(crh_image_create(renderer.raw(), width, height, rgba8, &handle_)); }
    // a snapshot of what the frame shows (an RGBA8 or RGBA8-attachment frame), copied on the device
    static Image from_frame(Frame& frame) {
        Image image;
        check(crh_image_create_from_frame(frame.raw(), &image.handle_));
        check(crh_image_size(image.handle_, &image.width_, &image.height_));
        return image;
    }
    // crh_image_turbulence -> a new Image of one level, width x height, origin (0, 0): procedural noise made on the device; binary64 arithmetic
    // in a fixed order, complete on return (a synchronous call).
    static Image turbulence(const Renderer& renderer, uint32_t width, uint32_t height, const Turbulence& turbulence) {
        const crh_turbulence how = turbulence.to_c();
        Image image;
        check(crh_image_turbulence(renderer.raw(), width, height, &how, &image.handle_));
        image.width_ = width, image.height_ = height;
        return image;
    }
    ~Image() {
        if (handle_) crh_image_destroy(handle_);
    }
    Image(Image&& other) noexcept : handle_(other.handle_), width_(other.width_), height_(other.height_), origin_(other.origin_) { other.handle_ = nullptr; }
    Image(const Image&) = delete;
    Image& operator=(const Image&) = delete;
    uint32_t width() const { return width_; }
    uint32_t height() const { return height_; }
    const crh_image* raw() const { return handle_; }
    // the levels below the image, built on the device; a second call changes nothing, and a table set before the call keeps its one level
    void generate_mipmaps() { check(crh_image_generate_mipmaps(handle_)); }
    uint32_t levels() const {
        uint32_t n = 0;
        check(crh_image_level_count(handle_, &n));
        return n;
    }
    // -> the texels of level `level` (0 = the image), width * height * 4 bytes of that level's size
    std::vector<uint8_t> download_level(uint32_t level, uint32_t* width = nullptr, uint32_t* height = nullptr) const {
        uint32_t w = 0, h = 0;
        check(crh_image_download_level(handle_, level, nullptr, &w, &h));
        std::vector<uint8_t> out((size_t)w * h * 4);
        check(crh_image_download_level(handle_, level, out.data(), &w, &h));
        if (width) *width = w;
        if (height) *height = h;
        return out;
    }
    // crh_image_blur -> a new Image of one level: the separable Gaussian of this image's level 0, integer and bit-exact, complete on return (a
    // synchronous call: one wait per blur). sigma_y < 0 means sigma_x. BlurEdge::Transparent grows the result by ceil(3 sigma) on every side
    // and its origin() is (Rx, Ry); the other edges keep the size. This image is not modified.
    Image blur(float sigma_x, float sigma_y = -1.0f, BlurEdge edge = BlurEdge::Transparent) const {
        Image image;
        check(crh_image_blur(handle_, sigma_x, sigma_y < 0.0f ? sigma_x : sigma_y, (uint32_t)edge, &image.handle_));
        check(crh_image_size(image.handle_, &image.width_, &image.height_));
        if (edge == BlurEdge::Transparent) image.origin_ = {(image.width_ - width_) / 2u, (image.height_ - height_) / 2u};
        return image;
    }
    // the texel of this image over texel (0, 0) of the image it was blurred or dilated from: (0, 0) unless blur() or morphology() grew it,
    // or crop(), trim() or a frame region cut it: then it may be negative, a signed value in these 32 bits (cast each to int32_t)
    std::array<uint32_t, 2> origin() const { return origin_; }
    // crh_image_composite, called on the backdrop -> a new Image of one level, of this image's size, origin (0, 0): `source` combined with this
    // image texel by texel by a Porter-Duff operator, a blend mode and a group opacity in [0, 1]; integer and bit-exact, complete on return.
    // Source texel (0, 0) lies over this image's texel `offset` (any integers; the source is transparent outside itself). To place a
    // BlurEdge::Transparent result so that the image it was blurred from would lie at (dx, dy): offset = {dx - origin()[0], dy - origin()[1]}
    // of the source. Neither image is modified; `source` may be this image.
    Image composite(const Image& source, CompositeOp op = CompositeOp::SrcOver, BlendMode mode = BlendMode::Normal, float opacity = 1.0f, std::array<int32_t, 2> offset = {0, 0}) const {
        const crh_composite how = {(uint32_t)op, (uint32_t)mode, opacity, offset[0], offset[1]};
        Image image;
        check(crh_image_composite(handle_, source.handle_, &how, &image.handle_));
        image.width_ = width_, image.height_ = height_;
        return image;
    }
    // crh_image_color_filter -> a new Image of one level, of this image's size and origin: every texel unpremultiplied, through the matrix, then
    // through the tables, and premultiplied again; integer and bit-exact, complete on return. A null matrix or tables is the identity. A blurred
    // snapshot through ColorMatrix::flood(r, g, b, a) is a drop shadow in that colour. This image is not modified.
    Image color_filter(const ColorMatrixValues* matrix = nullptr, const ColorTables* tables = nullptr) const {
        Image image;
        check(crh_image_color_filter(handle_, matrix ? matrix->data() : nullptr, tables ? tables->data() : nullptr, &image.handle_));
        image.width_ = width_, image.height_ = height_, image.origin_ = origin_;
        return image;
    }
    // crh_image_morphology -> a new Image of one level: per channel the min (Erode) or max (Dilate) of this image's level 0 over the rectangle
    // |dx| <= radius_x, |dy| <= radius_y; exact, complete on return (a synchronous call). Dilate under BlurEdge::Transparent grows the result by
    // the radius on every side and its origin() is (radius_x, radius_y), as blur() grows; everything else keeps the size and origin (0, 0).
    // Radii end at CRH_MAX_MORPHOLOGY_RADIUS. This image is not modified.
    Image morphology(MorphologyOp op, uint32_t radius_x, uint32_t radius_y, BlurEdge edge = BlurEdge::Transparent) const {
        Image image;
        check(crh_image_morphology(handle_, (uint32_t)op, radius_x, radius_y, (uint32_t)edge, &image.handle_));
        check(crh_image_size(image.handle_, &image.width_, &image.height_));
        if (op == MorphologyOp::Dilate && edge == BlurEdge::Transparent) image.origin_ = {radius_x, radius_y};
        return image;
    }
    Image dilate(uint32_t radius_x, uint32_t radius_y, BlurEdge edge = BlurEdge::Transparent) const { return morphology(MorphologyOp::Dilate, radius_x, radius_y, edge); }
    Image dilate(uint32_t radius) const { return morphology(MorphologyOp::Dilate, radius, radius); }
    Image erode(uint32_t radius_x, uint32_t radius_y, BlurEdge edge = BlurEdge::Transparent) const { return morphology(MorphologyOp::Erode, radius_x, radius_y, edge); }
    Image erode(uint32_t radius) const { return morphology(MorphologyOp::Erode, radius, radius); }
    // crh_image_convolve -> a new Image of one level, of this image's size and origin: this image's level 0 through a kernel matrix of up to
    // 15 x 15 entries; integer and bit-exact, complete on return (a synchronous call). preserve_alpha keeps every texel's alpha and convolves
    // the unpremultiplied colours. The result has this image's size under every edge. This image is not modified.
    Image convolve(const ConvolveKernel& kernel, BlurEdge edge = BlurEdge::Pad, bool preserve_alpha = false) const {
        const crh_convolve how = kernel.to_c(edge, preserve_alpha);
        Image image;
        check(crh_image_convolve(handle_, &how, &image.handle_));
        image.width_ = width_, image.height_ = height_, image.origin_ = origin_;
        return image;
    }
    // crh_image_lighting -> a new Image of one level, of this image's size and origin: this image's alpha as a height field lit by `light` (a
    // DistantLight, a PointLight or a SpotLight); binary64 arithmetic in a fixed order, complete on return (a synchronous call). Diffuse
    // results are opaque (MULTIPLY them onto a layer), specular ones premultiplied highlights (PLUS them). This image is not modified.
    template <class Light>
    Image lighting(const Light& light, const Lighting& lighting = Lighting()) const {
        const crh_lighting how = lighting.to_c(light);
        Image image;
        check(crh_image_lighting(handle_, &how, &image.handle_));
        image.width_ = width_, image.height_ = height_, image.origin_ = origin_;
        return image;
    }
    // crh_image_displace -> a new Image of one level, of this image's size, origin (0, 0): this image read through the per-texel offsets of
    // `map`, an image of the same size and renderer; integer and bit-exact, complete on return (a synchronous call). Neither image is modified.
    Image displace(const Image& map, const Displace& displace) const {
        const crh_displace how = displace.to_c();
        Image image;
        check(crh_image_displace(handle_, map.handle_, &how, &image.handle_));
        image.width_ = width_, image.height_ = height_;
        return image;
    }
    // crh_image_transform, the raw call -> a new Image of one level, transform.width x transform.height, origin (0, 0): this image seen through
    // transform.matrix (result -> this image); positions in binary64 in a fixed order, then integers; complete on return (a synchronous call).
    // This image is not modified.
    Image resample(const Transform& transform) const {
        const crh_transform how = transform.to_c();
        Image image;
        check(crh_image_transform(handle_, &how, &image.handle_));
        image.width_ = how.width, image.height_ = how.height;
        return image;
    }
    // transform_fit, then resample: this image moved by `forward` (its coordinates -> the caller's target space) in the smallest result that
    // holds all of it; the result's origin is where the target space's (0, 0) lies in it (two's complement when negative, as a crop's).
    Image transform(const std::array<double, 9>& forward, TransformFilter filter = TransformFilter::Linear, BlurEdge edge = BlurEdge::Transparent) const {
        const TransformFit fit = transform_fit(width_, height_, forward, filter, edge);
        Image image = resample(fit.transform);
        image.origin_ = {(uint32_t)fit.origin[0], (uint32_t)fit.origin[1]};
        return image;
    }
    // transform() by a rotation of `degrees`, clockwise on the screen (y points down), about (cx, cy) in this image's coordinates; a multiple
    // of 90 uses the entries 0 and +-1 exactly.
    Image rotate(double degrees, double cx, double cy, TransformFilter filter = TransformFilter::Linear, BlurEdge edge = BlurEdge::Transparent) const {
        const double quarter = degrees / 90.0, radians = degrees * 3.14159265358979323846 / 180.0;
        double c = std::cos(radians), s = std::sin(radians);
        if (quarter == std::floor(quarter)) {
            const int turn = (int)std::fmod(std::fmod(quarter, 4.0) + 4.0, 4.0);
            c = turn == 0 ? 1.0 : turn == 2 ? -1.0 : 0.0, s = turn == 1 ? 1.0 : turn == 3 ? -1.0 : 0.0;
        }
        return transform({c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy, 0.0, 0.0, 1.0}, filter, edge);
    }
    Image rotate(double degrees, TransformFilter filter = TransformFilter::Linear, BlurEdge edge = BlurEdge::Transparent) const {
        return rotate(degrees, width_ / 2.0, height_ / 2.0, filter, edge);
    }
    // crh_image_variable_blur -> a new Image of one level, of this image's size under every edge, origin (0, 0): blur() with the taps of each
    // texel's own level, the stored code of `blur.channel` of `mask`, an image of the same size and renderer; integer and bit-exact,
    // complete on return (a synchronous call). A mask of one value gives blur()'s bytes. Neither image is modified; the mask may be this image.
    Image variable_blur(const Image& mask, const VariableBlur& blur) const {
        const crh_variable_blur how = blur.to_c();
        Image image;
        check(crh_image_variable_blur(handle_, mask.handle_, &how, &image.handle_));
        image.width_ = width_, image.height_ = height_;
        return image;
    }
    // crh_image_distance_field -> a new Image of one level: per texel the exact Euclidean distance between texel centres to the shape (or,
    // Inside, to what is not the shape), coded over the spread on all four channels; complete on return (a synchronous call). Outside under
    // BlurEdge::Transparent grows the result by the spread on every side and its origin() is (spread, spread), as blur() grows; everything
    // else keeps the size and origin (0, 0). This image is not modified.
    Image distance_field(const Distance& distance) const {
        const crh_distance how = distance.to_c();
        Image image;
        check(crh_image_distance_field(handle_, &how, &image.handle_));
        check(crh_image_size(image.handle_, &image.width_, &image.height_));
        if (distance.mode == DistanceMode::Outside && distance.edge == BlurEdge::Transparent) image.origin_ = {distance.spread, distance.spread};
        return image;
    }
    // crh_image_resize -> a new Image of one level, width x height, the whole of this image resampled; complete on return (a synchronous
    // call). Its origin() is (0, 0) whatever this image's is. An axis that shrinks by more than the filter's cap (about 85 under Lanczos3)
    // is refused: chain two calls. This image is not modified.
    Image resize(uint32_t width, uint32_t height, ResizeFilter filter = ResizeFilter::Lanczos3) const {
        Image image;
        check(crh_image_resize(handle_, width, height, (uint32_t)filter, &image.handle_));
        check(crh_image_size(image.handle_, &image.width_, &image.height_));
        return image;
    }
    // crh_image_create_from_frame_region: byte for byte from_frame(frame).crop(x, y, width, height), without the full-size copy; the
    // rectangle may leave the frame (zeros there) and only its own size is limited to 16384. Its origin() is (-x, -y).
    static Image from_frame(Frame& frame, int32_t x, int32_t y, uint32_t width, uint32_t height) {
        Image image;
        check(crh_image_create_from_frame_region(frame.raw(), x, y, width, height, &image.handle_));
        image.width_ = width, image.height_ = height, image.origin_ = {0u - (uint32_t)x, 0u - (uint32_t)y};
        return image;
    }
    // crh_image_crop -> a new Image of one level, width x height (each in [1, 16384]): texel (i, j) is this image's (x + i, y + j), the bytes
    // as stored, (0, 0, 0, 0) outside this image; complete on return (a synchronous call). x and y are any int32: a rectangle that misses
    // this image is a transparent canvas, a larger one the transparent backdrop around it. Its origin() is this image's minus (x, y): a
    // signed value in origin()'s 32 bits, read through (int32_t) as composite()'s rule does. This image is not modified.
    Image crop(int32_t x, int32_t y, uint32_t width, uint32_t height) const {
        Image image;
        check(crh_image_crop(handle_, x, y, width, height, &image.handle_));
        image.width_ = width, image.height_ = height, image.origin_ = {origin_[0] - (uint32_t)x, origin_[1] - (uint32_t)y};
        return image;
    }
    // crh_image_statistics -> the per-channel histograms of the stored codes over all texels, and the bounds and the number of the texels
    // inside: stored code of `channel` >= `threshold` (1..255), distance_field()'s definition. Reduced on the device (a synchronous call).
    ImageStatistics statistics(Channel channel = Channel::A, uint32_t threshold = 1u) const {
        ImageStatistics out;
        check(crh_image_statistics(handle_, (uint32_t)channel, threshold, &out));
        return out;
    }
    // statistics(channel, threshold)'s x0, y0, x1, y1: half-open, all 0 if no texel is inside
    std::array<uint32_t, 4> bounds(Channel channel = Channel::A, uint32_t threshold = 1u) const {
        const ImageStatistics s = statistics(channel, threshold);
        return {s.x0, s.y0, s.x1, s.y1};
    }
    // statistics(), then crop() to the bounds grown by `margin` on every side and clipped to this image; nothing inside: the 1 x 1 crop at (0, 0)
    Image trim(Channel channel = Channel::A, uint32_t threshold = 1u, uint32_t margin = 0u) const {
        const std::array<uint32_t, 4> b = bounds(channel, threshold);
        if (b[2] == b[0]) return crop(0, 0, 1u, 1u);
        const uint32_t x0 = b[0] > margin ? b[0] - margin : 0u, y0 = b[1] > margin ? b[1] - margin : 0u;
        const uint32_t x1 = b[2] + margin < width_ ? b[2] + margin : width_, y1 = b[3] + margin < height_ ? b[3] + margin : height_;
        return crop((int32_t)x0, (int32_t)y0, x1 - x0, y1 - y0);
    }
    template <class Light>
    Image diffuse_lighting(const Light& light, float surface_scale = 1.0f, float constant = 1.0f, std::array<float, 3> color = {1.0f, 1.0f, 1.0f}, BlurEdge edge = BlurEdge::Pad) const {
        Lighting how;
        how.op = LightingOp::Diffuse, how.surface_scale = surface_scale, how.constant = constant, how.color = color, how.edge = edge;
        return lighting(light, how);
    }
    template <class Light>
    Image specular_lighting(const Light& light, float surface_scale = 1.0f, float constant = 1.0f, float specular_exponent = 1.0f, std::array<float, 3> color = {1.0f, 1.0f, 1.0f},
                            BlurEdge edge = BlurEdge::Pad) const {
        Lighting how;
        how.op = LightingOp::Specular, how.surface_scale = surface_scale, how.constant = constant, how.specular_exponent = specular_exponent, how.color = color, how.edge = edge;
        return lighting(light, how);
    }

  private:
    Image() = default;
    crh_image* handle_ = nullptr;
    uint32_t width_ = 0, height_ = 0;
    std::array<uint32_t, 2> origin_ = {0u, 0u};
};
inline void Frame::load_image(const Image& image) { check(crh_frame_load_image(handle_, image.raw())); }
class ImagePaint {
  public:
    // matrix: path -> texel, u = m0 x + m1 y + m2, v = m3 x + m4 y + m5
    ImagePaint(const Image& image, const std::array<float, 6>& matrix, Filter filter = Filter::Linear, Spread spread_x = Spread::Pad, Spread spread_y = Spread::Pad) {
        c_ = crh_image_paint{};
        c_.image = image.raw(), c_.filter = (uint32_t)filter, c_.spread_x = (uint32_t)spread_x, c_.spread_y = (uint32_t)spread_y;
        for (size_t i = 0; i < 6; ++i) c_.m[i] = matrix[i];
    }
    // the path rectangle [lower, upper] onto the whole image; path y points up on the frame, so y = upper[1] is the image's row 0
    static ImagePaint fit(const Image& image, const std::array<float, 2>& lower, const std::array<float, 2>& upper, Filter filter = Filter::Linear) {
        const float sx = (float)image.width() / (upper[0] - lower[0]), sy = (float)image.height() / (upper[1] - lower[1]);
        return ImagePaint(image, {sx, 0.0f, -sx * lower[0], 0.0f, -sy, sy * upper[1]}, filter);
    }
    void validate() const { check(crh_image_paint_validate(&c_)); } // host only: throws what Scene::set_paints would
    const crh_image_paint& to_c() const { return c_; }

  private:
    crh_image_paint c_;
};

// A batch of Shapes built together (one launch tessellates all of them). Shape below is the n == 1 case with the reference's signature.
class Scene {
  public:
    Scene(Renderer& renderer, const PathBatch& batch, Scene* existing = nullptr) : n_shapes_(batch.n_shapes()) {
        const crh_path_batch view = batch.view();
        // `existing` is given up only once the upload has taken it over: a batch that fails validation leaves it with its owner
        check(crh_scene_upload(renderer.raw(), &view, existing ? existing->raw() : nullptr, &handle_));
        if (existing) {
            existing->release();
            pass_table_ = std::move(existing->pass_table_), pass_images_ = std::move(existing->pass_images_), pass_assoc_ = std::move(existing->pass_assoc_), holds_pass_table_ = existing->holds_pass_table_; // (the C scene keeps its table)
        }
        crh_status st = crh_scene_tessellate(handle_);
        if (st == CRH_OK) st = crh_scene_status(handle_); // surfaces the reference's panics at the call site, like the reference
        if (st != CRH_OK) { // a constructor that throws runs no destructor: free the handle here
            crh_scene_destroy(handle_);
            handle_ = nullptr;
            throw Error(st);
        }
    }
    ~Scene() {
        if (handle_) crh_scene_destroy(handle_);
    }
    Scene(Scene&& other) noexcept
        : handle_(other.release()), n_shapes_(other.n_shapes_), pass_table_(std::move(other.pass_table_)), pass_images_(std::move(other.pass_images_)), pass_assoc_(std::move(other.pass_assoc_)), holds_pass_table_(other.holds_pass_table_) {}
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;
    uint32_t n_shapes() const { return n_shapes_; }
    ShapeBuffers buffers(uint32_t shape) const {
        ShapeBuffers b;
        check(crh_scene_shape_layout(handle_, shape, b.vertex_offsets, b.index_offsets));
        b.vertex_bytes.resize(b.vertex_offsets[7]);
        b.index_bytes.resize(b.index_offsets[2]);
        check(crh_scene_shape_download(handle_, shape, b.vertex_bytes.data(), b.index_bytes.data()));
        return b;
    }
    // Shape::set_dynamic_stroke_options (renderer.rs:360-376)
    void set_dynamic_stroke_options(uint32_t shape, size_t dynamic_stroke_options_index, const DynamicStrokeOptions& options) {
        const crh_dynamic_stroke_options c = options.to_c();
        check(crh_scene_set_dynamic_stroke_options(handle_, shape, (uint32_t)dynamic_stroke_options_index, &c));
    }
    // Stencil + Color of every Shape in index order, instance i = Shape i (the loop of examples/showcase/main.rs:236-250)
    void render(Frame& frame, const std::vector<float>& transforms, const std::vector<float>& colors) {
        if (transforms.size() != (size_t)n_shapes_ * 16 || colors.size() != (size_t)n_shapes_ * 4) throw Error(CRH_ERR_INVALID_ARGUMENT);
        paints_of_pass({}, {}); // (a table a RenderPass left belongs to that pass's instances)
        check(crh_scene_render(handle_, frame.raw(), transforms.data(), colors.data()));
    }
    // crh_scene_set_paints: instance_paint[i] = the index into `paints` of instance i's paint, or -1 for its solid colour; stays until the next call,
    // no paints clears it. The call waits for the renderer's work in flight: set the table when it changes, not per frame.
    void set_paints(const std::vector<Paint>& paints, const std::vector<int32_t>& instance_paint) const {
        install_paints(paints, {}, instance_paint);
        holds_pass_table_ = false; // the caller's own table: passes without paints leave it alone
    }
    // crh_scene_set_paints_with_images: instance_paint[i] below paints.size() names a gradient, from there on image paint i - paints.size()
    void set_paints(const std::vector<Paint>& paints, const std::vector<ImagePaint>& image_paints, const std::vector<int32_t>& instance_paint) const {
        install_paints(paints, image_paints, instance_paint);
        holds_pass_table_ = false;
    }
    // What RenderPass::submit asks for in front of its draws: the pass's table (none: the pass has no paints). A table an earlier pass put here
    // belongs to that pass's instance numbering, so it is replaced or removed; the call is skipped when the Scene already holds this very table.
    void paints_of_pass(const std::vector<Paint>& paints, const std::vector<int32_t>& instance_paint, const std::vector<ImagePaint>& image_paints = {}) const {
        if (paints.empty() && image_paints.empty()) {
            if (holds_pass_table_) install_paints({}, {}, {});
            holds_pass_table_ = false;
            return;
        }
        bool same = holds_pass_table_ && pass_table_.size() == paints.size() && pass_images_.size() == image_paints.size() && pass_assoc_ == instance_paint;
        for (size_t i = 0; same && i < paints.size(); ++i) same = std::memcmp(&pass_table_[i], &paints[i].to_c(), sizeof(crh_paint)) == 0;
        for (size_t i = 0; same && i < image_paints.size(); ++i) same = same_image_paint(pass_images_[i], image_paints[i].to_c());
        if (same) return;
        install_paints(paints, image_paints, instance_paint);
        pass_table_.clear(), pass_images_.clear();
        for (const Paint& p : paints) pass_table_.push_back(p.to_c());
        for (const ImagePaint& p : image_paints) pass_images_.push_back(p.to_c());
        pass_assoc_ = instance_paint;
        holds_pass_table_ = true;
    }
    crh_scene* raw() const { return handle_; }
    crh_scene* release() {
        crh_scene* h = handle_;
        handle_ = nullptr;
        return h;
    }

  private:
    void install_paints(const std::vector<Paint>& paints, const std::vector<ImagePaint>& image_paints, const std::vector<int32_t>& instance_paint) const {
        std::vector<crh_paint> table;
        for (const Paint& p : paints) table.push_back(p.to_c());
        if (image_paints.empty()) { // a list without an image paint goes the way it always went
            check(crh_scene_set_paints(handle_, table.data(), (uint32_t)table.size(), instance_paint.data(), (uint32_t)instance_paint.size()));
            return;
        }
        std::vector<crh_image_paint> images;
        for (const ImagePaint& p : image_paints) images.push_back(p.to_c());
        check(crh_scene_set_paints_with_images(handle_, table.data(), (uint32_t)table.size(), images.data(), (uint32_t)images.size(), instance_paint.data(), (uint32_t)instance_paint.size()));
    }
    static bool same_image_paint(const crh_image_paint& a, const crh_image_paint& b) { // (field by field: the struct has padding)
        return a.image == b.image && a.filter == b.filter && a.spread_x == b.spread_x && a.spread_y == b.spread_y && std::memcmp(a.m, b.m, sizeof(a.m)) == 0;
    }
    crh_scene* handle_ = nullptr;
    uint32_t n_shapes_ = 0;
    // the paint table a RenderPass installed (none: the Scene holds the caller's own table, or nothing)
    mutable std::vector<crh_paint> pass_table_;
    mutable std::vector<crh_image_paint> pass_images_;
    mutable std::vector<int32_t> pass_assoc_;
    mutable bool holds_pass_table_ = false;
};

// wgpu::RenderPass stand-in: records Shape::render calls with the pass state they see and submits them as one draw list.
class RenderPass {
  public:
    RenderPass(Renderer& renderer, Frame& frame) : config_(renderer.get_config()), frame_(frame) {}
    // instance data of the pass (the instance buffers bound at slot 0 / 2, renderer.rs:462-466): returns the instance index
    uint32_t push_instance(const float (&transform)[16], const float (&color)[4]) {
        transforms_.insert(transforms_.end(), transform, transform + 16);
        colors_.insert(colors_.end(), color, color + 4);
        instance_paint_.push_back(-1);
        return (uint32_t)(colors_.size() / 4 - 1);
    }
    // ... with a paint as the source of the instance's Color covers (times `color`); the pass hands its paints to every Scene it submits to
    uint32_t push_instance(const float (&transform)[16], const float (&color)[4], const Paint& paint) {
        const uint32_t index = push_instance(transform, color);
        instance_paint_.back() = (int32_t)paints_.size();
        paints_.push_back(paint);
        return index;
    }
    // ... with an image paint: the pass numbers its gradients first and its image paints behind them when it submits
    uint32_t push_instance(const float (&transform)[16], const float (&color)[4], const ImagePaint& paint) {
        const uint32_t index = push_instance(transform, color);
        instance_paint_.back() = -2 - (int32_t)image_paints_.size(); // (-2 - k: image paint k, resolved in submit)
        image_paints_.push_back(paint);
        return index;
    }
    // Renderer::set_clip_depth (renderer.rs:932-938)
    void set_clip_depth(size_t clip_depth) {
        if (clip_depth >= ((size_t)1 << config_.clip_nesting_counter_bits)) throw Error(CRH_ERR_CLIP_STACK_OVERFLOW);
        clip_depth_ = (uint32_t)clip_depth;
    }
    // Renderer::save_alpha_context / restore_alpha_context (renderer.rs:941-985) select the layer of the following alpha-context draws
    void set_alpha_layer(size_t alpha_layer) {
        if (alpha_layer >= config_.alpha_layer_count) throw Error(CRH_ERR_TOO_MANY_NESTED_OPACITY_GROUPS);
        alpha_layer_ = (uint32_t)alpha_layer;
    }
    // Shape::render(&renderer, &mut render_pass, instance_indices, render_operation) (renderer.rs:267-273) for Shape `shape` of `scene`
    // The Scenes / Shapes of a pass may be different objects: the frame keeps clip nesting counters, winding counters, saved alphas and sample
    // colours between the submissions, as the caller-owned stencil attachment and alpha layers of the reference do (renderer.rs:148-158, 257-266).
    void render(const Scene& scene, uint32_t shape, uint32_t first_instance, uint32_t end_instance, RenderOperation op) {
        for (uint32_t i = first_instance; i < end_instance; ++i) {
            draws_.push_back(crh_draw{shape, i, (uint32_t)op, clip_depth_, alpha_layer_});
            scenes_.push_back(&scene);
        }
    }
    // end of the pass: everything recorded executes in order, one crh_scene_render_draws per run of draws of the same object
    void submit() {
        for (const Scene* scene : scenes_)
            if (scene != scenes_.front()) {
                frame_.keep_pass_state(); // the pass spans objects: every sample's colour and stencil stay with the frame from its first draw on
                break;
            }
        for (size_t begin = 0; begin < draws_.size();) {
            size_t end = begin;
            while (end < draws_.size() && scenes_[end] == scenes_[begin]) ++end;
            std::vector<int32_t> association = instance_paint_;
            for (int32_t& k : association)
                if (k <= -2) k = (int32_t)paints_.size() + (-2 - k);
            scenes_[begin]->paints_of_pass(paints_, association, image_paints_); // (a pass without paints removes what an earlier pass installed)
            check(crh_scene_render_draws(scenes_[begin]->raw(), frame_.raw(), transforms_.data(), colors_.data(), (uint32_t)(colors_.size() / 4), draws_.data() + begin, (uint32_t)(end - begin)));
            begin = end;
        }
        draws_.clear();
        scenes_.clear();
    }

  private:
    Configuration config_;
    Frame& frame_;
    std::vector<float> transforms_, colors_;
    std::vector<Paint> paints_;
    std::vector<ImagePaint> image_paints_;
    std::vector<int32_t> instance_paint_; // per instance: index into paints_, or -1
    std::vector<crh_draw> draws_;
    std::vector<const Scene*> scenes_; // the object every draw belongs to
    uint32_t clip_depth_ = 0, alpha_layer_ = 0;
};

// Shape (renderer.rs:163-171): `Shape::from_paths(&device, &renderer, &dynamic_stroke_options, &paths, existing_shape)` (renderer.rs:177-183)
class Shape : public Scene {
  public:
    static Shape from_paths(Renderer& renderer, const std::vector<DynamicStrokeOptions>& dynamic_stroke_options, const std::vector<Path>& paths,
                            Shape* existing_shape = nullptr) {
        PathBatch batch;
        batch.add_shape(dynamic_stroke_options, paths);
        return Shape(renderer, batch, existing_shape);
    }
    ShapeBuffers buffers() const { return Scene::buffers(0); }
    void set_dynamic_stroke_options(size_t dynamic_stroke_options_index, const DynamicStrokeOptions& options) { // renderer.rs:360-376
        Scene::set_dynamic_stroke_options(0, dynamic_stroke_options_index, options);
    }
    // Shape::render for one pass: see RenderPass::render(scene, 0, instances..., op)
    void render(RenderPass& pass, uint32_t first_instance, uint32_t end_instance, RenderOperation op) const { pass.render(*this, 0, first_instance, end_instance, op); }

  private:
    Shape(Renderer& renderer, const PathBatch& batch, Shape* existing) : Scene(renderer, batch, existing) {}
};

// ---------------------------------------------------------------------------------------------- text.rs
enum class Orientation : uint32_t { RightToLeft = 0, LeftToRight = 1, TopToBottom = 2, BottomToTop = 3 }; // :106-117
enum class Alignment : uint32_t { Begin = 0, Baseline = 1, Center = 2, End = 3 };                       // :119-131
struct Layout {                                                                                         // :133-143
    float size;
    Orientation orientation = Orientation::LeftToRight;
    Alignment major_alignment = Alignment::Begin, minor_alignment = Alignment::Baseline;
};

class Font { // text.rs:11-38; face() of the reference returns the parsed ttf_parser::Face — here the Font is the face
  public:
    Font(std::string name, const std::vector<uint8_t>& font_data) : name_(std::move(name)) { check(crh_font_create(font_data.data(), font_data.size(), &handle_)); }
    ~Font() { crh_font_destroy(handle_); }
    Font(const Font&) = delete;
    Font& operator=(const Font&) = delete;
    const std::string& name() const { return name_; }
    const Font& face() const { return *this; }
    crh_font_metrics metrics() const {
        crh_font_metrics m;
        check(crh_font_get_metrics(handle_, &m));
        return m;
    }
    std::optional<uint16_t> glyph_index(char32_t c) const {
        uint16_t glyph;
        uint32_t found;
        check(crh_font_glyph_index(handle_, (uint32_t)c, &glyph, &found));
        return found ? std::optional<uint16_t>(glyph) : std::nullopt;
    }
    crh_font* raw() const { return handle_; }

  private:
    std::string name_;
    crh_font* handle_ = nullptr;
};

// ---- utils.rs:168-203: column-major 4x4 matrices as the instance buffer holds them (shaders.wgsl:13-27), element [4 * column + row]
using Mat4 = std::array<float, 16>;
inline Mat4 perspective_projection(float field_of_view_y, float aspect_ratio, float near, float far) { // utils.rs:181-192
    const float height = 1.0f / std::tan(field_of_view_y * 0.5f), denominator = 1.0f / (near - far);
    Mat4 m{};
    m[0] = height / aspect_ratio;
    m[5] = height;
    m[10] = -far * denominator;
    m[11] = 1.0f;
    m[14] = near * far * denominator;
    return m;
}
inline Mat4 matrix_multiplication(const Mat4& a, const Mat4& b) { // utils.rs:194-203: a * b, accumulated left to right like the reference
    Mat4 out{};
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            float acc = a[r] * b[4 * c];
            for (int k = 1; k < 4; ++k) acc = acc + a[4 * k + r] * b[4 * c + k];
            out[4 * c + r] = acc;
        }
    return out;
}
inline Mat4 translation_matrix(float x, float y, float z) { // what motor3d_to_mat4 (utils.rs:168-179) yields for a pure translator
    Mat4 m{};
    m[0] = m[5] = m[10] = m[15] = 1.0f;
    m[12] = x, m[13] = y, m[14] = z;
    return m;
}

namespace detail {
inline std::vector<Path> take_paths(crh_path_list* list) {
    crh_path_batch view;
    const crh_status st = crh_path_list_view(list, &view);
    std::vector<Path> out;
    if (st == CRH_OK) {
        static const int floats[5] = {2, 4, 6, 5, 10};
        size_t at = 0;
        for (uint32_t p = 0; p < view.n_paths; ++p) {
            Path path;
            path.start = Vec2{view.path_start[2 * p], view.path_start[2 * p + 1]};
            for (uint32_t s = view.path_segment_begin[p]; s < view.path_segment_begin[p + 1]; ++s) {
                path.segment_types.push_back((SegmentType)view.segment_types[s]);
                path.control.insert(path.control.end(), view.control_data + at, view.control_data + at + floats[view.segment_types[s]]);
                at += floats[view.segment_types[s]];
            }
            out.push_back(std::move(path));
        }
    }
    crh_path_list_destroy(list);
    check(st);
    return out;
}
} // namespace detail

inline std::vector<Path> paths_of_glyph(const Font& face, uint16_t glyph_id) { // text.rs:97-104
    crh_path_list* list = nullptr;
    check(crh_paths_of_glyph(face.raw(), glyph_id, &list));
    return detail::take_paths(list);
}
// text.rs:236-263; clipping_area = clockwise convex polygon of (x, y) pairs, or empty
inline std::vector<Path> paths_of_text(const Font& face, const Layout& layout, const std::u32string& text, const std::vector<Vec2>& clipping_area = {}) {
    const crh_text_layout c = {layout.size, (uint32_t)layout.orientation, (uint32_t)layout.major_alignment, (uint32_t)layout.minor_alignment};
    std::vector<float> clip;
    for (const Vec2& p : clipping_area) clip.push_back(p.first), clip.push_back(p.second);
    crh_path_list* list = nullptr;
    check(crh_paths_of_text(face.raw(), &c, reinterpret_cast<const uint32_t*>(text.data()), text.size(), clip.empty() ? nullptr : clip.data(), clip.size() / 2, &list));
    return detail::take_paths(list);
}

// text.rs:266-347: bounding box of the entire text and the glyph positions of its characters, line by line
struct TextGeometry {
    size_t major_axis;                                           // 0 horizontal, 1 vertical
    Vec2 half_extent;
    std::vector<std::pair<size_t, std::vector<Vec2>>> lines;     // (line_range_end, glyph positions incl. the line break)

    static TextGeometry make(const Font& face, const Layout& layout, const std::u32string& text) { // TextGeometry::new, text.rs:284-307
        const crh_text_layout c = {layout.size, (uint32_t)layout.orientation, (uint32_t)layout.major_alignment, (uint32_t)layout.minor_alignment};
        const uint32_t* chars = reinterpret_cast<const uint32_t*>(text.data());
        uint64_t n_lines = 0;
        check(crh_text_aligned_positions(face.raw(), &c, chars, text.size(), nullptr, nullptr, nullptr, nullptr, nullptr, &n_lines));
        int64_t extent[2], offset[2];
        std::vector<int64_t> positions((text.size() + 1) * 3);
        std::vector<uint64_t> ends(n_lines), lengths(n_lines);
        check(crh_text_aligned_positions(face.raw(), &c, chars, text.size(), extent, offset, positions.data(), ends.data(), lengths.data(), &n_lines));
        TextGeometry g;
        g.major_axis = (layout.orientation == Orientation::RightToLeft || layout.orientation == Orientation::LeftToRight) ? 0 : 1;
        const float scale = layout.size / (float)face.metrics().height;
        g.half_extent = {(float)extent[0] * scale * 0.5f, (float)extent[1] * scale * 0.5f};
        size_t at = 0;
        for (uint64_t l = 0; l < n_lines; ++l) {
            std::vector<Vec2> line;
            for (uint64_t i = 0; i < lengths[l]; ++i, ++at)
                line.push_back({(float)(positions[at * 3] - offset[0]) * scale, (float)(positions[at * 3 + 1] - offset[1]) * scale});
            g.lines.emplace_back((size_t)ends[l], std::move(line));
        }
        return g;
    }
    size_t line_index_from_char_index(size_t char_index) const { // text.rs:310-315 (the reference unwraps: out of range throws here)
        for (size_t i = 0; i < lines.size(); ++i)
            if (lines[i].first > char_index) return i;
        throw Error(CRH_ERR_INVALID_ARGUMENT);
    }
    size_t char_index_from_position(Vec2 cursor) const { // text.rs:318-331
        const auto axis = [](const Vec2& v, size_t a) { return a == 0 ? v.first : v.second; };
        const float minor_half_extent = axis(half_extent, 1 - major_axis);
        float v = (minor_half_extent - axis(cursor, 1 - major_axis)) * (float)lines.size() / (minor_half_extent * 2.0f);
        v = std::fmin(std::fmax(v, 0.0f), (float)(lines.size() - 1)); // f32::max / min return the other operand for NaN
        const size_t line_index = (size_t)v;
        const std::vector<Vec2>& glyph_positions = lines[line_index].second;
        size_t found = glyph_positions.size() - 1;
        for (size_t i = 0; i + 1 < glyph_positions.size(); ++i)
            if ((axis(glyph_positions[i], major_axis) + axis(glyph_positions[i + 1], major_axis)) * 0.5f > axis(cursor, major_axis)) {
                found = i;
                break;
            }
        return found + (line_index == 0 ? 0 : lines[line_index - 1].first);
    }
    size_t advance_char_index_by_line_index(size_t char_index, ptrdiff_t relative_line_index) const { // text.rs:334-346
        const size_t line_index = line_index_from_char_index(char_index);
        if (relative_line_index < 0 && line_index == 0) return 0;
        if (relative_line_index > 0 && line_index == lines.size() - 1) return lines.back().first - 1;
        const std::vector<Vec2>& glyph_positions = lines[line_index].second;
        Vec2 cursor = glyph_positions[char_index + glyph_positions.size() - lines[line_index].first];
        const float line_minor_extent = (major_axis == 0 ? half_extent.second : half_extent.first) * 2.0f / (float)lines.size();
        (major_axis == 0 ? cursor.second : cursor.first) -= line_minor_extent * (float)relative_line_index;
        return char_index_from_position(cursor);
    }
};
inline size_t byte_offset_of_char_index(const std::string& utf8, size_t char_index) { // text.rs:350-352
    size_t chars = 0;
    for (size_t i = 0; i < utf8.size(); ++i)
        if (((unsigned char)utf8[i] & 0xC0u) != 0x80u && chars++ == char_index) return i;
    return utf8.size();
}

} // namespace contrast_renderer
