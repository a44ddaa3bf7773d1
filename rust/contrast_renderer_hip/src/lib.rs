//! contrast_renderer's `Renderer` / `Shape` / `Path` API (Lichtso/contrast_renderer v0.1.4) over `libcontrast_hip.so`.
//!
//! The reference tessellates on the CPU (`stroke.rs`, `fill.rs`, `convex_hull.rs`) and rasterises through wgpu (`shaders.wgsl`); this
//! crate keeps its public types and call order and sends the work to hand-written HIP kernels for MI355X through the C ABI of
//! `include/contrast_hip.h` (raw bindings: [`ffi`], generated from that header). What changes for a caller:
//!
//! * `&wgpu::Device` becomes the HIP device ordinal given to [`Renderer::new`]; `&wgpu::Queue` disappears (uploads are ordered on
//!   the renderer's own HIP streams);
//! * the caller-owned `wgpu::RenderPass` becomes [`RenderPass`], which records `Shape::render` calls in order and submits them as one
//!   pass over a [`Frame`] (the colour + depth / stencil attachments);
//! * `SafeFloat<f32, N>` fields are plain `[f32; N]` / `f32` here: the library validates finiteness and canonicalises `-0.0` on
//!   upload, where the reference does it in `SafeFloat::from` (`safe_float.rs:44-52`).
//!
//! Statuses 1..=5 are the reference's [`Error`] variants in declaration order (`error.rs:5-16`). What the reference *panics* on
//! (non-finite input `safe_float.rs:46`, degenerate cubics `fill.rs:174,178`) panics here too, with the library's message.
//!
//! NOTE: the image this crate was written in has no Rust toolchain; the crate ships as source. Its raw bindings are generated from the
//! header and checked against it by `tests/test_rust_shim.py`; the tested callers of the same ABI are the C++ and Python mirrors.
pub mod ffi;

use std::ffi::CStr;
use std::ops::Range;
use std::ptr;

/// error.rs:5-16, same order
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Error {
    NumberOfStencilBitsIsUnsupported,
    ClipStackOverflow,
    TooManyNestedOpacityGroups,
    TooManyDashIntervals,
    DynamicStrokeOptionsIndexOutOfBounds,
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(ffi::crh_last_error()) }.to_string_lossy().into_owned()
}

fn status(code: ffi::crh_status) -> Result<(), Error> {
    match code {
        ffi::CRH_OK => Ok(()),
        ffi::CRH_ERR_NUMBER_OF_STENCIL_BITS_IS_UNSUPPORTED => Err(Error::NumberOfStencilBitsIsUnsupported),
        ffi::CRH_ERR_CLIP_STACK_OVERFLOW => Err(Error::ClipStackOverflow),
        ffi::CRH_ERR_TOO_MANY_NESTED_OPACITY_GROUPS => Err(Error::TooManyNestedOpacityGroups),
        ffi::CRH_ERR_TOO_MANY_DASH_INTERVALS => Err(Error::TooManyDashIntervals),
        ffi::CRH_ERR_DYNAMIC_STROKE_OPTIONS_INDEX_OUT_OF_BOUNDS => Err(Error::DynamicStrokeOptionsIndexOutOfBounds),
        // the reference panics where the library reports 6 (safe_float.rs:46,114) and 7 (fill.rs:174,178); 8.. are not reference states
        other => panic!("contrast_hip status {}: {}", other, last_error()),
    }
}

// ------------------------------------------------------------------------------------------------ path.rs

/// path.rs:15-18
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct LineSegment {
    pub control_points: [[f32; 2]; 1],
}
/// path.rs:22-25
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct IntegralQuadraticCurveSegment {
    pub control_points: [[f32; 2]; 2],
}
/// path.rs:29-32
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct IntegralCubicCurveSegment {
    pub control_points: [[f32; 2]; 3],
}
/// path.rs:36-43
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct RationalQuadraticCurveSegment {
    pub weight: f32,
    pub control_points: [[f32; 2]; 2],
}
/// path.rs:47-52
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct RationalCubicCurveSegment {
    pub weights: [f32; 4],
    pub control_points: [[f32; 2]; 3],
}
/// path.rs:56-67 (discriminants = CRH_SEGMENT_*)
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum SegmentType {
    Line = 0,
    IntegralQuadraticCurve = 1,
    IntegralCubicCurve = 2,
    RationalQuadraticCurve = 3,
    RationalCubicCurve = 4,
}
/// path.rs:71-82
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Join {
    Miter = 0,
    Bevel = 1,
    Round = 2,
}
/// path.rs:86-101
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Cap {
    Square = 0,
    Round = 1,
    Out = 2,
    In = 3,
    Right = 4,
    Left = 5,
    Butt = 6,
}
/// path.rs:105-118
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct DashInterval {
    pub gap_start: f32,
    pub gap_end: f32,
    pub dash_start: Cap,
    pub dash_end: Cap,
}
/// path.rs:121
pub const MAX_DASH_INTERVALS: usize = ffi::CRH_MAX_DASH_INTERVALS;
/// path.rs:127-149
#[derive(Debug, Clone, PartialEq)]
pub enum DynamicStrokeOptions {
    Dashed { join: Join, pattern: Vec<DashInterval>, phase: f32 },
    Solid { join: Join, start: Cap, end: Cap },
}
/// path.rs:153-167
#[derive(Debug, Clone, Copy, PartialEq)]
pub enum CurveApproximation {
    UniformlySpacedParameters(usize),
    UniformTangentAngle(f32),
}
/// path.rs:171-192
#[derive(Debug, Clone, PartialEq)]
pub struct StrokeOptions {
    pub width: f32,
    pub offset: f32,
    pub miter_clip: f32,
    pub closed: bool,
    pub dynamic_stroke_options_group: usize,
    pub curve_approximation: CurveApproximation,
}
impl StrokeOptions {
    /// path.rs:196-200
    pub fn legalize(&mut self) {
        self.width = self.width.abs();
        self.offset = self.offset.clamp(-0.5, 0.5);
        self.miter_clip = self.miter_clip.abs();
    }
}
/// path.rs:213-230
#[derive(Default, Debug, Clone, PartialEq)]
pub struct Path {
    pub stroke_options: Option<StrokeOptions>,
    pub start: [f32; 2],
    pub line_segments: Vec<LineSegment>,
    pub integral_quadratic_curve_segments: Vec<IntegralQuadraticCurveSegment>,
    pub integral_cubic_curve_segments: Vec<IntegralCubicCurveSegment>,
    pub rational_quadratic_curve_segments: Vec<RationalQuadraticCurveSegment>,
    pub rational_cubic_curve_segments: Vec<RationalCubicCurveSegment>,
    pub segment_types: Vec<SegmentType>,
}
impl Path {
    /// path.rs:232-236 and the push_* family :240-318
    pub fn push_line(&mut self, segment: LineSegment) {
        self.line_segments.push(segment);
        self.segment_types.push(SegmentType::Line);
    }
    pub fn push_integral_quadratic_curve(&mut self, segment: IntegralQuadraticCurveSegment) {
        self.integral_quadratic_curve_segments.push(segment);
        self.segment_types.push(SegmentType::IntegralQuadraticCurve);
    }
    pub fn push_integral_cubic_curve(&mut self, segment: IntegralCubicCurveSegment) {
        self.integral_cubic_curve_segments.push(segment);
        self.segment_types.push(SegmentType::IntegralCubicCurve);
    }
    pub fn push_rational_quadratic_curve(&mut self, segment: RationalQuadraticCurveSegment) {
        self.rational_quadratic_curve_segments.push(segment);
        self.segment_types.push(SegmentType::RationalQuadraticCurve);
    }
    pub fn push_rational_cubic_curve(&mut self, segment: RationalCubicCurveSegment) {
        self.rational_cubic_curve_segments.push(segment);
        self.segment_types.push(SegmentType::RationalCubicCurve);
    }
}

fn convert_dynamic(options: &DynamicStrokeOptions) -> ffi::crh_dynamic_stroke_options {
    let empty = ffi::crh_dash_interval { gap_start: 0.0, gap_end: 0.0, dash_start: 0, dash_end: 0 };
    let mut out = ffi::crh_dynamic_stroke_options { dashed: 0, join: 0, pattern_len: 0, pattern: [empty; ffi::CRH_MAX_DASH_INTERVALS], phase: 0.0, start: 0, end: 0 };
    match options {
        DynamicStrokeOptions::Dashed { join, pattern, phase } => {
            out.dashed = 1;
            out.join = *join as u32;
            out.pattern_len = pattern.len() as u32; // > MAX_DASH_INTERVALS comes back as TooManyDashIntervals (renderer.rs:32-34)
            for (slot, interval) in out.pattern.iter_mut().zip(pattern.iter()) {
                *slot = ffi::crh_dash_interval { gap_start: interval.gap_start, gap_end: interval.gap_end, dash_start: interval.dash_start as u32, dash_end: interval.dash_end as u32 };
            }
            out.phase = *phase;
        }
        DynamicStrokeOptions::Solid { join, start, end } => {
            out.join = *join as u32;
            out.start = *start as u32;
            out.end = *end as u32;
        }
    }
    out
}

fn convert_stroke(options: &StrokeOptions) -> ffi::crh_stroke_options {
    let (curve_approximation, steps, angle_step) = match options.curve_approximation {
        CurveApproximation::UniformlySpacedParameters(steps) => (ffi::CRH_CURVE_UNIFORMLY_SPACED_PARAMETERS, steps as u32, 0.0),
        CurveApproximation::UniformTangentAngle(angle_step) => (ffi::CRH_CURVE_UNIFORM_TANGENT_ANGLE, 0, angle_step),
    };
    ffi::crh_stroke_options {
        width: options.width,
        offset: options.offset,
        miter_clip: options.miter_clip,
        closed: options.closed as u32,
        dynamic_stroke_options_group: options.dynamic_stroke_options_group as u32,
        curve_approximation,
        steps,
        angle_step,
    }
}

/// `&[Path]` of one or more Shapes flattened into the struct-of-arrays batch of the C ABI (segment order = `Path::segment_types`, record
/// layouts = path.rs:15-52). Owns the vectors the `crh_path_batch` view points into.
#[derive(Default)]
pub struct PathBatch {
    shape_path_begin: Vec<u32>,
    path_segment_begin: Vec<u32>,
    path_start: Vec<f32>,
    path_stroke_options: Vec<i32>,
    segment_types: Vec<u8>,
    control_data: Vec<f32>,
    stroke_options: Vec<ffi::crh_stroke_options>,
    shape_dynamic_begin: Vec<u32>,
    dynamic_stroke_options: Vec<ffi::crh_dynamic_stroke_options>,
}
impl PathBatch {
    pub fn new() -> Self {
        Self { shape_path_begin: vec![0], path_segment_begin: vec![0], shape_dynamic_begin: vec![0], ..Default::default() }
    }
    /// Appends one Shape (the arguments of `Shape::from_paths`, renderer.rs:180-181).
    pub fn push_shape(&mut self, dynamic_stroke_options: &[DynamicStrokeOptions], paths: &[Path]) {
        for path in paths {
            self.path_start.extend_from_slice(&path.start);
            let mut line = path.line_segments.iter();
            let mut integral_quadratic = path.integral_quadratic_curve_segments.iter();
            let mut integral_cubic = path.integral_cubic_curve_segments.iter();
            let mut rational_quadratic = path.rational_quadratic_curve_segments.iter();
            let mut rational_cubic = path.rational_cubic_curve_segments.iter();
            for segment_type in &path.segment_types {
                self.segment_types.push(*segment_type as u8);
                match segment_type {
                    SegmentType::Line => {
                        for point in &line.next().unwrap().control_points {
                            self.control_data.extend_from_slice(point);
                        }
                    }
                    SegmentType::IntegralQuadraticCurve => {
                        for point in &integral_quadratic.next().unwrap().control_points {
                            self.control_data.extend_from_slice(point);
                        }
                    }
                    SegmentType::IntegralCubicCurve => {
                        for point in &integral_cubic.next().unwrap().control_points {
                            self.control_data.extend_from_slice(point);
                        }
                    }
                    SegmentType::RationalQuadraticCurve => {
                        let segment = rational_quadratic.next().unwrap();
                        self.control_data.push(segment.weight);
                        for point in &segment.control_points {
                            self.control_data.extend_from_slice(point);
                        }
                    }
                    SegmentType::RationalCubicCurve => {
                        let segment = rational_cubic.next().unwrap();
                        self.control_data.extend_from_slice(&segment.weights);
                        for point in &segment.control_points {
                            self.control_data.extend_from_slice(point);
                        }
                    }
                }
            }
            self.path_segment_begin.push(self.segment_types.len() as u32);
            self.path_stroke_options.push(match &path.stroke_options {
                None => -1,
                Some(options) => {
                    self.stroke_options.push(convert_stroke(options));
                    self.stroke_options.len() as i32 - 1
                }
            });
        }
        self.shape_path_begin.push(self.path_stroke_options.len() as u32);
        self.dynamic_stroke_options.extend(dynamic_stroke_options.iter().map(convert_dynamic));
        self.shape_dynamic_begin.push(self.dynamic_stroke_options.len() as u32);
    }
    pub fn shape_count(&self) -> usize {
        self.shape_path_begin.len() - 1
    }
    fn view(&self) -> ffi::crh_path_batch {
        ffi::crh_path_batch {
            n_shapes: self.shape_count() as u32,
            shape_path_begin: self.shape_path_begin.as_ptr(),
            n_paths: self.path_stroke_options.len() as u32,
            path_segment_begin: self.path_segment_begin.as_ptr(),
            path_start: self.path_start.as_ptr(),
            path_stroke_options: self.path_stroke_options.as_ptr(),
            n_segments: self.segment_types.len() as u32,
            segment_types: self.segment_types.as_ptr(),
            control_data: self.control_data.as_ptr(),
            n_control_floats: self.control_data.len() as u32,
            n_stroke_options: self.stroke_options.len() as u32,
            stroke_options: self.stroke_options.as_ptr(),
            shape_dynamic_begin: self.shape_dynamic_begin.as_ptr(),
            n_dynamic_stroke_options: self.dynamic_stroke_options.len() as u32,
            dynamic_stroke_options: self.dynamic_stroke_options.as_ptr(),
        }
    }
}

// ------------------------------------------------------------------------------------------------ renderer.rs

/// renderer.rs:145-160, same order (= crh_render_op)
#[derive(Clone, Copy, PartialOrd, Ord, PartialEq, Eq, Debug)]
pub enum RenderOperation {
    Stencil = 0,
    Clip = 1,
    UnClip = 2,
    Color = 3,
    SaveAlphaContext = 4,
    ScaleAlphaContext = 5,
    RestoreAlphaContext = 6,
}

/// `Option<wgpu::Face>` of `Configuration::cull_mode`; front = counter-clockwise on screen (renderer.rs:477)
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum Face {
    Front = 1,
    Back = 2,
}
/// `wgpu::CompareFunction` of `Configuration::depth_compare` (fragment depth OP stored depth)
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum CompareFunction {
    Always = 0,
    Never = 1,
    Less = 2,
    Equal = 3,
    LessEqual = 4,
    Greater = 5,
    NotEqual = 6,
    GreaterEqual = 7,
}

/// `wgpu::BlendFactor`, same order (= crh_blend_factor); `Renderer::new` refuses the dual-source factors (status 8, a panic: no reference variant)
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum BlendFactor {
    Zero = 0,
    One = 1,
    Src = 2,
    OneMinusSrc = 3,
    SrcAlpha = 4,
    OneMinusSrcAlpha = 5,
    Dst = 6,
    OneMinusDst = 7,
    DstAlpha = 8,
    OneMinusDstAlpha = 9,
    SrcAlphaSaturated = 10,
    Constant = 11,
    OneMinusConstant = 12,
    Src1 = 13,
    OneMinusSrc1 = 14,
    Src1Alpha = 15,
    OneMinusSrc1Alpha = 16,
}
/// `wgpu::BlendOperation` (= crh_blend_operation)
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum BlendOperation {
    Add = 0,
    Subtract = 1,
    ReverseSubtract = 2,
    Min = 3,
    Max = 4,
}
/// `wgpu::BlendComponent`
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub struct BlendComponent {
    pub src_factor: BlendFactor,
    pub dst_factor: BlendFactor,
    pub operation: BlendOperation,
}
impl BlendComponent {
    pub const REPLACE: Self = Self { src_factor: BlendFactor::One, dst_factor: BlendFactor::Zero, operation: BlendOperation::Add };
    pub const OVER: Self = Self { src_factor: BlendFactor::One, dst_factor: BlendFactor::OneMinusSrcAlpha, operation: BlendOperation::Add };
    fn raw(&self) -> ffi::crh_blend_component {
        ffi::crh_blend_component { src_factor: self.src_factor as u32, dst_factor: self.dst_factor as u32, operation: self.operation as u32 }
    }
}
/// `wgpu::BlendState`
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub struct BlendState {
    pub color: BlendComponent,
    pub alpha: BlendComponent,
}
impl BlendState {
    pub const REPLACE: Self = Self { color: BlendComponent::REPLACE, alpha: BlendComponent::REPLACE };
    pub const ALPHA_BLENDING: Self = Self {
        color: BlendComponent { src_factor: BlendFactor::SrcAlpha, dst_factor: BlendFactor::OneMinusSrcAlpha, operation: BlendOperation::Add },
        alpha: BlendComponent::OVER,
    };
    pub const PREMULTIPLIED_ALPHA_BLENDING: Self = Self { color: BlendComponent::OVER, alpha: BlendComponent::OVER };
}
/// `wgpu::ColorWrites` bits
pub struct ColorWrites;
impl ColorWrites {
    pub const RED: u32 = 1;
    pub const GREEN: u32 = 2;
    pub const BLUE: u32 = 4;
    pub const ALPHA: u32 = 8;
    pub const COLOR: u32 = 7;
    pub const ALL: u32 = 15;
}
/// `wgpu::TextureFormat` of the colour target. The value is the frame format that keeps f32 colours within a pass; [`TextureFormat::attachment`]
/// is the one that rounds every write, as a hardware blender does.
#[repr(u32)]
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum TextureFormat {
    Rgba8Unorm = ffi::CRH_FORMAT_RGBA8,
    Bgra8Unorm = ffi::CRH_FORMAT_BGRA8,
    Rgba8UnormSrgb = ffi::CRH_FORMAT_RGBA8_SRGB,
    Bgra8UnormSrgb = ffi::CRH_FORMAT_BGRA8_SRGB,
}
impl TextureFormat {
    pub fn attachment(self) -> u32 {
        match self {
            TextureFormat::Rgba8Unorm => ffi::CRH_FORMAT_RGBA8_ATTACHMENT,
            other => other as u32 + 1,
        }
    }
}
/// `wgpu::ColorTargetState` (`blend: None` = replace). `constant` stands for `RenderPass::set_blend_constant`, which this library keeps with
/// the renderer. `format` is kept host-side: the format [`Frame::new`] creates (the C ABI names a frame's format at `crh_frame_create_format`).
#[derive(Clone, Copy, PartialEq, Debug)]
pub struct ColorTargetState {
    pub blend: Option<BlendState>,
    pub write_mask: u32,
    pub constant: [f32; 4],
    pub format: TextureFormat,
}
impl ColorTargetState {
    fn raw(&self) -> ffi::crh_color_target_state {
        let b = self.blend.unwrap_or(BlendState::REPLACE);
        ffi::crh_color_target_state { blend_enabled: self.blend.is_some() as u32, color: b.color.raw(), alpha: b.alpha.raw(), write_mask: self.write_mask, constant: self.constant }
    }
}

/// renderer.rs:380-405. `blending` = the colour cover's blend state (None: the premultiplied "over" of examples/showcase/main.rs:32-43);
/// `depth_stencil_format` and `color_attachment_in_stencil_pass` are wgpu details without meaning for a compute rasterizer.
/// `msaa_sample_count`: 1, 2, 4 or 8, at the standard sample locations (Vulkan / D3D, listed in include/contrast_hip.h); the library
/// reports CRH_ERR_UNSUPPORTED for any other count (a panic here, as for every status that is not a reference error).
#[derive(Clone, Copy, Debug)]
pub struct Configuration {
    pub cull_mode: Option<Face>,
    pub depth_compare: CompareFunction,
    pub depth_write_enabled: bool,
    pub msaa_sample_count: u32,
    pub clip_nesting_counter_bits: usize,
    pub winding_counter_bits: usize,
    pub alpha_layer_count: usize,
    pub blending: Option<ColorTargetState>,
}
impl Default for Configuration {
    /// examples/showcase/main.rs:45-56
    fn default() -> Self {
        Self {
            cull_mode: None,
            depth_compare: CompareFunction::Always,
            depth_write_enabled: false,
            msaa_sample_count: 4,
            clip_nesting_counter_bits: 4,
            winding_counter_bits: 4,
            alpha_layer_count: 0,
            blending: None,
        }
    }
}

/// renderer.rs:408
pub struct Renderer {
    raw: *mut ffi::crh_renderer,
    config: Configuration,
}
impl Renderer {
    /// renderer.rs:432 — `device` is the HIP device ordinal where the reference takes `&wgpu::Device`
    pub fn new(device: i32, config: Configuration) -> Result<Self, Error> {
        let c = ffi::crh_config {
            msaa_sample_count: config.msaa_sample_count,
            clip_nesting_counter_bits: config.clip_nesting_counter_bits as u32,
            winding_counter_bits: config.winding_counter_bits as u32,
            alpha_layer_count: config.alpha_layer_count as u32,
            cull_mode: config.cull_mode.map_or(ffi::CRH_CULL_NONE, |face| face as u32),
            depth_compare: config.depth_compare as u32,
            depth_write_enabled: config.depth_write_enabled as u32,
        };
        let mut raw = ptr::null_mut();
        let blending = config.blending.map(|b| b.raw());
        let blending_ptr = blending.as_ref().map_or(ptr::null(), |b| b as *const ffi::crh_color_target_state);
        status(unsafe { ffi::crh_renderer_create_blended(&c, blending_ptr, device, &mut raw) })?;
        Ok(Self { raw, config })
    }
    /// renderer.rs:887
    pub fn get_config(&self) -> &Configuration {
        &self.config
    }
    pub fn synchronize(&self) {
        status(unsafe { ffi::crh_renderer_synchronize(self.raw) }).unwrap()
    }
}
impl Drop for Renderer {
    fn drop(&mut self) {
        unsafe { ffi::crh_renderer_destroy(self.raw) }
    }
}

/// The colour attachment (premultiplied; RGBA8, BGRA8 or their sRGB forms) plus the depth / stencil attachments of a render pass: caller-owned in
/// the reference (`wgpu::TextureView`s handed to `begin_render_pass`), an object of the library here.
pub struct Frame {
    raw: *mut ffi::crh_frame,
    width: u32,
    height: u32,
}
impl Frame {
    /// In the format of the renderer's `Configuration::blending` (`Rgba8Unorm` without one)
    pub fn new(renderer: &Renderer, width: u32, height: u32) -> Result<Self, Error> {
        let format = renderer.config.blending.map_or(TextureFormat::Rgba8Unorm, |b| b.format);
        Self::with_format(renderer, width, height, format as u32)
    }
    /// `format`: a `CRH_FORMAT_*` value (`TextureFormat as u32`, `TextureFormat::attachment`, ...)
    pub fn with_format(renderer: &Renderer, width: u32, height: u32, format: u32) -> Result<Self, Error> {
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_frame_create_format(renderer.raw, width, height, format, &mut raw) })?;
        Ok(Self { raw, width, height })
    }
    /// `LoadOp::Clear` of colour, depth (1.0) and stencil (examples/showcase/main.rs:217-230)
    pub fn clear(&mut self) {
        status(unsafe { ffi::crh_frame_clear(self.raw) }).unwrap()
    }
    /// The reference's stencil attachment and alpha layers are caller-owned and outlive a `Shape::render` call (renderer.rs:148-158, 892-985): from this
    /// call until `clear` the frame keeps clip / winding counters, saved alphas and the colour of every sample between passes. (It also starts by itself at
    /// the first pass that ends with state left over; `RenderPass::submit` calls this when its draws span several objects.)
    pub fn keep_pass_state(&mut self) {
        status(unsafe { ffi::crh_frame_keep_pass_state(self.raw) }).unwrap()
    }
    /// The depth of the 3-D scene the Shapes are decals in: `[height][width]`
    pub fn upload_depth(&mut self, depth: &[f32]) {
        assert_eq!(depth.len(), (self.width * self.height) as usize);
        status(unsafe { ffi::crh_frame_upload_depth(self.raw, depth.as_ptr()) }).unwrap()
    }
    /// `LoadOp::Load` of caller content: premultiplied 8-bit pixels in the frame's storage order (B G R A for a BGRA format), row 0 = top. Stencil, alpha layers and pass state are reset as by `clear`, depth is kept.
    pub fn upload(&mut self, rgba8: &[u8]) {
        assert_eq!(rgba8.len(), (self.width * self.height * 4) as usize);
        status(unsafe { ffi::crh_frame_upload(self.raw, rgba8.as_ptr() as *const _) }).unwrap()
    }
    /// `crh_frame_load_image`: `upload` with the bytes taken from level 0 of an `Image` on the device (the same size, the same renderer);
    /// complete on return, so the image may be dropped afterwards.
    pub fn load_image(&mut self, image: &Image) -> Result<(), Error> {
        status(unsafe { ffi::crh_frame_load_image(self.raw, image.raw) })
    }
    /// Premultiplied 8-bit pixels in the frame's storage order, row 0 = top
    pub fn download(&mut self) -> Vec<u8> {
        let mut pixels = vec![0u8; (self.width * self.height * 4) as usize];
        status(unsafe { ffi::crh_frame_download(self.raw, pixels.as_mut_ptr() as *mut _) }).unwrap();
        pixels
    }
    /// Waits for the last pass into this frame only
    pub fn synchronize(&self) {
        status(unsafe { ffi::crh_frame_synchronize(self.raw) }).unwrap()
    }
    /// The tile split of the multi-GPU path: passes into this frame draw the pixel rows `rows` only (whole 16-pixel tile rows)
    pub fn set_tile_rows(&self, rows: std::ops::Range<u32>) {
        status(unsafe { ffi::crh_frame_set_tile_rows(self.raw, rows.start, rows.end) }).unwrap()
    }
}
impl Drop for Frame {
    fn drop(&mut self) {
        unsafe { ffi::crh_frame_destroy(self.raw) }
    }
}

/// renderer.rs:163-171 — a set of Paths which is always rendered together
pub struct Shape {
    raw: *mut ffi::crh_scene,
    dynamic_stroke_options_count: usize,
}
impl Shape {
    /// renderer.rs:177-183. `existing_shape` is consumed like the reference's `Option<(Shape, &wgpu::Queue)>`: its device allocations
    /// are reused when large enough (renderer.rs:216-221).
    pub fn from_paths(renderer: &Renderer, dynamic_stroke_options: &[DynamicStrokeOptions], paths: &[Path], existing_shape: Option<Shape>) -> Result<Self, Error> {
        let mut batch = PathBatch::new();
        batch.push_shape(dynamic_stroke_options, paths);
        let view = batch.view();
        // `existing_shape` is moved in (renderer.rs:182): from here on the library owns its handle
        let existing = match existing_shape {
            Some(shape) => {
                let raw = shape.raw;
                std::mem::forget(shape);
                raw
            }
            None => ptr::null_mut(),
        };
        let mut raw = ptr::null_mut();
        match status(unsafe { ffi::crh_shape_from_paths(renderer.raw, &view, existing, &mut raw) }) {
            Ok(()) => Ok(Self { raw, dynamic_stroke_options_count: dynamic_stroke_options.len() }),
            Err(error) => {
                // like the reference, an Err drops the Shape that was moved in: `raw` is it once the upload took it over, `existing` before
                let victim = if raw.is_null() { existing } else { raw };
                if !victim.is_null() {
                    unsafe { ffi::crh_scene_destroy(victim) }
                }
                Err(error)
            }
        }
    }
    /// renderer.rs:267-273 — records one draw into the pass; the instances are indices into the pass' instance data
    pub fn render(&self, _renderer: &Renderer, render_pass: &mut RenderPass, instance_indices: Range<u32>, render_operation: RenderOperation) {
        for instance in instance_indices {
            render_pass.draws.push((self.raw, ffi::crh_draw { shape: 0, instance, op: render_operation as u32, clip_depth: render_pass.clip_depth, alpha_layer: render_pass.alpha_layer }));
        }
    }
    /// renderer.rs:360-376
    pub fn set_dynamic_stroke_options(&self, dynamic_stroke_options_group_index: usize, dynamic_stroke_options_group: &DynamicStrokeOptions) -> Result<(), Error> {
        if dynamic_stroke_options_group_index >= self.dynamic_stroke_options_count {
            return Err(Error::DynamicStrokeOptionsIndexOutOfBounds);
        }
        let options = convert_dynamic(dynamic_stroke_options_group);
        status(unsafe { ffi::crh_scene_set_dynamic_stroke_options(self.raw, 0, dynamic_stroke_options_group_index as u32, &options) })
    }
    /// Parity tap: the byte image `renderer.rs:198-209` uploads, with its cumulative END offsets
    pub fn buffers(&self) -> ([u64; 8], [u64; 3], Vec<u8>, Vec<u8>) {
        let (mut vertex_offsets, mut index_offsets) = ([0u64; 8], [0u64; 3]);
        status(unsafe { ffi::crh_scene_shape_layout(self.raw, 0, vertex_offsets.as_mut_ptr(), index_offsets.as_mut_ptr()) }).unwrap();
        let (mut vertices, mut indices) = (vec![0u8; vertex_offsets[7] as usize], vec![0u8; index_offsets[2] as usize]);
        status(unsafe { ffi::crh_scene_shape_download(self.raw, 0, vertices.as_mut_ptr() as *mut _, indices.as_mut_ptr() as *mut _) }).unwrap();
        (vertex_offsets, index_offsets, vertices, indices)
    }
}
impl Drop for Shape {
    fn drop(&mut self) {
        unsafe { ffi::crh_scene_destroy(self.raw) }
    }
}

/// Many Shapes built together: one launch tessellates all of them (the reference's one-call-per-Shape loop, renderer.rs:187, is
/// launch-latency bound on a GPU). No counterpart upstream; `Shape` is the `n == 1` case.
pub struct Scene {
    raw: *mut ffi::crh_scene,
    shape_count: usize,
}
impl Scene {
    pub fn new(renderer: &Renderer, batch: &PathBatch) -> Result<Self, Error> {
        let view = batch.view();
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_scene_upload(renderer.raw, &view, ptr::null_mut(), &mut raw) })?;
        let scene = Self { raw, shape_count: batch.shape_count() };
        scene.tessellate()?;
        status(unsafe { ffi::crh_scene_status(scene.raw) })?;
        Ok(scene)
    }
    /// The arithmetic of `from_paths` for every Shape, asynchronously on the renderer's tessellation stream
    pub fn tessellate(&self) -> Result<(), Error> {
        status(unsafe { ffi::crh_scene_tessellate(self.raw) })
    }
    /// Stencil + Color of every Shape in index order, instance i = Shape i (the loop of examples/showcase/main.rs:236-250)
    pub fn render(&self, frame: &mut Frame, transforms: &[[f32; 16]], colors: &[[f32; 4]]) -> Result<(), Error> {
        assert!(transforms.len() == self.shape_count && colors.len() == self.shape_count);
        status(unsafe { ffi::crh_scene_render(self.raw, frame.raw, transforms.as_ptr() as *const f32, colors.as_ptr() as *const f32) })
    }
    /// A recorded pass over the Shapes of this Scene: `draws[i]` = (index of the Shape, index into `transforms` / `colors`, operation, clip
    /// depth and alpha layer in effect) — what a sequence of `Shape::render` calls between `Renderer::set_clip_depth` /
    /// `save_alpha_context` calls records in the reference (renderer.rs:267-355, :932-985). Clip nesting and alpha contexts may span Shapes
    /// here: one call is one pass.
    pub fn render_draws(&self, frame: &mut Frame, transforms: &[[f32; 16]], colors: &[[f32; 4]], draws: &[(u32, u32, RenderOperation, u32, u32)]) -> Result<(), Error> {
        assert!(transforms.len() == colors.len());
        let raw_draws: Vec<ffi::crh_draw> = draws
            .iter()
            .map(|&(shape, instance, op, clip_depth, alpha_layer)| {
                assert!((shape as usize) < self.shape_count && (instance as usize) < transforms.len());
                ffi::crh_draw { shape, instance, op: op as u32, clip_depth, alpha_layer }
            })
            .collect();
        status(unsafe {
            ffi::crh_scene_render_draws(self.raw, frame.raw, transforms.as_ptr() as *const f32, colors.as_ptr() as *const f32, transforms.len() as u32, raw_draws.as_ptr(), raw_draws.len() as u32)
        })
    }
}
/// What a gradient does outside [0, 1] (`crh_spread`)
#[derive(Clone, Copy, PartialEq, Debug)]
pub enum Spread {
    Pad = 0,
    Repeat = 1,
    Reflect = 2,
}
/// A linear, radial or conic gradient in the Shape's path coordinates: the source of a Color cover in place of the instance's one colour
/// (include/contrast_hip.h, `crh_scene_set_paints`, states the model). Stops are (offset, straight RGBA), at most 8.
#[derive(Clone, Copy)]
pub struct Paint(pub ffi::crh_paint);
impl Paint {
    fn with(kind: u32, spread: Spread, p0: [f32; 2], p1: [f32; 2], stops: &[(f32, [f32; 4])]) -> Self {
        assert!(!stops.is_empty() && stops.len() <= 8);
        let mut table = [ffi::crh_gradient_stop { offset: 0.0, color: [0.0; 4] }; 8];
        for (slot, &(offset, color)) in table.iter_mut().zip(stops) {
            *slot = ffi::crh_gradient_stop { offset, color };
        }
        Paint(ffi::crh_paint { kind, spread: spread as u32, p0, p1, n_stops: stops.len() as u32, stops: table })
    }
    /// t = 0 at `p0`, t = 1 at `p1`
    pub fn linear(p0: [f32; 2], p1: [f32; 2], stops: &[(f32, [f32; 4])], spread: Spread) -> Self {
        Self::with(1, spread, p0, p1, stops)
    }
    /// t = distance from `center` / `radius`
    pub fn radial(center: [f32; 2], radius: f32, stops: &[(f32, [f32; 4])], spread: Spread) -> Self {
        Self::with(2, spread, center, [radius, 0.0], stops)
    }
    /// t = 0 on the ray from `center` at the angle `start`, t = 1 at `end`: radians, from +x towards +y, 0 < |end - start| <= 2 pi;
    /// `end < start` reads the stops clockwise
    pub fn conic(center: [f32; 2], start: f32, end: f32, stops: &[(f32, [f32; 4])], spread: Spread) -> Self {
        Self::with(ffi::CRH_PAINT_CONIC, spread, center, [start, end], stops)
    }
    /// Host only: what `Scene::set_paints` would refuse
    pub fn validate(&self) -> Result<(), Error> {
        status(unsafe { ffi::crh_paint_validate(&self.0) })
    }
}
impl Scene {
    /// `instance_paint[i]` = the index into `paints` of instance i's paint, or -1 for its solid colour. Stays with the Scene until the next
    /// call; no paints clears it.
    pub fn set_paints(&self, paints: &[Paint], instance_paint: &[i32]) -> Result<(), Error> {
        let table: Vec<ffi::crh_paint> = paints.iter().map(|p| p.0).collect();
        status(unsafe { ffi::crh_scene_set_paints(self.raw, table.as_ptr(), table.len() as u32, instance_paint.as_ptr(), instance_paint.len() as u32) })
    }
}
/// How an image paint reads between texel centres (`CRH_FILTER_*`)
#[derive(Clone, Copy, PartialEq, Debug)]
pub enum Filter {
    Nearest = 0,
    Linear = 1,
    /// `CRH_FILTER_NEAREST | CRH_FILTER_MIPMAP`: the nearest texel of two levels, blended by the level of detail
    NearestMipmap = 0x100,
    /// `CRH_FILTER_LINEAR | CRH_FILTER_MIPMAP`: trilinear
    LinearMipmap = 0x101,
}
/// What `Image::blur` reads outside the image (`crh_blur_edge`)
#[derive(Clone, Copy, PartialEq, Debug)]
pub enum BlurEdge {
    /// (0, 0, 0, 0); the result grows by the radius on every side
    Transparent = 0,
    Pad = 1,
    Repeat = 2,
    Reflect = 3,
}
/// `crh_blur_taps` (host only) -> the integer taps q[0 ..= radius] of one axis of `Image::blur`, radius = ceil(3 sigma) = len() - 1; they sum
/// to exactly 65536 over the 2 radius + 1 positions (include/contrast_hip.h, `crh_image_blur`, states the rule).
pub fn blur_taps(sigma: f32) -> Result<Vec<u32>, Error> {
    let mut radius = 0u32;
    status(unsafe { ffi::crh_blur_taps(sigma, ptr::null_mut(), 0, &mut radius) })?;
    let mut taps = vec![0u32; radius as usize + 1];
    status(unsafe { ffi::crh_blur_taps(sigma, taps.as_mut_ptr(), taps.len() as u32, &mut radius) })?;
    Ok(taps)
}
/// The Porter-Duff operator of `Image::composite` (`crh_composite_op`)
#[derive(Clone, Copy, PartialEq, Debug)]
pub enum CompositeOp {
    Clear = 0,
    Copy = 1,
    Dst = 2,
    SrcOver = 3,
    DstOver = 4,
    SrcIn = 5,
    DstIn = 6,
    SrcOut = 7,
    DstOut = 8,
    SrcAtop = 9,
    DstAtop = 10,
    Xor = 11,
    Plus = 12,
}
/// The blend mode of `Image::composite` (`crh_blend_mode`): the W3C compositing-1 separable modes with a polynomial premultiplied form
#[derive(Clone, Copy, PartialEq, Debug)]
pub enum BlendMode {
    Normal = 0,
    Multiply = 1,
    Screen = 2,
    Overlay = 3,
    Darken = 4,
    Lighten = 5,
    HardLight = 6,
    Difference = 7,
    Exclusion = 8,
}
/// `crh_composite_texels` (host only): the compositing rule on `source.len() / 4` texel pairs of premultiplied RGBA8
/// (include/contrast_hip.h, `crh_image_composite`, states the rule).
pub fn composite_texels(source: &[u8], backdrop: &[u8], op: CompositeOp, mode: BlendMode, opacity: f32) -> Result<Vec<u8>, Error> {
    assert!(source.len() == backdrop.len() && source.len() % 4 == 0);
    let how = ffi::crh_composite { op: op as u32, mode: mode as u32, opacity, x: 0, y: 0 };
    let mut out = vec![0u8; source.len()];
    status(unsafe { ffi::crh_composite_texels(&how, source.as_ptr() as *const _, backdrop.as_ptr() as *const _, (source.len() / 4) as u64, out.as_mut_ptr() as *mut _) })?;
    Ok(out)
}
/// The 4 x 5 matrices of `Image::color_filter`: rows r', g', b', a', columns r, g, b, a, 1 on unpremultiplied colours in [0, 1]. The
/// coefficients are those of SVG filter effects (feColorMatrix), computed in f64 and rounded to f32 once.
pub struct ColorMatrix;
impl ColorMatrix {
    fn rows(m: [f64; 20]) -> [f32; 20] {
        let mut out = [0f32; 20];
        for (o, v) in out.iter_mut().zip(m.iter()) {
            *o = *v as f32;
        }
        out
    }
    pub fn identity() -> [f32; 20] {
        Self::opacity(1.0)
    }
    pub fn saturate(s: f64) -> [f32; 20] {
        Self::rows([
            0.213 + 0.787 * s, 0.715 - 0.715 * s, 0.072 - 0.072 * s, 0.0, 0.0, //
            0.213 - 0.213 * s, 0.715 + 0.285 * s, 0.072 - 0.072 * s, 0.0, 0.0, //
            0.213 - 0.213 * s, 0.715 - 0.715 * s, 0.072 + 0.928 * s, 0.0, 0.0, //
            0.0, 0.0, 0.0, 1.0, 0.0,
        ])
    }
    pub fn hue_rotate(degrees: f64) -> [f32; 20] {
        let (s, c) = degrees.to_radians().sin_cos();
        Self::rows([
            0.213 + c * 0.787 - s * 0.213, 0.715 - c * 0.715 - s * 0.715, 0.072 - c * 0.072 + s * 0.928, 0.0, 0.0, //
            0.213 - c * 0.213 + s * 0.143, 0.715 + c * 0.285 + s * 0.140, 0.072 - c * 0.072 - s * 0.283, 0.0, 0.0, //
            0.213 - c * 0.213 - s * 0.787, 0.715 - c * 0.715 + s * 0.715, 0.072 + c * 0.928 + s * 0.072, 0.0, 0.0, //
            0.0, 0.0, 0.0, 1.0, 0.0,
        ])
    }
    pub fn luminance_to_alpha() -> [f32; 20] {
        Self::rows([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.2125, 0.7154, 0.0721, 0.0, 0.0])
    }
    /// Every texel takes the straight colour (r, g, b) and a times its alpha: the colour of a drop shadow
    pub fn flood(r: f64, g: f64, b: f64, a: f64) -> [f32; 20] {
        Self::rows([0.0, 0.0, 0.0, 0.0, r, 0.0, 0.0, 0.0, 0.0, g, 0.0, 0.0, 0.0, 0.0, b, 0.0, 0.0, 0.0, a, 0.0])
    }
    pub fn opacity(a: f64) -> [f32; 20] {
        Self::rows([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, a, 0.0])
    }
}
/// `crh_color_filter_texels` (host only): the colour-filter rule on `texels.len() / 4` texels of premultiplied RGBA8; `None` is the identity
/// (include/contrast_hip.h, `crh_image_color_filter`, states the rule).
pub fn color_filter_texels(texels: &[u8], matrix: Option<&[f32; 20]>, tables: Option<&[u8; 1024]>) -> Result<Vec<u8>, Error> {
    assert!(texels.len() % 4 == 0);
    let mut out = vec![0u8; texels.len()];
    let (m, t) = (matrix.map_or(ptr::null(), |m| m.as_ptr()), tables.map_or(ptr::null(), |t| t.as_ptr()));
    status(unsafe { ffi::crh_color_filter_texels(m, t, texels.as_ptr() as *const _, (texels.len() / 4) as u64, out.as_mut_ptr() as *mut _) })?;
    Ok(out)
}
/// The operator of `Image::morphology` (`crh_morphology_op`): per channel the min or the max over the window
#[derive(Clone, Copy, PartialEq, Debug)]
pub enum MorphologyOp {
    Erode = 0,
    Dilate = 1,
}
/// `crh_morphology_size` (host only) -> (width, height) of the result of `Image::morphology` on a width x height image
pub fn morphology_size(width: u32, height: u32, op: MorphologyOp, radius_x: u32, radius_y: u32, edge: BlurEdge) -> Result<(u32, u32), Error> {
    let (mut w, mut h) = (0u32, 0u32);
    status(unsafe { ffi::crh_morphology_size(width, height, op as u32, radius_x, radius_y, edge as u32, &mut w, &mut h) })?;
    Ok((w, h))
}
/// `crh_morphology_texels` (host only): the rule on a width x height image of RGBA8 in host memory -> (width, height, texels) of the result
/// (include/contrast_hip.h, `crh_image_morphology`, states the rule).
pub fn morphology_texels(width: u32, height: u32, texels: &[u8], op: MorphologyOp, radius_x: u32, radius_y: u32, edge: BlurEdge) -> Result<(u32, u32, Vec<u8>), Error> {
    assert_eq!(texels.len(), width as usize * height as usize * 4);
    let (w, h) = morphology_size(width, height, op, radius_x, radius_y, edge)?;
    let mut out = vec![0u8; w as usize * h as usize * 4];
    status(unsafe { ffi::crh_morphology_texels(width, height, texels.as_ptr() as *const _, op as u32, radius_x, radius_y, edge as u32, out.as_mut_ptr() as *mut _) })?;
    Ok((w, h, out))
}
/// A kernel matrix of `Image::convolve` (`crh_convolve`): `order_x` columns and `order_y` rows, row-major, in SVG's orientation
/// (feConvolveMatrix's kernelMatrix carries over unchanged); `target` = the kernel cell on the output texel.
#[derive(Clone, PartialEq, Debug)]
pub struct ConvolveKernel {
    pub order_x: u32,
    pub order_y: u32,
    pub values: Vec<f32>,
    pub divisor: f32,
    pub bias: f32,
    pub target: (u32, u32),
}
impl ConvolveKernel {
    /// The target is the centre, the bias 0
    pub fn new(order_x: u32, order_y: u32, values: Vec<f32>, divisor: f32) -> ConvolveKernel {
        assert_eq!(values.len(), order_x as usize * order_y as usize);
        ConvolveKernel { order_x, order_y, values, divisor, bias: 0.0, target: (order_x / 2, order_y / 2) }
    }
    pub fn identity() -> ConvolveKernel {
        ConvolveKernel::new(1, 1, vec![1.0], 1.0)
    }
    pub fn sharpen(amount: f32) -> ConvolveKernel {
        ConvolveKernel::new(3, 3, vec![0.0, -amount, 0.0, -amount, 1.0 + 4.0 * amount, -amount, 0.0, -amount, 0.0], 1.0)
    }
    /// The mean of n x n texels
    pub fn box_filter(n: u32) -> ConvolveKernel {
        ConvolveKernel::new(n, n, vec![1.0; (n * n) as usize], (n * n) as f32)
    }
    pub fn emboss() -> ConvolveKernel {
        ConvolveKernel::new(3, 3, vec![-2.0, -1.0, 0.0, -1.0, 1.0, 1.0, 0.0, 1.0, 2.0], 1.0)
    }
    pub fn laplacian() -> ConvolveKernel {
        ConvolveKernel::new(3, 3, vec![0.0, 1.0, 0.0, 1.0, -4.0, 1.0, 0.0, 1.0, 0.0], 1.0)
    }
    pub fn sobel_x() -> ConvolveKernel {
        ConvolveKernel::new(3, 3, vec![-1.0, 0.0, 1.0, -2.0, 0.0, 2.0, -1.0, 0.0, 1.0], 1.0)
    }
    pub fn sobel_y() -> ConvolveKernel {
        ConvolveKernel::new(3, 3, vec![-1.0, -2.0, -1.0, 0.0, 0.0, 0.0, 1.0, 2.0, 1.0], 1.0)
    }
    /// The C struct; it points into `values`, so it is used no longer than `self` lives
    fn to_c(&self, edge: BlurEdge, preserve_alpha: bool) -> ffi::crh_convolve {
        assert_eq!(self.values.len(), self.order_x as usize * self.order_y as usize);
        ffi::crh_convolve { order_x: self.order_x, order_y: self.order_y, target_x: self.target.0, target_y: self.target.1, kernel: self.values.as_ptr(), divisor: self.divisor, bias: self.bias,
                            edge: edge as u32, preserve_alpha: preserve_alpha as u32 }
    }
}
/// `crh_convolve_validate` (host only): what `Image::convolve` would refuse
pub fn convolve_validate(kernel: &ConvolveKernel, edge: BlurEdge, preserve_alpha: bool) -> Result<(), Error> {
    let how = kernel.to_c(edge, preserve_alpha);
    status(unsafe { ffi::crh_convolve_validate(&how) })
}
/// `crh_convolve_coefficients` (host only) -> (k, bias_k): the quantised kernel, order_x * order_y entries row-major
pub fn convolve_coefficients(kernel: &ConvolveKernel) -> Result<(Vec<i32>, i32), Error> {
    let how = kernel.to_c(BlurEdge::Pad, false);
    let mut k = vec![0i32; kernel.values.len()];
    let mut bias_k = 0i32;
    status(unsafe { ffi::crh_convolve_coefficients(&how, k.as_mut_ptr(), k.len() as u32, &mut bias_k) })?;
    Ok((k, bias_k))
}
/// `crh_convolve_texels` (host only): the rule on a width x height image of RGBA8 in host memory -> the texels of the result, of the same size
/// (include/contrast_hip.h, `crh_image_convolve`, states the rule).
pub fn convolve_texels(width: u32, height: u32, texels: &[u8], kernel: &ConvolveKernel, edge: BlurEdge, preserve_alpha: bool) -> Result<Vec<u8>, Error> {
    assert_eq!(texels.len(), width as usize * height as usize * 4);
    let how = kernel.to_c(edge, preserve_alpha);
    let mut out = vec![0u8; texels.len()];
    status(unsafe { ffi::crh_convolve_texels(width, height, texels.as_ptr() as *const _, &how, out.as_mut_ptr() as *mut _) })?;
    Ok(out)
}
/// `crh_lighting_op`
#[derive(Clone, Copy, PartialEq, Debug)]
pub enum LightingOp {
    Diffuse = 0,
    Specular = 1,
}
/// The light of `Image::lighting` (`crh_light_kind` and its fields): coordinates in the image's texel space, x right, y down, z towards the
/// viewer; angles in degrees (a `cone_angle` of 0 = no cone).
#[derive(Clone, Copy, PartialEq, Debug)]
pub enum Light {
    Distant { azimuth: f32, elevation: f32 },
    Point { position: [f32; 3] },
    Spot { position: [f32; 3], points_at: [f32; 3], exponent: f32, cone_angle: f32 },
}
/// What is lit and how: the fields of `crh_lighting` that do not describe the light
#[derive(Clone, Copy, PartialEq, Debug)]
pub struct Lighting {
    pub op: LightingOp,
    pub surface_scale: f32,
    pub constant: f32,
    pub specular_exponent: f32,
    pub color: [f32; 3],
    pub edge: BlurEdge,
}
impl Default for Lighting {
    fn default() -> Lighting {
        Lighting { op: LightingOp::Diffuse, surface_scale: 1.0, constant: 1.0, specular_exponent: 1.0, color: [1.0; 3], edge: BlurEdge::Pad }
    }
}
impl Lighting {
    /// The C struct; the fields the light does not use stay 0
    fn to_c(&self, light: &Light) -> ffi::crh_lighting {
        let mut how = ffi::crh_lighting { op: self.op as u32, light: 0, edge: self.edge as u32, surface_scale: self.surface_scale, constant: self.constant,
                                          specular_exponent: self.specular_exponent, color: self.color, azimuth: 0.0, elevation: 0.0, position: [0.0; 3], points_at: [0.0; 3],
                                          spot_exponent: 0.0, cone_angle: 0.0 };
        match *light {
            Light::Distant { azimuth, elevation } => {
                how.light = ffi::CRH_LIGHT_DISTANT;
                how.azimuth = azimuth;
                how.elevation = elevation;
            }
            Light::Point { position } => {
                how.light = ffi::CRH_LIGHT_POINT;
                how.position = position;
            }
            Light::Spot { position, points_at, exponent, cone_angle } => {
                how.light = ffi::CRH_LIGHT_SPOT;
                how.position = position;
                how.points_at = points_at;
                how.spot_exponent = exponent;
                how.cone_angle = cone_angle;
            }
        }
        how
    }
}
/// `crh_lighting_validate` (host only): what `Image::lighting` would refuse
pub fn lighting_validate(light: &Light, lighting: &Lighting) -> Result<(), Error> {
    let how = lighting.to_c(light);
    status(unsafe { ffi::crh_lighting_validate(&how) })
}
/// `crh_lighting_texels` (host only): the rule on a width x height image of RGBA8 in host memory -> the texels of the result, of the same size
/// (include/contrast_hip.h, `crh_image_lighting`, states the rule).
pub fn lighting_texels(width: u32, height: u32, texels: &[u8], light: &Light, lighting: &Lighting) -> Result<Vec<u8>, Error> {
    assert_eq!(texels.len(), width as usize * height as usize * 4);
    let how = lighting.to_c(light);
    let mut out = vec![0u8; texels.len()];
    status(unsafe { ffi::crh_lighting_texels(width, height, texels.as_ptr() as *const _, &how, out.as_mut_ptr() as *mut _) })?;
    Ok(out)
}
/// `crh_turbulence_kind`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum TurbulenceKind {
    FractalNoise = 0,
    Turbulence = 1,
}
/// The fields of `crh_turbulence` (include/contrast_hip.h, `crh_image_turbulence`, states the rule): lattice cells per texel on each axis,
/// octaves of twice the frequency and half the weight each, the seed of the tables, whether the image tiles with itself, whether alpha is
/// 255 instead of a fourth channel of noise, and the noise-space position of texel (0, 0).
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct Turbulence {
    pub base_frequency: [f32; 2],
    pub octaves: u32,
    pub seed: i32,
    pub kind: TurbulenceKind,
    pub stitch: bool,
    pub opaque: bool,
    pub offset: [f32; 2],
}
impl Default for Turbulence {
    fn default() -> Turbulence {
        Turbulence { base_frequency: [0.0; 2], octaves: 1, seed: 0, kind: TurbulenceKind::Turbulence, stitch: false, opaque: false, offset: [0.0; 2] }
    }
}
impl Turbulence {
    fn to_c(&self) -> ffi::crh_turbulence {
        ffi::crh_turbulence { kind: self.kind as u32, octaves: self.octaves, seed: self.seed, stitch: self.stitch as u32, opaque: self.opaque as u32,
                              base_frequency: self.base_frequency, offset: self.offset }
    }
}
/// `crh_turbulence_validate` (host only): what `Image::turbulence` would refuse of the fields
pub fn turbulence_validate(turbulence: &Turbulence) -> Result<(), Error> {
    let how = turbulence.to_c();
    status(unsafe { ffi::crh_turbulence_validate(&how) })
}
/// `crh_turbulence_tables` (host only) -> (the permutation of 0..255, the unit gradients as gradient[(k * 256 + i) * 2 + c]) that `seed` gives
pub fn turbulence_tables(seed: i32) -> Result<(Vec<u8>, Vec<f64>), Error> {
    let (mut lattice, mut gradient) = (vec![0u8; 256], vec![0f64; 4 * 256 * 2]);
    status(unsafe { ffi::crh_turbulence_tables(seed, lattice.as_mut_ptr(), gradient.as_mut_ptr()) })?;
    Ok((lattice, gradient))
}
/// `crh_turbulence_texels` (host only): the rule -> the width * height * 4 bytes of the image
pub fn turbulence_texels(width: u32, height: u32, turbulence: &Turbulence) -> Result<Vec<u8>, Error> {
    let how = turbulence.to_c();
    status(unsafe { ffi::crh_turbulence_validate(&how) })?;
    assert!(width >= 1 && height >= 1 && width <= 16384 && height <= 16384);
    let mut out = vec![0u8; width as usize * height as usize * 4];
    status(unsafe { ffi::crh_turbulence_texels(width, height, &how, out.as_mut_ptr() as *mut _) })?;
    Ok(out)
}
/// `crh_channel`: the channel of a displacement map that moves an axis
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Channel {
    R = 0,
    G = 1,
    B = 2,
    A = 3,
}
/// The fields of `crh_displace` (include/contrast_hip.h, `crh_image_displace`, states the rule): the scale of each axis in texels (SVG has
/// one: give it twice), the map's channels that move x and y, the filter (`Nearest` or `Linear`) and what the SOURCE is outside itself.
/// The defaults are SVG's.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct Displace {
    pub scale: [f32; 2],
    pub x_channel: Channel,
    pub y_channel: Channel,
    pub filter: Filter,
    pub edge: BlurEdge,
}
impl Default for Displace {
    fn default() -> Displace {
        Displace { scale: [0.0; 2], x_channel: Channel::A, y_channel: Channel::A, filter: Filter::Linear, edge: BlurEdge::Transparent }
    }
}
impl Displace {
    fn to_c(&self) -> ffi::crh_displace {
        ffi::crh_displace { scale: self.scale, x_channel: self.x_channel as u32, y_channel: self.y_channel as u32, filter: self.filter as u32, edge: self.edge as u32 }
    }
}
/// `crh_displace_validate` (host only): what `Image::displace` would refuse of the fields
pub fn displace_validate(displace: &Displace) -> Result<(), Error> {
    let how = displace.to_c();
    status(unsafe { ffi::crh_displace_validate(&how) })
}
/// `crh_displace_offset` (host only) -> the offsets (qx, qy), in 1/256 texel, of two straight map codes <= 255
pub fn displace_offset(displace: &Displace, code_x: u32, code_y: u32) -> Result<[i32; 2], Error> {
    let how = displace.to_c();
    let mut q = [0i32; 2];
    status(unsafe { ffi::crh_displace_offset(&how, code_x, code_y, q.as_mut_ptr()) })?;
    Ok(q)
}
/// `crh_displace_texels` (host only): the rule on two width * height * 4 byte slices, the source and the map -> the bytes of the result
pub fn displace_texels(width: u32, height: u32, texels: &[u8], map: &[u8], displace: &Displace) -> Result<Vec<u8>, Error> {
    assert_eq!(texels.len(), width as usize * height as usize * 4);
    assert_eq!(map.len(), texels.len());
    let how = displace.to_c();
    let mut out = vec![0u8; texels.len()];
    status(unsafe { ffi::crh_displace_texels(width, height, texels.as_ptr() as *const _, map.as_ptr() as *const _, &how, out.as_mut_ptr() as *mut _) })?;
    Ok(out)
}
/// The fields of `crh_variable_blur` (include/contrast_hip.h, `crh_image_variable_blur`, states the rule): per axis the sigma at mask code 0
/// and at code 255 (linear in the code between; either may be the larger), the mask's channel whose STORED code is the level, and what
/// the SOURCE is outside itself. The edge's default is `Pad` because the call keeps the size and a backdrop should not darken at its rim.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct VariableBlur {
    pub sigma_x: [f32; 2],
    pub sigma_y: [f32; 2],
    pub channel: Channel,
    pub edge: BlurEdge,
}
impl Default for VariableBlur {
    fn default() -> VariableBlur {
        VariableBlur { sigma_x: [0.0; 2], sigma_y: [0.0; 2], channel: Channel::A, edge: BlurEdge::Pad }
    }
}
impl VariableBlur {
    fn to_c(&self) -> ffi::crh_variable_blur {
        ffi::crh_variable_blur { sigma_x: self.sigma_x, sigma_y: self.sigma_y, channel: self.channel as u32, edge: self.edge as u32 }
    }
}
/// `crh_variable_blur_validate` (host only): what `Image::variable_blur` would refuse of the fields
pub fn variable_blur_validate(blur: &VariableBlur) -> Result<(), Error> {
    let how = blur.to_c();
    status(unsafe { ffi::crh_variable_blur_validate(&how) })
}
/// `crh_variable_blur_sigma` (host only) -> the sigmas (x, y) of one mask code <= 255
pub fn variable_blur_sigma(blur: &VariableBlur, code: u32) -> Result<[f32; 2], Error> {
    let how = blur.to_c();
    let (mut sigma_x, mut sigma_y) = (0f32, 0f32);
    status(unsafe { ffi::crh_variable_blur_sigma(&how, code, &mut sigma_x, &mut sigma_y) })?;
    Ok([sigma_x, sigma_y])
}
/// `crh_variable_blur_texels` (host only): the rule on two width * height * 4 byte slices, the source and the mask -> the bytes of the result
pub fn variable_blur_texels(width: u32, height: u32, texels: &[u8], mask: &[u8], blur: &VariableBlur) -> Result<Vec<u8>, Error> {
    assert_eq!(texels.len(), width as usize * height as usize * 4);
    assert_eq!(mask.len(), texels.len());
    let how = blur.to_c();
    let mut out = vec![0u8; texels.len()];
    status(unsafe { ffi::crh_variable_blur_texels(width, height, texels.as_ptr() as *const _, mask.as_ptr() as *const _, &how, out.as_mut_ptr() as *mut _) })?;
    Ok(out)
}
/// `crh_transform_filter`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum TransformFilter {
    Nearest = 0,
    Linear = 1,
    /// Catmull-Rom over 4 x 4 texels
    Cubic = 2,
}
/// The fields of `crh_transform` (include/contrast_hip.h, `crh_image_transform`, states the rule): the matrix that maps RESULT coordinates
/// (x, y, 1) to SOURCE coordinates, row-major, the result's size, the filter and what the SOURCE is outside itself.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct Transform {
    pub matrix: [f64; 9],
    pub width: u32,
    pub height: u32,
    pub filter: TransformFilter,
    pub edge: BlurEdge,
}
impl Default for Transform {
    fn default() -> Transform {
        Transform { matrix: [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], width: 1, height: 1, filter: TransformFilter::Linear, edge: BlurEdge::Transparent }
    }
}
impl Transform {
    fn to_c(&self) -> ffi::crh_transform {
        ffi::crh_transform { matrix: self.matrix, width: self.width, height: self.height, filter: self.filter as u32, edge: self.edge as u32 }
    }
}
/// `crh_transform_validate` (host only): what `Image::resample` would refuse of the fields
pub fn transform_validate(transform: &Transform) -> Result<(), Error> {
    let how = transform.to_c();
    status(unsafe { ffi::crh_transform_validate(&how) })
}
/// `crh_transform_fit` (host only): for a width x height source and `forward`, which maps SOURCE coordinates to the caller's target space,
/// the call whose result holds the whole source, and where the target space's (0, 0) lies in that result
pub fn transform_fit(width: u32, height: u32, forward: &[f64; 9], filter: TransformFilter, edge: BlurEdge) -> Result<(Transform, [i32; 2]), Error> {
    let mut how = Transform::default().to_c();
    let mut origin = [0i32; 2];
    status(unsafe { ffi::crh_transform_fit(width, height, forward.as_ptr(), filter as u32, edge as u32, &mut how, origin.as_mut_ptr()) })?;
    Ok((Transform { matrix: how.matrix, width: how.width, height: how.height, filter, edge }, origin))
}
/// `crh_transform_position` (host only) -> where result texel (i, j) reads the source, in 1/256 texel, and whether the texel is visible
pub fn transform_position(transform: &Transform, i: u32, j: u32) -> Result<([i32; 2], bool), Error> {
    let how = transform.to_c();
    let mut position = [0i32; 2];
    let mut visible = 0u32;
    status(unsafe { ffi::crh_transform_position(&how, i, j, position.as_mut_ptr(), &mut visible) })?;
    Ok((position, visible != 0))
}
/// `crh_transform_texels` (host only): the rule on the width * height * 4 bytes of a source -> the bytes of the result
pub fn transform_texels(width: u32, height: u32, texels: &[u8], transform: &Transform) -> Result<Vec<u8>, Error> {
    assert_eq!(texels.len(), width as usize * height as usize * 4);
    transform_validate(transform)?;
    let how = transform.to_c();
    let mut out = vec![0u8; transform.width as usize * transform.height as usize * 4];
    status(unsafe { ffi::crh_transform_texels(width, height, texels.as_ptr() as *const _, &how, out.as_mut_ptr() as *mut _) })?;
    Ok(out)
}
/// `crh_distance_mode`: what the distance is measured to
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum DistanceMode {
    /// to the shape: 255 on it, falling to 0 at the spread (glow, outline, spread)
    Outside = 0,
    /// to what is not the shape: 0 off it, rising into it (chisel, inner glow)
    Inside = 1,
}
/// The fields of `crh_distance` (include/contrast_hip.h, `crh_image_distance_field`, states the rule): the mode, the channel whose stored
/// code against the threshold makes the shape, the spread in texels (1..=255) and what the source is outside itself.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Distance {
    pub spread: u32,
    pub mode: DistanceMode,
    pub channel: Channel,
    pub threshold: u32,
    pub edge: BlurEdge,
}
impl Default for Distance {
    fn default() -> Distance {
        Distance { spread: 1, mode: DistanceMode::Outside, channel: Channel::A, threshold: 128, edge: BlurEdge::Transparent }
    }
}
impl Distance {
    fn to_c(&self) -> ffi::crh_distance {
        ffi::crh_distance { mode: self.mode as u32, channel: self.channel as u32, threshold: self.threshold, spread: self.spread, edge: self.edge as u32 }
    }
}
/// `crh_distance_validate` (host only): what `Image::distance_field` would refuse of the fields
pub fn distance_validate(distance: &Distance) -> Result<(), Error> {
    let how = distance.to_c();
    status(unsafe { ffi::crh_distance_validate(&how) })
}
/// `crh_distance_code` (host only) -> the result byte of one squared distance between texel centres
pub fn distance_code(distance: &Distance, squared_distance: u64) -> Result<u32, Error> {
    let how = distance.to_c();
    let mut code = 0u32;
    status(unsafe { ffi::crh_distance_code(&how, squared_distance, &mut code) })?;
    Ok(code)
}
/// `crh_distance_size` (host only) -> (width, height) of the result of `Image::distance_field` on a width x height image
pub fn distance_size(width: u32, height: u32, distance: &Distance) -> Result<(u32, u32), Error> {
    let how = distance.to_c();
    let (mut w, mut h) = (0u32, 0u32);
    status(unsafe { ffi::crh_distance_size(width, height, &how, &mut w, &mut h) })?;
    Ok((w, h))
}
/// `crh_distance_texels` (host only): the rule on a width x height image of RGBA8 in host memory -> (width, height, texels) of the result
pub fn distance_texels(width: u32, height: u32, texels: &[u8], distance: &Distance) -> Result<(u32, u32, Vec<u8>), Error> {
    assert_eq!(texels.len(), width as usize * height as usize * 4);
    let (w, h) = distance_size(width, height, distance)?;
    let how = distance.to_c();
    let mut out = vec![0u8; w as usize * h as usize * 4];
    status(unsafe { ffi::crh_distance_texels(width, height, texels.as_ptr() as *const _, &how, out.as_mut_ptr() as *mut _) })?;
    Ok((w, h, out))
}
/// `crh_resize_filter`: the reconstruction filter of `Image::resize`, widened by the ratio on an axis that shrinks
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ResizeFilter {
    /// support 0.5: nearest when magnifying, the exact area mean at integer ratios
    Box = 0,
    /// support 1: bilinear when magnifying
    Triangle = 1,
    /// support 2: the interpolating cubic (B = 0, C = 1/2)
    CatmullRom = 2,
    /// support 2: Mitchell-Netravali with B = C = 1/3; softer, not interpolating
    Mitchell = 3,
    /// support 3: the sharpest, with ringing at hard edges
    Lanczos3 = 4,
}
/// `crh_resize_taps` (host only) -> (first, count, taps) of one axis of `Image::resize` from n source texels to m: output o reads the source
/// indices first[o] .. first[o] + count[o] - 1 with the signed taps that follow each other in `taps`; an output's taps sum to exactly
/// 16384 (include/contrast_hip.h, `crh_image_resize`, states the rule).
pub fn resize_taps(n: u32, m: u32, filter: ResizeFilter) -> Result<(Vec<i32>, Vec<u16>, Vec<i16>), Error> {
    let mut total = 0u64;
    status(unsafe { ffi::crh_resize_taps(n, m, filter as u32, ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), 0, &mut total) })?;
    let (mut first, mut count, mut taps) = (vec![0i32; m as usize], vec![0u16; m as usize], vec![0i16; total as usize]);
    status(unsafe { ffi::crh_resize_taps(n, m, filter as u32, first.as_mut_ptr(), count.as_mut_ptr(), taps.as_mut_ptr(), total, ptr::null_mut()) })?;
    Ok((first, count, taps))
}
/// `crh_resize_texels` (host only): the rule on a width x height image of RGBA8 in host memory -> the out_width x out_height result's bytes
pub fn resize_texels(width: u32, height: u32, texels: &[u8], out_width: u32, out_height: u32, filter: ResizeFilter) -> Result<Vec<u8>, Error> {
    assert_eq!(texels.len(), width as usize * height as usize * 4);
    let legal = (1..=16384).contains(&out_width) && (1..=16384).contains(&out_height); // (what the library refuses gets a texel's room and the library's status)
    let mut out = vec![0u8; if legal { out_width as usize * out_height as usize * 4 } else { 4 }];
    status(unsafe { ffi::crh_resize_texels(width, height, texels.as_ptr() as *const _, out_width, out_height, filter as u32, out.as_mut_ptr() as *mut _) })?;
    Ok(out)
}
/// `crh_image_stats` as it is: `histogram[256 * c + v]` = how many texels store code v in channel c (r, g, b, a), [x0, x1) x [y0, y1) around
/// the texels inside (all 0 if none is), `count` = their number
pub type ImageStatistics = ffi::crh_image_stats;
/// `crh_crop_texels` (host only): the rule of `Image::crop` on a width x height image of RGBA8 in host memory -> the out_width x out_height result's bytes
pub fn crop_texels(width: u32, height: u32, texels: &[u8], x: i32, y: i32, out_width: u32, out_height: u32) -> Result<Vec<u8>, Error> {
    assert_eq!(texels.len(), width as usize * height as usize * 4);
    let legal = (1..=16384).contains(&out_width) && (1..=16384).contains(&out_height); // (what the library refuses gets a texel's room and the library's status)
    let mut out = vec![0u8; if legal { out_width as usize * out_height as usize * 4 } else { 4 }];
    status(unsafe { ffi::crh_crop_texels(width, height, texels.as_ptr() as *const _, x, y, out_width, out_height, out.as_mut_ptr() as *mut _) })?;
    Ok(out)
}
/// `crh_statistics_texels` (host only): the rule of `Image::statistics` on a width x height image of RGBA8 in host memory
pub fn statistics_texels(width: u32, height: u32, texels: &[u8], channel: Channel, threshold: u32) -> Result<ImageStatistics, Error> {
    assert_eq!(texels.len(), width as usize * height as usize * 4);
    let mut out = ImageStatistics { histogram: [0u32; 1024], x0: 0, y0: 0, x1: 0, y1: 0, count: 0 };
    status(unsafe { ffi::crh_statistics_texels(width, height, texels.as_ptr() as *const _, channel as u32, threshold, &mut out) })?;
    Ok(out)
}
/// `crh_image`: width x height texels of premultiplied RGBA8 on the device, row 0 = top — the bytes `Frame::download` hands out. One level
/// until `generate_mipmaps`. Dropping it while a Scene's paint table names it is legal: the table keeps the pixels and their mipmaps.
pub struct Image {
    raw: *mut ffi::crh_image,
    width: u32,
    height: u32,
    origin: (u32, u32),
}
impl Image {
    /// `rgba8`: width * height * 4 bytes, copied before the call returns
    pub fn new(renderer: &Renderer, width: u32, height: u32, rgba8: &[u8]) -> Result<Image, Error> {
        assert_eq!(rgba8.len(), width as usize * height as usize * 4);
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_create(renderer.raw, width, height, rgba8.as_ptr() as *const _, &mut raw) })?;
        Ok(Image { raw, width, height, origin: (0, 0) })
    }
    /// `crh_image_turbulence` -> a new `Image` of one level, width x height, origin (0, 0): procedural noise made on the device (SVG
    /// feTurbulence); binary64 arithmetic in a fixed order, complete on return (a synchronous call).
    pub fn turbulence(renderer: &Renderer, width: u32, height: u32, turbulence: &Turbulence) -> Result<Image, Error> {
        let how = turbulence.to_c();
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_turbulence(renderer.raw, width, height, &how, &mut raw) })?;
        Ok(Image { raw, width, height, origin: (0, 0) })
    }
    /// A snapshot of what the frame shows (an RGBA8 or RGBA8-attachment frame), copied on the device
    pub fn from_frame(frame: &Frame) -> Result<Image, Error> {
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_create_from_frame(frame.raw, &mut raw) })?;
        let (mut width, mut height) = (0u32, 0u32);
        status(unsafe { ffi::crh_image_size(raw, &mut width, &mut height) })?;
        Ok(Image { raw, width, height, origin: (0, 0) })
    }
    pub fn size(&self) -> (u32, u32) {
        (self.width, self.height)
    }
    /// `crh_image_generate_mipmaps`: the levels below the image, built on the device. A second call changes nothing; a paint table set before
    /// the call keeps drawing the one level.
    pub fn generate_mipmaps(&mut self) -> Result<(), Error> {
        status(unsafe { ffi::crh_image_generate_mipmaps(self.raw) })
    }
    /// 1 until `generate_mipmaps`, then floor(log2(max(width, height))) + 1
    pub fn levels(&self) -> Result<u32, Error> {
        let mut n = 0u32;
        status(unsafe { ffi::crh_image_level_count(self.raw, &mut n) })?;
        Ok(n)
    }
    /// -> (width, height, texels) of level `level` (0 = the image itself)
    pub fn download_level(&self, level: u32) -> Result<(u32, u32, Vec<u8>), Error> {
        let (mut width, mut height) = (0u32, 0u32);
        status(unsafe { ffi::crh_image_download_level(self.raw, level, ptr::null_mut(), &mut width, &mut height) })?;
        let mut out = vec![0u8; width as usize * height as usize * 4];
        status(unsafe { ffi::crh_image_download_level(self.raw, level, out.as_mut_ptr() as *mut _, &mut width, &mut height) })?;
        Ok((width, height, out))
    }
    /// `crh_image_blur` -> a new `Image` of one level: the separable Gaussian of this image's level 0, integer and bit-exact, complete on
    /// return (a synchronous call: one wait per blur). Sigmas in [0, `CRH_MAX_BLUR_SIGMA`]. `BlurEdge::Transparent` grows the result by
    /// ceil(3 sigma) on every side and its `origin()` is (Rx, Ry); the other edges keep the size. This image is not modified.
    pub fn blur(&self, sigma_x: f32, sigma_y: f32, edge: BlurEdge) -> Result<Image, Error> {
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_blur(self.raw, sigma_x, sigma_y, edge as u32, &mut raw) })?;
        let (mut width, mut height) = (0u32, 0u32);
        status(unsafe { ffi::crh_image_size(raw, &mut width, &mut height) })?;
        let origin = if edge == BlurEdge::Transparent { ((width - self.width) / 2, (height - self.height) / 2) } else { (0, 0) };
        Ok(Image { raw, width, height, origin })
    }
    /// The texel of this image over texel (0, 0) of the image it was blurred or dilated from: (0, 0) unless `blur` or `morphology` grew it,
    /// or `crop`, `trim` or `from_frame_region` cut it: a crop at (x, y) moves the origin by (-x, -y), so it can be negative — a signed value
    /// in these 32 bits (`as i32`), as `composite`'s offset rule reads it
    pub fn origin(&self) -> (u32, u32) {
        self.origin
    }
    /// `crh_image_create_from_frame_region`: byte for byte `from_frame(frame)?.crop(x, y, width, height)`, origin (-x, -y), without the
    /// full-size copy; the rectangle may leave the frame (zeros there) and only its own size is limited to 16384.
    pub fn from_frame_region(frame: &Frame, x: i32, y: i32, width: u32, height: u32) -> Result<Image, Error> {
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_create_from_frame_region(frame.raw, x, y, width, height, &mut raw) })?;
        Ok(Image { raw, width, height, origin: ((x as u32).wrapping_neg(), (y as u32).wrapping_neg()) })
    }
    /// `crh_image_crop` -> a new `Image` of one level, width x height (each in [1, 16384]): texel (i, j) is this image's (x + i, y + j), the
    /// bytes as stored, (0, 0, 0, 0) outside this image; complete on return (a synchronous call). x and y are any i32: a rectangle that
    /// misses this image is a transparent canvas, a larger one the transparent backdrop around it. Its origin is this image's minus (x, y).
    pub fn crop(&self, x: i32, y: i32, width: u32, height: u32) -> Result<Image, Error> {
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_crop(self.raw, x, y, width, height, &mut raw) })?;
        Ok(Image { raw, width, height, origin: (self.origin.0.wrapping_sub(x as u32), self.origin.1.wrapping_sub(y as u32)) })
    }
    /// `crh_image_statistics` -> the per-channel histograms of the stored codes over all texels, and the bounds and the number of the texels
    /// inside: stored code of `channel` >= `threshold` (1..=255), `distance_field`'s definition. Reduced on the device (a synchronous call).
    pub fn statistics(&self, channel: Channel, threshold: u32) -> Result<ImageStatistics, Error> {
        let mut out = ImageStatistics { histogram: [0u32; 1024], x0: 0, y0: 0, x1: 0, y1: 0, count: 0 };
        status(unsafe { ffi::crh_image_statistics(self.raw, channel as u32, threshold, &mut out) })?;
        Ok(out)
    }
    /// `statistics(channel, threshold)`'s (x0, y0, x1, y1): half-open, all 0 if no texel is inside
    pub fn bounds(&self, channel: Channel, threshold: u32) -> Result<(u32, u32, u32, u32), Error> {
        let s = self.statistics(channel, threshold)?;
        Ok((s.x0, s.y0, s.x1, s.y1))
    }
    /// `statistics`, then `crop` to the bounds grown by `margin` on every side and clipped to this image; nothing inside: the 1 x 1 crop at (0, 0)
    pub fn trim(&self, channel: Channel, threshold: u32, margin: u32) -> Result<Image, Error> {
        let (x0, y0, x1, y1) = self.bounds(channel, threshold)?;
        if x1 == x0 {
            return self.crop(0, 0, 1, 1);
        }
        let (x0, y0) = (x0.saturating_sub(margin), y0.saturating_sub(margin));
        let (x1, y1) = ((x1 + margin).min(self.width), (y1 + margin).min(self.height));
        self.crop(x0 as i32, y0 as i32, x1 - x0, y1 - y0)
    }
    /// `crh_image_composite`, called on the backdrop -> a new `Image` of one level, of this image's size, origin (0, 0): `source` combined
    /// with this image texel by texel by a Porter-Duff operator, a blend mode and a group opacity in [0, 1]; integer and bit-exact, complete
    /// on return. Source texel (0, 0) lies over this image's texel `offset` (any integers; the source is transparent outside itself). To
    /// place a `BlurEdge::Transparent` result so that the image it was blurred from would lie at (dx, dy): offset = (dx - origin().0,
    /// dy - origin().1) of the source. Neither image is modified; `source` may be this image.
    pub fn composite(&self, source: &Image, op: CompositeOp, mode: BlendMode, opacity: f32, offset: (i32, i32)) -> Result<Image, Error> {
        let how = ffi::crh_composite { op: op as u32, mode: mode as u32, opacity, x: offset.0, y: offset.1 };
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_composite(self.raw, source.raw, &how, &mut raw) })?;
        Ok(Image { raw, width: self.width, height: self.height, origin: (0, 0) })
    }
    /// `crh_image_color_filter` -> a new `Image` of one level, of this image's size and origin: every texel unpremultiplied, through the 4 x 5
    /// matrix, then through the four 256-entry tables, and premultiplied again; integer and bit-exact, complete on return. `None` is the
    /// identity. A blurred snapshot through `ColorMatrix::flood(r, g, b, a)` is a drop shadow in that colour. This image is not modified.
    pub fn color_filter(&self, matrix: Option<&[f32; 20]>, tables: Option<&[u8; 1024]>) -> Result<Image, Error> {
        let mut raw = ptr::null_mut();
        let (m, t) = (matrix.map_or(ptr::null(), |m| m.as_ptr()), tables.map_or(ptr::null(), |t| t.as_ptr()));
        status(unsafe { ffi::crh_image_color_filter(self.raw, m, t, &mut raw) })?;
        Ok(Image { raw, width: self.width, height: self.height, origin: self.origin })
    }
    /// `crh_image_morphology` -> a new `Image` of one level: per channel the min (`Erode`) or max (`Dilate`) of this image's level 0 over the
    /// rectangle |dx| <= radius_x, |dy| <= radius_y; exact, complete on return (a synchronous call). Radii in [0, `CRH_MAX_MORPHOLOGY_RADIUS`].
    /// `Dilate` under `BlurEdge::Transparent` grows the result by the radius on every side and its `origin()` is (radius_x, radius_y), as
    /// `blur` grows; everything else keeps the size and origin (0, 0). This image is not modified.
    pub fn morphology(&self, op: MorphologyOp, radius_x: u32, radius_y: u32, edge: BlurEdge) -> Result<Image, Error> {
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_morphology(self.raw, op as u32, radius_x, radius_y, edge as u32, &mut raw) })?;
        let (mut width, mut height) = (0u32, 0u32);
        status(unsafe { ffi::crh_image_size(raw, &mut width, &mut height) })?;
        let origin = if op == MorphologyOp::Dilate && edge == BlurEdge::Transparent { (radius_x, radius_y) } else { (0, 0) };
        Ok(Image { raw, width, height, origin })
    }
    /// `crh_image_distance_field` -> a new `Image` of one level: per texel the exact Euclidean distance between texel centres to the shape
    /// (or, `Inside`, to what is not the shape), coded over the spread on all four channels; complete on return (a synchronous call).
    /// `Outside` under `BlurEdge::Transparent` grows the result by the spread on every side and its origin is (spread, spread).
    pub fn distance_field(&self, distance: &Distance) -> Result<Image, Error> {
        let how = distance.to_c();
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_distance_field(self.raw, &how, &mut raw) })?;
        let (mut width, mut height) = (0u32, 0u32);
        status(unsafe { ffi::crh_image_size(raw, &mut width, &mut height) })?;
        let origin = if distance.mode == DistanceMode::Outside && distance.edge == BlurEdge::Transparent { (distance.spread, distance.spread) } else { (0, 0) };
        Ok(Image { raw, width, height, origin })
    }
    /// `crh_image_resize` -> a new `Image` of one level, width x height, the whole of this image resampled; complete on return (a
    /// synchronous call); its origin is (0, 0). An axis that shrinks by more than the filter's cap (about 85 under `Lanczos3`) is refused
    /// with `CRH_ERR_UNSUPPORTED`: chain two calls.
    pub fn resize(&self, width: u32, height: u32, filter: ResizeFilter) -> Result<Image, Error> {
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_resize(self.raw, width, height, filter as u32, &mut raw) })?;
        Ok(Image { raw, width, height, origin: (0, 0) })
    }
    pub fn dilate(&self, radius_x: u32, radius_y: u32, edge: BlurEdge) -> Result<Image, Error> {
        self.morphology(MorphologyOp::Dilate, radius_x, radius_y, edge)
    }
    pub fn erode(&self, radius_x: u32, radius_y: u32, edge: BlurEdge) -> Result<Image, Error> {
        self.morphology(MorphologyOp::Erode, radius_x, radius_y, edge)
    }
    /// `crh_image_convolve` -> a new `Image` of one level, of this image's size and origin: this image's level 0 through a kernel matrix of
    /// up to `CRH_MAX_CONVOLVE_ORDER` entries per axis; integer and bit-exact, complete on return (a synchronous call). `preserve_alpha` keeps
    /// every texel's alpha and convolves the unpremultiplied colours. The size is the source's under every edge. This image is not modified.
    pub fn convolve(&self, kernel: &ConvolveKernel, edge: BlurEdge, preserve_alpha: bool) -> Result<Image, Error> {
        let how = kernel.to_c(edge, preserve_alpha);
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_convolve(self.raw, &how, &mut raw) })?;
        Ok(Image { raw, width: self.width, height: self.height, origin: self.origin })
    }
    /// `crh_image_displace` -> a new `Image` of one level, of this image's size, origin (0, 0): this image read through the per-texel
    /// offsets of `map`, an image of the same size and renderer (SVG feDisplacementMap); integer and bit-exact, complete on return (a
    /// synchronous call). Neither image is modified.
    pub fn displace(&self, map: &Image, displace: &Displace) -> Result<Image, Error> {
        let how = displace.to_c();
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_displace(self.raw, map.raw, &how, &mut raw) })?;
        Ok(Image { raw, width: self.width, height: self.height, origin: (0, 0) })
    }
    /// `crh_image_transform`, the raw call -> a new `Image` of one level, `transform.width` x `transform.height`, origin (0, 0): this image
    /// seen through `transform.matrix` (result -> this image); positions in binary64 in a fixed order, then integers; complete on return (a
    /// synchronous call). This image is not modified.
    pub fn resample(&self, transform: &Transform) -> Result<Image, Error> {
        let how = transform.to_c();
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_transform(self.raw, &how, &mut raw) })?;
        Ok(Image { raw, width: transform.width, height: transform.height, origin: (0, 0) })
    }
    /// `transform_fit`, then `resample`: this image moved by `forward` (its coordinates -> the caller's target space) in the smallest result
    /// that holds all of it; the result's origin is where the target space's (0, 0) lies in it (two's complement when negative, as a crop's).
    pub fn transform(&self, forward: &[f64; 9], filter: TransformFilter, edge: BlurEdge) -> Result<Image, Error> {
        let (fitted, origin) = transform_fit(self.width, self.height, forward, filter, edge)?;
        let mut image = self.resample(&fitted)?;
        image.origin = (origin[0] as u32, origin[1] as u32);
        Ok(image)
    }
    /// `transform` by a rotation of `degrees`, clockwise on the screen (y points down), about `center` in this image's coordinates, `None` =
    /// its middle; a multiple of 90 uses the entries 0 and +-1 exactly.
    pub fn rotate(&self, degrees: f64, center: Option<[f64; 2]>, filter: TransformFilter, edge: BlurEdge) -> Result<Image, Error> {
        let [cx, cy] = center.unwrap_or([self.width as f64 / 2.0, self.height as f64 / 2.0]);
        let quarter = degrees / 90.0;
        let (c, s) = if quarter == quarter.floor() {
            [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][quarter.rem_euclid(4.0) as usize]
        } else {
            (degrees.to_radians().cos(), degrees.to_radians().sin())
        };
        self.transform(&[c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy, 0.0, 0.0, 1.0], filter, edge)
    }
    /// `crh_image_variable_blur` -> a new `Image` of one level, of this image's size under every edge, origin (0, 0): `blur` with the taps
    /// of each texel's own level, the stored code of `blur.channel` of `mask`, an image of the same size and renderer; integer and
    /// bit-exact, complete on return (a synchronous call). A mask of one value gives `blur`'s bytes. Neither image is modified.
    pub fn variable_blur(&self, mask: &Image, blur: &VariableBlur) -> Result<Image, Error> {
        let how = blur.to_c();
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_variable_blur(self.raw, mask.raw, &how, &mut raw) })?;
        Ok(Image { raw, width: self.width, height: self.height, origin: (0, 0) })
    }
    /// `crh_image_lighting` -> a new `Image` of one level, of this image's size and origin: this image's alpha as a height field lit by
    /// `light`; binary64 arithmetic in a fixed order, complete on return (a synchronous call). Diffuse results are opaque (MULTIPLY them onto
    /// a layer), specular ones premultiplied highlights (PLUS them). This image is not modified.
    pub fn lighting(&self, light: &Light, lighting: &Lighting) -> Result<Image, Error> {
        let how = lighting.to_c(light);
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_image_lighting(self.raw, &how, &mut raw) })?;
        Ok(Image { raw, width: self.width, height: self.height, origin: self.origin })
    }
    /// `lighting` with `LightingOp::Diffuse`: SVG feDiffuseLighting
    pub fn diffuse_lighting(&self, light: &Light, surface_scale: f32, constant: f32, color: [f32; 3], edge: BlurEdge) -> Result<Image, Error> {
        self.lighting(light, &Lighting { op: LightingOp::Diffuse, surface_scale, constant, specular_exponent: 1.0, color, edge })
    }
    /// `lighting` with `LightingOp::Specular`: SVG feSpecularLighting
    pub fn specular_lighting(&self, light: &Light, surface_scale: f32, constant: f32, specular_exponent: f32, color: [f32; 3], edge: BlurEdge) -> Result<Image, Error> {
        self.lighting(light, &Lighting { op: LightingOp::Specular, surface_scale, constant, specular_exponent, color, edge })
    }
}
impl Drop for Image {
    fn drop(&mut self) {
        unsafe { ffi::crh_image_destroy(self.raw) }
    }
}
/// The texels of an `Image` as the source of a Color cover, times the instance colour (include/contrast_hip.h,
/// `crh_scene_set_paints_with_images`, states the model). `matrix` maps path coordinates to texels: u = m0 x + m1 y + m2, v = m3 x + m4 y + m5.
#[derive(Clone, Copy)]
pub struct ImagePaint(pub ffi::crh_image_paint);
impl ImagePaint {
    pub fn new(image: &Image, matrix: [f32; 6], filter: Filter, spread_x: Spread, spread_y: Spread) -> Self {
        ImagePaint(ffi::crh_image_paint { image: image.raw, filter: filter as u32, spread_x: spread_x as u32, spread_y: spread_y as u32, m: matrix })
    }
    /// The path rectangle [lower, upper] onto the whole image; path y points up on the frame, so y = upper[1] is the image's row 0
    pub fn fit(image: &Image, lower: [f32; 2], upper: [f32; 2], filter: Filter) -> Self {
        let (sx, sy) = (image.width as f32 / (upper[0] - lower[0]), image.height as f32 / (upper[1] - lower[1]));
        Self::new(image, [sx, 0.0, -sx * lower[0], 0.0, -sy, sy * upper[1]], filter, Spread::Pad, Spread::Pad)
    }
    /// Host only: what `Scene::set_paints_with_images` would refuse
    pub fn validate(&self) -> Result<(), Error> {
        status(unsafe { ffi::crh_image_paint_validate(&self.0) })
    }
}
impl Scene {
    /// `instance_paint[i]` below `paints.len()` names a gradient, from there on image paint `i - paints.len()`, -1 the solid colour. Stays
    /// with the Scene until the next call (of this or of `set_paints`); the table keeps the pixels of its images.
    pub fn set_paints_with_images(&self, paints: &[Paint], image_paints: &[ImagePaint], instance_paint: &[i32]) -> Result<(), Error> {
        let table: Vec<ffi::crh_paint> = paints.iter().map(|p| p.0).collect();
        let images: Vec<ffi::crh_image_paint> = image_paints.iter().map(|p| p.0).collect();
        status(unsafe {
            ffi::crh_scene_set_paints_with_images(self.raw, table.as_ptr(), table.len() as u32, images.as_ptr(), images.len() as u32, instance_paint.as_ptr(), instance_paint.len() as u32)
        })
    }
}
impl Drop for Scene {
    fn drop(&mut self) {
        unsafe { ffi::crh_scene_destroy(self.raw) }
    }
}

/// What the reference records into a caller-owned `wgpu::RenderPass` (renderer.rs:267-355): `Shape::render` calls in order, the clip
/// depth (`Renderer::set_clip_depth`, renderer.rs:932-938) and the alpha layer in effect. `submit` runs the pass over the frame.
pub struct RenderPass<'a> {
    frame: &'a mut Frame,
    transforms: Vec<[f32; 16]>,
    colors: Vec<[f32; 4]>,
    draws: Vec<(*mut ffi::crh_scene, ffi::crh_draw)>,
    clip_depth: u32,
    alpha_layer: u32,
}
impl<'a> RenderPass<'a> {
    pub fn new(frame: &'a mut Frame) -> Self {
        Self { frame, transforms: Vec::new(), colors: Vec::new(), draws: Vec::new(), clip_depth: 0, alpha_layer: 0 }
    }
    /// One entry of the instance buffers the reference binds at vertex slots 0 and 1 (column-major mat4 + straight-alpha colour,
    /// shaders.wgsl:13-27); returns its index for `Shape::render`'s `instance_indices`
    pub fn push_instance(&mut self, transform: [f32; 16], color: [f32; 4]) -> u32 {
        self.transforms.push(transform);
        self.colors.push(color);
        self.transforms.len() as u32 - 1
    }
    /// renderer.rs:932-938
    pub fn set_clip_depth(&mut self, renderer: &Renderer, clip_depth: usize) -> Result<(), Error> {
        if clip_depth >= (1 << renderer.config.clip_nesting_counter_bits) {
            return Err(Error::ClipStackOverflow);
        }
        self.clip_depth = clip_depth as u32;
        Ok(())
    }
    /// renderer.rs:940-977 / :979-985: the alpha layer of the following Save / Scale / RestoreAlphaContext draws
    pub fn set_alpha_layer(&mut self, renderer: &Renderer, alpha_layer: usize) -> Result<(), Error> {
        if alpha_layer >= renderer.config.alpha_layer_count {
            return Err(Error::TooManyNestedOpacityGroups);
        }
        self.alpha_layer = alpha_layer as u32;
        Ok(())
    }
    /// Runs the recorded draws, in order, as one `crh_scene_render_draws` per run of draws of the same Shape object. Clip nesting counters,
    /// winding counters, saved alpha contexts and the colour of every sample stay with the [`Frame`] between those calls (the library keeps
    /// them in HBM from the first pass that ends with state left over until `Frame::clear`), so the reference's pattern — `a.render(Stencil)`,
    /// `set_clip_depth(1)`, `a.render(Clip)`, other Shapes, `set_clip_depth(0)`, `a.render(UnClip)` (renderer.rs:257-266) — works with `a`
    /// and the clipped Shapes as separate objects, as does an opacity group around other Shapes (renderer.rs:941-985).
    pub fn submit(self) -> Result<(), Error> {
        if self.draws.windows(2).any(|pair| pair[0].0 != pair[1].0) {
            // the pass spans objects: every sample's colour and stencil stay with the frame from its first draw on
            status(unsafe { ffi::crh_frame_keep_pass_state(self.frame.raw) })?;
        }
        let mut begin = 0;
        while begin < self.draws.len() {
            let scene = self.draws[begin].0;
            let mut end = begin;
            while end < self.draws.len() && self.draws[end].0 == scene {
                end += 1;
            }
            let draws: Vec<ffi::crh_draw> = self.draws[begin..end].iter().map(|(_, draw)| *draw).collect();
            status(unsafe {
                ffi::crh_scene_render_draws(scene, self.frame.raw, self.transforms.as_ptr() as *const f32, self.colors.as_ptr() as *const f32, self.transforms.len() as u32, draws.as_ptr(), draws.len() as u32)
            })?;
            begin = end;
        }
        Ok(())
    }
}

// ------------------------------------------------------------------------------------------------ multi-GPU (no counterpart upstream)

/// One rank of the framebuffer exchange (include/contrast_hip.h `crh_comm_*`): one process per GPU, rank g renders the Shape range
/// [`Comm::shard`] gives it into a private [`Frame`]; [`Comm::exchange`] composites the layers in rank order into rank 0's result.
pub struct Comm {
    raw: *mut ffi::crh_comm,
    rank: u32,
}
impl Comm {
    /// Rank 0 creates the id and hands it to the other ranks by any means
    pub fn unique_id() -> [u8; ffi::CRH_COMM_ID_BYTES] {
        let mut id = [0u8; ffi::CRH_COMM_ID_BYTES];
        status(unsafe { ffi::crh_comm_unique_id(id.as_mut_ptr() as *mut _) }).unwrap();
        id
    }
    pub fn new(renderer: &Renderer, rank: u32, world: u32, unique_id: &[u8; ffi::CRH_COMM_ID_BYTES]) -> Result<Self, Error> {
        let mut raw = ptr::null_mut();
        status(unsafe { ffi::crh_comm_create(renderer.raw, rank, world, unique_id.as_ptr() as *const _, &mut raw) })?;
        Ok(Self { raw, rank })
    }
    /// The contiguous, order-preserving Shape range of a rank
    pub fn shard(n_items: u32, rank: u32, world: u32) -> Range<u32> {
        let (mut begin, mut end) = (0u32, 0u32);
        status(unsafe { ffi::crh_comm_shard(n_items, rank, world, &mut begin, &mut end) }).unwrap();
        begin..end
    }
    /// The pixel rows of rank `rank`'s slab of a frame `height` pixels high (whole 16-pixel tile rows)
    pub fn slab_rows(height: u32, rank: u32, world: u32) -> Range<u32> {
        let (mut begin, mut end) = (0u32, 0u32);
        status(unsafe { ffi::crh_comm_slab_rows(height, rank, world, &mut begin, &mut end) }).unwrap();
        begin..end
    }
    /// Collective. `result` must be `Some` on rank 0 and `None` elsewhere.
    pub fn exchange(&self, layer: &mut Frame, result: Option<&mut Frame>) -> Result<(), Error> {
        assert_eq!(self.rank == 0, result.is_some());
        status(unsafe { ffi::crh_frame_exchange(self.raw, layer.raw, result.map_or(ptr::null_mut(), |frame| frame.raw)) })
    }
    /// Collective, the tile split: every rank's slab of rows (`Frame::set_tile_rows`) straight into rank 0's `result`.
    pub fn gather_slabs(&self, layer: &mut Frame, result: Option<&mut Frame>) -> Result<(), Error> {
        assert_eq!(self.rank == 0, result.is_some());
        status(unsafe { ffi::crh_frame_gather_slabs(self.raw, layer.raw, result.map_or(ptr::null_mut(), |frame| frame.raw)) })
    }
}
impl Drop for Comm {
    fn drop(&mut self) {
        unsafe { ffi::crh_comm_destroy(self.raw) }
    }
}
