"""Host-side mirror of the reference's renderer.rs API over the C ABI (ctypes): Renderer, Shape, RenderOperation — plus the
batch forms (Scene = many Shapes built and rendered together, Frame = the render pass attachments).

All arithmetic runs in libcontrast_hip.so on the GPU; this module only marshals arguments.
"""
import ctypes as C
import dataclasses
import math
from dataclasses import dataclass
from enum import IntEnum, IntFlag
from typing import ClassVar, Optional, Tuple

import numpy as np

from . import _ffi
from ._ffi import ContrastError, check
from .path import batch_from_shapes


class RenderOperation(IntEnum):  # renderer.rs:145-160
    Stencil = 0
    Clip = 1
    UnClip = 2
    Color = 3
    SaveAlphaContext = 4
    ScaleAlphaContext = 5
    RestoreAlphaContext = 6


class Cull(IntEnum):  # Option<wgpu::Face> of Configuration::cull_mode (renderer.rs:383-384); front = counter-clockwise on screen
    Disabled = 0
    Front = 1
    Back = 2


class Compare(IntEnum):  # wgpu::CompareFunction of Configuration::depth_compare (renderer.rs:387-388): fragment depth OP stored depth
    Always = 0
    Never = 1
    Less = 2
    Equal = 3
    LessEqual = 4
    Greater = 5
    NotEqual = 6
    GreaterEqual = 7


class BlendFactor(IntEnum):  # wgpu::BlendFactor, same order (crh_blend_factor)
    Zero = 0
    One = 1
    Src = 2
    OneMinusSrc = 3
    SrcAlpha = 4
    OneMinusSrcAlpha = 5
    Dst = 6
    OneMinusDst = 7
    DstAlpha = 8
    OneMinusDstAlpha = 9
    SrcAlphaSaturated = 10
    Constant = 11
    OneMinusConstant = 12
    Src1 = 13  # 13-16: dual-source factors; the colour cover has one output, so the renderer refuses them (Unsupported)
    OneMinusSrc1 = 14
    Src1Alpha = 15
    OneMinusSrc1Alpha = 16


class BlendOperation(IntEnum):  # wgpu::BlendOperation (crh_blend_operation)
    Add = 0
    Subtract = 1
    ReverseSubtract = 2
    Min = 3
    Max = 4


@dataclass(frozen=True)
class BlendComponent:  # wgpu::BlendComponent; the default is BlendComponent::REPLACE
    src_factor: int = BlendFactor.One
    dst_factor: int = BlendFactor.Zero
    operation: int = BlendOperation.Add
    REPLACE: ClassVar["BlendComponent"]
    OVER: ClassVar["BlendComponent"]

    def to_c(self):
        return _ffi.BlendComponentC(int(self.src_factor), int(self.dst_factor), int(self.operation))


BlendComponent.REPLACE = BlendComponent(BlendFactor.One, BlendFactor.Zero, BlendOperation.Add)
BlendComponent.OVER = BlendComponent(BlendFactor.One, BlendFactor.OneMinusSrcAlpha, BlendOperation.Add)


@dataclass(frozen=True)
class BlendState:  # wgpu::BlendState
    color: BlendComponent = BlendComponent.REPLACE
    alpha: BlendComponent = BlendComponent.REPLACE
    REPLACE: ClassVar["BlendState"]
    ALPHA_BLENDING: ClassVar["BlendState"]
    PREMULTIPLIED_ALPHA_BLENDING: ClassVar["BlendState"]


BlendState.REPLACE = BlendState(BlendComponent.REPLACE, BlendComponent.REPLACE)
BlendState.ALPHA_BLENDING = BlendState(BlendComponent(BlendFactor.SrcAlpha, BlendFactor.OneMinusSrcAlpha, BlendOperation.Add), BlendComponent.OVER)
BlendState.PREMULTIPLIED_ALPHA_BLENDING = BlendState(BlendComponent.OVER, BlendComponent.OVER)


class ColorWrites(IntFlag):  # wgpu::ColorWrites
    RED = 1
    GREEN = 2
    BLUE = 4
    ALPHA = 8
    COLOR = 7
    ALL = 15


class TextureFormat(IntEnum):
    """wgpu::TextureFormat of the colour target (renderer.rs:380-382). The value is the frame format that keeps f32 colours within a pass
    (FORMAT_*); `attachment` is the one that rounds every write, as a hardware blender does."""
    Rgba8Unorm = 0
    Bgra8Unorm = 3
    Rgba8UnormSrgb = 5
    Bgra8UnormSrgb = 7

    @property
    def attachment(self):
        return FORMAT_RGBA8_ATTACHMENT if self == TextureFormat.Rgba8Unorm else int(self) + 1


@dataclass(frozen=True)
class ColorTargetState:
    """wgpu::ColorTargetState of the colour cover (renderer.rs:380-382): `blend` None = the source replaces the target.
    `constant` stands for RenderPass::set_blend_constant, which this library keeps with the renderer. `format` is kept host-side: it is
    the format Frame(renderer, ...) creates by default (the C ABI names a frame's format at crh_frame_create_format)."""
    blend: Optional[BlendState] = None
    write_mask: int = ColorWrites.ALL
    constant: Tuple[float, float, float, float] = (0.0, 0.0, 0.0, 0.0)
    format: TextureFormat = TextureFormat.Rgba8Unorm

    def to_c(self):
        b = self.blend or BlendState.REPLACE
        return _ffi.ColorTargetStateC(1 if self.blend is not None else 0, b.color.to_c(), b.alpha.to_c(), int(self.write_mask),
                                      (C.c_float * 4)(*[float(v) for v in self.constant]))

    @staticmethod
    def from_c(c):
        comp = lambda x: BlendComponent(BlendFactor(x.src_factor), BlendFactor(x.dst_factor), BlendOperation(x.operation))
        blend = BlendState(comp(c.color), comp(c.alpha)) if c.blend_enabled else None
        return ColorTargetState(blend, ColorWrites(c.write_mask), tuple(float(v) for v in c.constant))


class Spread(IntEnum):  # crh_spread: what a gradient does outside [0, 1]
    Pad = 0
    Repeat = 1
    Reflect = 2


class PaintKind(IntEnum):  # crh_paint_kind
    Linear = 1
    Radial = 2
    Conic = 4  # (3 is not a kind: crh_paint_validate refuses it)


@dataclass(frozen=True)
class GradientStop:  # crh_gradient_stop: offset in [0, 1], straight RGBA
    offset: float
    color: Tuple[float, float, float, float]


@dataclass(frozen=True)
class Paint:
    """crh_paint: a linear, radial or conic gradient in the Shape's path coordinates, the source of a Color cover in place of the instance's one
    colour (include/contrast_hip.h crh_scene_set_paints states the model). Stops: GradientStop or (offset, (r, g, b, a)) pairs, at most 8."""
    kind: int
    spread: int
    p0: Tuple[float, float]
    p1: Tuple[float, float]
    stops: Tuple[GradientStop, ...]

    @staticmethod
    def _stops(stops):
        return tuple(s if isinstance(s, GradientStop) else GradientStop(float(s[0]), tuple(float(v) for v in s[1])) for s in stops)

    @staticmethod
    def linear(p0, p1, stops, spread=Spread.Pad):
        """t = 0 at p0, t = 1 at p1."""
        return Paint(PaintKind.Linear, spread, (float(p0[0]), float(p0[1])), (float(p1[0]), float(p1[1])), Paint._stops(stops))

    @staticmethod
    def radial(center, radius, stops, spread=Spread.Pad):
        """t = distance from `center` / radius."""
        return Paint(PaintKind.Radial, spread, (float(center[0]), float(center[1])), (float(radius), 0.0), Paint._stops(stops))

    @staticmethod
    def conic(center, start, end, stops, spread=Spread.Pad):
        """t = 0 on the ray from `center` at the angle `start`, t = 1 at `end`: radians, from +x towards +y in the Shape's path coordinates,
        0 < |end - start| <= 2 pi; end < start reads the stops clockwise."""
        return Paint(PaintKind.Conic, spread, (float(center[0]), float(center[1])), (float(start), float(end)), Paint._stops(stops))

    def to_c(self):
        if not 0 < len(self.stops) <= _ffi.MAX_GRADIENT_STOPS:
            raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"a paint has 1..{_ffi.MAX_GRADIENT_STOPS} stops, not {len(self.stops)}")
        c = _ffi.PaintC()
        c.kind, c.spread, c.n_stops = int(self.kind), int(self.spread), len(self.stops)
        c.p0[0], c.p0[1], c.p1[0], c.p1[1] = self.p0[0], self.p0[1], self.p1[0], self.p1[1]
        for i, s in enumerate(self.stops):
            c.stops[i].offset = s.offset
            for ch in range(4):
                c.stops[i].color[ch] = s.color[ch]
        return c

    def validate(self):
        """crh_paint_validate (host only): raises ContrastError for what crh_scene_set_paints would refuse."""
        check(_ffi.load_library().crh_paint_validate(C.byref(self.to_c())))


@dataclass
class Configuration:  # renderer.rs:380-405 (fields that change results on this path)
    msaa_sample_count: int = 1  # 1, 2, 4 or 8, standard sample locations (include/contrast_hip.h); any other count: ContrastError (CRH_ERR_UNSUPPORTED)
    clip_nesting_counter_bits: int = 4
    winding_counter_bits: int = 4
    alpha_layer_count: int = 0
    cull_mode: int = Cull.Disabled          # the three depth / cull fields act on the colour cover only (renderer.rs:743-745)
    depth_compare: int = Compare.Always
    depth_write_enabled: bool = False
    blending: Optional[ColorTargetState] = None  # the colour cover's blend state (renderer.rs:380-382); None = the showcase's premultiplied "over"


class Renderer:
    """Renderer::new (renderer.rs:432): validates the stencil bit budget, owns one HIP stream on `device`."""

    def __init__(self, config: Configuration = None, device: int = 0):
        self.lib = _ffi.load_library()
        config = config or Configuration()
        c = _ffi.ConfigC(config.msaa_sample_count, config.clip_nesting_counter_bits, config.winding_counter_bits, config.alpha_layer_count,
                         int(config.cull_mode), int(config.depth_compare), 1 if config.depth_write_enabled else 0)
        handle = C.c_void_p()
        blending = C.byref(config.blending.to_c()) if config.blending is not None else None
        check(self.lib.crh_renderer_create_blended(C.byref(c), blending, device, C.byref(handle)))
        self.handle = handle
        self.config = config
        self.device = device

    def get_config(self):
        return self.config

    def get_blending(self) -> ColorTargetState:
        """The colour cover's blend state the renderer was created with (the "over" state when Configuration.blending is None)."""
        out = _ffi.ColorTargetStateC()
        check(self.lib.crh_renderer_get_blending(self.handle, C.byref(out)))
        state = ColorTargetState.from_c(out)
        if self.config.blending is not None:
            state = dataclasses.replace(state, format=self.config.blending.format)
        return state

    def synchronize(self):
        check(self.lib.crh_renderer_synchronize(self.handle))

    def enable_timing(self, enabled=True):
        """True / 1: HIP events around every kernel; 2: around the raster lane's kernels only (cheap enough for a timed loop); False / 0: off"""
        check(self.lib.crh_renderer_enable_timing(self.handle, int(enabled)))

    def kernel_times(self):
        """[(kernel name, milliseconds, algorithmic bytes)] of the last tessellate / render call (HIP events on the renderer's stream)."""
        n = C.c_uint32()
        check(self.lib.crh_renderer_kernel_times(self.handle, None, 0, C.byref(n)))
        out = (_ffi.KernelTimeC * max(1, n.value))()
        check(self.lib.crh_renderer_kernel_times(self.handle, out, n.value, C.byref(n)))
        return [(out[i].name.decode(), out[i].ms, out[i].algorithmic_bytes) for i in range(n.value)]

    def selftest_fmath(self, fn, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(a if b is None else b, dtype=np.float32)
        out = np.zeros_like(a)
        fp = C.POINTER(C.c_float)
        check(self.lib.crh_selftest_fmath(self.handle, fn, a.ctypes.data_as(fp), b.ctypes.data_as(fp), out.ctypes.data_as(fp), a.size))
        return out

    def selftest_srgb(self, x):
        """The raster kernels' sRGB codec run on the GPU: -> (encode(x) as uint8, decode of the 256 codes as float32)."""
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        codes = np.zeros(x.size, dtype=np.uint8)
        decoded = np.zeros(256, dtype=np.float32)
        check(self.lib.crh_selftest_srgb(self.handle, x.ctypes.data_as(C.POINTER(C.c_float)), codes.ctypes.data_as(C.POINTER(C.c_uint8)), x.size,
                                         decoded.ctypes.data_as(C.POINTER(C.c_float))))
        return codes, decoded

    def __del__(self):
        if getattr(self, "handle", None) and self.lib is not None:
            self.lib.crh_renderer_destroy(self.handle)
            self.handle = None


FORMAT_RGBA8, FORMAT_RGBA16F, FORMAT_RGBA8_ATTACHMENT = 0, 1, 2  # (2: RGBA8 storage, every blend rounded to 8 bits like an Rgba8Unorm attachment)
# the other colour targets (include/contrast_hip.h): B G R A byte order and / or sRGB-encoded rgb; *_ATTACHMENT rounds every write
FORMAT_BGRA8, FORMAT_BGRA8_ATTACHMENT, FORMAT_RGBA8_SRGB, FORMAT_RGBA8_SRGB_ATTACHMENT, FORMAT_BGRA8_SRGB, FORMAT_BGRA8_SRGB_ATTACHMENT = 3, 4, 5, 6, 7, 8


class Frame:
    """The colour attachment (premultiplied; RGBA8, BGRA8, their sRGB forms, or RGBA16F for the layers of the multi-GPU exchange) and
    per-sample winding state of one render pass. `format` None = the renderer's Configuration.blending.format (FORMAT_RGBA8 without one)."""

    def __init__(self, renderer: Renderer, width: int, height: int, format: Optional[int] = None):
        if format is None:
            blending = renderer.config.blending
            format = int(blending.format) if blending is not None else FORMAT_RGBA8
        format = int(format)
        self.renderer = renderer
        self.lib = renderer.lib
        self.width, self.height, self.format = width, height, format
        handle = C.c_void_p()
        check(self.lib.crh_frame_create_format(renderer.handle, width, height, format, C.byref(handle)))
        self.handle = handle

    def clear(self):
        check(self.lib.crh_frame_clear(self.handle))

    def keep_pass_state(self):
        """From now until clear(): clip / winding counters, saved alphas and the f32 colour of every sample stay with the frame between
        passes (the reference's caller-owned stencil attachment and alpha layers, renderer.rs:148-158, 257-266)."""
        check(self.lib.crh_frame_keep_pass_state(self.handle))

    def synchronize(self):
        """Waits for the last render into this frame only (the next frame of a double-buffered loop keeps running)."""
        check(self.lib.crh_frame_synchronize(self.handle))

    def set_tile_rows(self, row_begin, row_end):
        """The tile split of the multi-GPU path: passes into this frame draw the pixel rows [row_begin, row_end) only (whole 16-pixel tile rows;
        slab_rows() gives a rank's), the rest stays transparent; (0, height) gives the whole frame back."""
        check(self.lib.crh_frame_set_tile_rows(self.handle, int(row_begin), int(row_end)))

    def clear_depth(self, value=1.0):
        """LoadOp::Clear(value) of the depth attachment (main.rs:223-226); it exists when the configuration tests or writes depth."""
        check(self.lib.crh_frame_clear_depth(self.handle, value))

    def upload_depth(self, depth):
        """The depth of the 3-D scene the Shapes are decals in: [height, width] floats, replicated to every sample."""
        d = np.ascontiguousarray(depth, dtype=np.float32).reshape(self.height, self.width)
        check(self.lib.crh_frame_upload_depth(self.handle, d.ctypes.data_as(C.POINTER(C.c_float))))

    def download_depth(self):
        """-> [height, width, msaa_sample_count] float32."""
        out = np.zeros((self.height, self.width, self.renderer.config.msaa_sample_count), dtype=np.float32)
        check(self.lib.crh_frame_download_depth(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def upload(self, image):
        """LoadOp::Load of caller content: [height, width, 4] premultiplied 8-bit pixels in the frame's storage order (B G R A for a BGRA
        format; sRGB-encoded rgb for an sRGB one) replace the pixels, stencil, alpha layers and pass state are
        reset as by clear(), depth is left alone; the next pass loads the pixels. An RGBA16F frame, a frame restricted by set_tile_rows() and an
        image of another size are refused (InvalidArgument)."""
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.shape != (self.height, self.width, 4):
            raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"an upload takes a ({self.height}, {self.width}, 4) uint8 image, not {image.shape} {image.dtype}")
        data = np.ascontiguousarray(image)
        check(self.lib.crh_frame_upload(self.handle, data.ctypes.data))

    def load_image(self, image):
        """crh_frame_load_image: upload() with the bytes taken from level 0 of an Image on the device — how a composed layer comes back into
        a frame without a round trip through the host. The same reset and the same frames refused as upload(); an image of another size or
        of another renderer is refused (InvalidArgument). Complete when this returns: the image may be destroyed afterwards."""
        check(self.lib.crh_frame_load_image(self.handle, image.handle))

    def download(self):
        """-> [height, width, 4] uint8 in the frame's storage order (R G B A, or B G R A for a BGRA format) or float16 (an RGBA16F frame)."""
        if self.format == FORMAT_RGBA16F:
            out = np.zeros((self.height, self.width, 4), dtype=np.float16)
            check(self.lib.crh_frame_download_f16(self.handle, out.ctypes.data))
            return out
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        check(self.lib.crh_frame_download(self.handle, out.ctypes.data))
        return out

    def device_pointer(self):
        p = C.c_void_p()
        check(self.lib.crh_frame_device_pointer(self.handle, C.byref(p)))
        return p.value

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.crh_frame_destroy(self.handle)
            self.handle = None


class Filter(IntEnum):  # CRH_FILTER_*: the two base filters, and each with CRH_FILTER_MIPMAP (0x100) OR-ed on
    Nearest = 0
    Linear = 1
    NearestMipmap = 0x100
    LinearMipmap = 0x101


class BlurEdge(IntEnum):  # crh_blur_edge: what a blur reads outside the image
    Transparent = 0  # (0, 0, 0, 0); the result grows by the radius on every side
    Pad = 1
    Repeat = 2
    Reflect = 3


MAX_BLUR_SIGMA = 64.0   # CRH_MAX_BLUR_SIGMA
MAX_BLUR_RADIUS = 192   # CRH_MAX_BLUR_RADIUS


def blur_taps(sigma):
    """crh_blur_taps (host only) -> (taps, radius): the integer taps q[0 .. radius] of one axis of Image.blur as a uint32 array, radius =
    ceil(3 sigma); symmetric about q[0], summing to exactly 65536 over the 2 radius + 1 positions (include/contrast_hip.h crh_image_blur)."""
    lib = _ffi.load_library()
    taps = np.zeros(MAX_BLUR_RADIUS + 1, dtype=np.uint32)
    radius = C.c_uint32()
    check(lib.crh_blur_taps(float(sigma), taps.ctypes.data_as(C.POINTER(C.c_uint32)), len(taps), C.byref(radius)))
    return taps[:int(radius.value) + 1].copy(), int(radius.value)


class CompositeOp(IntEnum):  # crh_composite_op: Porter-Duff, (fa, fb) in include/contrast_hip.h
    Clear = 0
    Copy = 1
    Dst = 2
    SrcOver = 3
    DstOver = 4
    SrcIn = 5
    DstIn = 6
    SrcOut = 7
    DstOut = 8
    SrcAtop = 9
    DstAtop = 10
    Xor = 11
    Plus = 12


class BlendMode(IntEnum):  # crh_blend_mode: the W3C compositing-1 separable modes with a polynomial premultiplied form
    Normal = 0
    Multiply = 1
    Screen = 2
    Overlay = 3
    Darken = 4
    Lighten = 5
    HardLight = 6
    Difference = 7
    Exclusion = 8


def composite_texels(source, backdrop, op=CompositeOp.SrcOver, mode=BlendMode.Normal, opacity=1.0):
    """crh_composite_texels (host only): the compositing rule of Image.composite on n texel pairs, two (n, 4) uint8 arrays of premultiplied
    RGBA8 -> an (n, 4) uint8 array (include/contrast_hip.h crh_image_composite states the rule)."""
    source, backdrop = np.ascontiguousarray(source), np.ascontiguousarray(backdrop)
    for texels in (source, backdrop):
        if texels.dtype != np.uint8 or texels.ndim != 2 or texels.shape[1] != 4 or texels.shape != source.shape:
            raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"composite_texels takes two (n, 4) uint8 arrays of one length, not {source.shape} {source.dtype} and {backdrop.shape} {backdrop.dtype}")
    how = _ffi.CompositeC(int(op), int(mode), float(opacity), 0, 0)
    out = np.empty_like(source)
    check(_ffi.load_library().crh_composite_texels(C.byref(how), source.ctypes.data, backdrop.ctypes.data, source.shape[0], out.ctypes.data))
    return out


COLOR_MATRIX_MAX = 16.0  # CRH_COLOR_MATRIX_MAX


class ColorMatrix:
    """The 4 x 5 matrices of Image.color_filter as lists of 20 floats, row-major: rows r', g', b', a', columns r, g, b, a, 1 on unpremultiplied
    colours in [0, 1]. The coefficients are those of SVG filter effects (feColorMatrix), computed in float64 and rounded to f32 once."""

    @staticmethod
    def _rows(rows):
        return [float(np.float32(v)) for row in rows for v in row]

    @staticmethod
    def identity():
        return ColorMatrix._rows([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0]])

    @staticmethod
    def saturate(s):
        """feColorMatrix type="saturate": s = 0 is grayscale, 1 the identity, above 1 oversaturates"""
        s = float(s)
        return ColorMatrix._rows([[0.213 + 0.787 * s, 0.715 - 0.715 * s, 0.072 - 0.072 * s, 0, 0],
                                  [0.213 - 0.213 * s, 0.715 + 0.285 * s, 0.072 - 0.072 * s, 0, 0],
                                  [0.213 - 0.213 * s, 0.715 - 0.715 * s, 0.072 + 0.928 * s, 0, 0],
                                  [0, 0, 0, 1, 0]])

    @staticmethod
    def hue_rotate(degrees):
        """feColorMatrix type="hueRotate": the hue turned by `degrees`"""
        angle = math.radians(float(degrees))
        c, s = math.cos(angle), math.sin(angle)
        return ColorMatrix._rows([[0.213 + c * 0.787 - s * 0.213, 0.715 - c * 0.715 - s * 0.715, 0.072 - c * 0.072 + s * 0.928, 0, 0],
                                  [0.213 - c * 0.213 + s * 0.143, 0.715 + c * 0.285 + s * 0.140, 0.072 - c * 0.072 - s * 0.283, 0, 0],
                                  [0.213 - c * 0.213 - s * 0.787, 0.715 - c * 0.715 + s * 0.715, 0.072 + c * 0.928 + s * 0.072, 0, 0],
                                  [0, 0, 0, 1, 0]])

    @staticmethod
    def luminance_to_alpha():
        """feColorMatrix type="luminanceToAlpha": the colour becomes (0, 0, 0), the alpha the luminance — SVG's default mask type"""
        return ColorMatrix._rows([[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0.2125, 0.7154, 0.0721, 0, 0]])

    @staticmethod
    def flood(r, g, b, a):
        """Every texel takes the straight colour (r, g, b) and a times its alpha: the colour of a drop shadow"""
        return ColorMatrix._rows([[0, 0, 0, 0, r], [0, 0, 0, 0, g], [0, 0, 0, 0, b], [0, 0, 0, a, 0]])

    @staticmethod
    def opacity(a):
        return ColorMatrix._rows([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, a, 0]])


def _color_filter_arguments(matrix, tables):
    """-> (a c_float * 20 or None, a contiguous uint8 array of 1024 or None)"""
    m = t = None
    if matrix is not None:
        values = [float(v) for v in np.asarray(matrix, dtype=np.float64).ravel()]
        if len(values) != 20:
            raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"a colour matrix has 20 coefficients, not {len(values)}")
        m = (C.c_float * 20)(*values)
    if tables is not None:
        t = np.ascontiguousarray(tables)
        if t.dtype != np.uint8 or t.size != 1024:
            raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"colour tables are 1024 uint8 values (r, g, b, a: 256 each), not {t.shape} {t.dtype}")
    return m, t


def color_filter_texels(texels, matrix=None, tables=None):
    """crh_color_filter_texels (host only): the colour-filter rule of Image.color_filter on an (n, 4) uint8 array of premultiplied RGBA8 ->
    an (n, 4) uint8 array (include/contrast_hip.h crh_image_color_filter states the rule)."""
    texels = np.ascontiguousarray(texels)
    if texels.dtype != np.uint8 or texels.ndim != 2 or texels.shape[1] != 4:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"color_filter_texels takes an (n, 4) uint8 array, not {texels.shape} {texels.dtype}")
    m, t = _color_filter_arguments(matrix, tables)
    out = np.empty_like(texels)
    check(_ffi.load_library().crh_color_filter_texels(m, None if t is None else t.ctypes.data_as(C.POINTER(C.c_uint8)), texels.ctypes.data, texels.shape[0], out.ctypes.data))
    return out


class MorphologyOp(IntEnum):  # crh_morphology_op: the per-channel min or max over the window
    Erode = 0
    Dilate = 1


MAX_MORPHOLOGY_RADIUS = 192  # CRH_MAX_MORPHOLOGY_RADIUS


def morphology_size(width, height, op, radius_x, radius_y=None, edge=BlurEdge.Transparent):
    """crh_morphology_size (host only) -> (width, height) of the result of Image.morphology on a width x height image: grown by the radius on
    every side for MorphologyOp.Dilate under BlurEdge.Transparent, else the same. Raises ContrastError for what Image.morphology refuses."""
    radius_y = radius_x if radius_y is None else radius_y
    w, h = C.c_uint32(), C.c_uint32()
    check(_ffi.load_library().crh_morphology_size(int(width), int(height), int(op), int(radius_x), int(radius_y), int(edge), C.byref(w), C.byref(h)))
    return int(w.value), int(h.value)


def morphology_texels(pixels, op, radius_x, radius_y=None, edge=BlurEdge.Transparent):
    """crh_morphology_texels (host only): the rule of Image.morphology on a (height, width, 4) uint8 array -> the (height', width', 4) uint8
    result (include/contrast_hip.h crh_image_morphology states the rule). radius_y=None means radius_x."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 4:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"morphology_texels takes a (height, width, 4) uint8 array, not {pixels.shape} {pixels.dtype}")
    radius_y = radius_x if radius_y is None else radius_y
    w, h = morphology_size(pixels.shape[1], pixels.shape[0], op, radius_x, radius_y, edge)
    out = np.empty((h, w, 4), dtype=np.uint8)
    check(_ffi.load_library().crh_morphology_texels(pixels.shape[1], pixels.shape[0], pixels.ctypes.data, int(op), int(radius_x), int(radius_y), int(edge), out.ctypes.data))
    return out


MAX_CONVOLVE_ORDER = 15    # CRH_MAX_CONVOLVE_ORDER
CONVOLVE_MAX_GAIN = 64.0   # CRH_CONVOLVE_MAX_GAIN


class ConvolveKernel:
    """Kernel matrices of Image.convolve as lists of rows, in SVG's orientation (feConvolveMatrix's kernelMatrix carries over unchanged). With
    divisor=None Image.convolve divides by the sum of the entries, or by 1 where that sum is 0, as SVG does."""

    @staticmethod
    def identity():
        return [[1.0]]

    @staticmethod
    def sharpen(amount=1.0):
        """The source plus `amount` times its difference from its four neighbours' mean: entries sum to 1"""
        a = float(amount)
        return [[0.0, -a, 0.0], [-a, 1.0 + 4.0 * a, -a], [0.0, -a, 0.0]]

    @staticmethod
    def box(n):
        """The mean of n x n texels (divisor=None divides by n * n)"""
        return [[1.0] * int(n) for _ in range(int(n))]

    @staticmethod
    def emboss():
        return [[-2.0, -1.0, 0.0], [-1.0, 1.0, 1.0], [0.0, 1.0, 2.0]]

    @staticmethod
    def laplacian():
        """5 of 9 taps; the entries sum to 0: use a bias of 0.5 to see both signs, preserve_alpha=True to keep the layer's shape"""
        return [[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]]

    @staticmethod
    def sobel_x():
        """6 of 9 taps: the horizontal gradient"""
        return [[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]

    @staticmethod
    def sobel_y():
        return [[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]]


def _convolve_arguments(kernel, divisor, bias, target, edge, preserve_alpha):
    """-> (ConvolveC, the c_float array its kernel points to: keep it alive for as long as the struct is used)"""
    k = np.asarray(kernel, dtype=np.float32)
    if k.ndim != 2 or k.size == 0:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"a convolution kernel is a 2-D array of at least one entry, not {k.shape}")
    order_y, order_x = k.shape
    if divisor is None:  # SVG: the sum of the entries, or 1 if that is 0
        total = float(np.float32(np.asarray(kernel, dtype=np.float64).sum()))
        divisor = total if total != 0.0 else 1.0
    target_x, target_y = (order_x // 2, order_y // 2) if target is None else target
    values = (C.c_float * k.size)(*[float(v) for v in k.ravel()])
    how = _ffi.ConvolveC(order_x, order_y, int(target_x), int(target_y), C.cast(values, C.POINTER(C.c_float)), float(divisor), float(bias), int(edge), int(preserve_alpha))
    return how, values


def convolve_coefficients(kernel, divisor=None, bias=0.0):
    """crh_convolve_coefficients (host only) -> (k, bias_k): the quantised kernel as an int32 array of the kernel's shape, k = floor(kernel /
    divisor * 65536 + 0.5), and floor(bias * 65536 + 0.5). Raises ContrastError for what Image.convolve refuses."""
    how, values = _convolve_arguments(kernel, divisor, bias, None, BlurEdge.Pad, False)
    k = np.zeros((how.order_y, how.order_x), dtype=np.int32)
    bias_k = C.c_int32()
    check(_ffi.load_library().crh_convolve_coefficients(C.byref(how), k.ctypes.data_as(C.POINTER(C.c_int32)), k.size, C.byref(bias_k)))
    return k, int(bias_k.value)


def convolve_texels(pixels, kernel, divisor=None, bias=0.0, target=None, edge=BlurEdge.Pad, preserve_alpha=False):
    """crh_convolve_texels (host only): the rule of Image.convolve on a (height, width, 4) uint8 array -> a (height, width, 4) uint8 array
    (include/contrast_hip.h crh_image_convolve states the rule)."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 4:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"convolve_texels takes a (height, width, 4) uint8 array, not {pixels.shape} {pixels.dtype}")
    how, values = _convolve_arguments(kernel, divisor, bias, target, edge, preserve_alpha)
    out = np.empty_like(pixels)
    check(_ffi.load_library().crh_convolve_texels(pixels.shape[1], pixels.shape[0], pixels.ctypes.data, C.byref(how), out.ctypes.data))
    return out


class LightingOp(IntEnum):  # crh_lighting_op
    Diffuse = 0
    Specular = 1


class LightKind(IntEnum):  # crh_light_kind
    Distant = 0
    Point = 1
    Spot = 2


@dataclass(frozen=True)
class DistantLight:
    """A light infinitely far away (SVG feDistantLight): azimuth in the image plane from the x axis towards y (down), elevation above the
    plane, both in degrees."""
    azimuth: float = 0.0
    elevation: float = 0.0


@dataclass(frozen=True)
class PointLight:
    """A light at (x, y, z) in the image's texel space, x right, y down, z towards the viewer (SVG fePointLight)."""
    x: float = 0.0
    y: float = 0.0
    z: float = 0.0


@dataclass(frozen=True)
class SpotLight:
    """A light at `position` that shines towards `points_at` (SVG feSpotLight): its colour falls off as the cosine to the axis raised to
    `exponent`, and with cone_angle (degrees, in (0, 90]; 0 = no cone) is cut off outside the cone."""
    position: Tuple[float, float, float] = (0.0, 0.0, 1.0)
    points_at: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    exponent: float = 1.0
    cone_angle: float = 0.0


def _lighting_arguments(light, op, surface_scale, constant, specular_exponent, color, edge):
    """-> LightingC; the fields the light does not use stay 0"""
    how = _ffi.LightingC()
    how.op, how.edge = int(op), int(edge)
    how.surface_scale, how.constant, how.specular_exponent = float(surface_scale), float(constant), float(specular_exponent)
    how.color = (C.c_float * 3)(*[float(v) for v in color])
    if isinstance(light, DistantLight):
        how.light, how.azimuth, how.elevation = LightKind.Distant, float(light.azimuth), float(light.elevation)
    elif isinstance(light, PointLight):
        how.light = LightKind.Point
        how.position = (C.c_float * 3)(float(light.x), float(light.y), float(light.z))
    elif isinstance(light, SpotLight):
        how.light = LightKind.Spot
        how.position = (C.c_float * 3)(*[float(v) for v in light.position])
        how.points_at = (C.c_float * 3)(*[float(v) for v in light.points_at])
        how.spot_exponent, how.cone_angle = float(light.exponent), float(light.cone_angle)
    else:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"a light is a DistantLight, a PointLight or a SpotLight, not {type(light).__name__}")
    return how


def lighting_texels(pixels, light, op=LightingOp.Diffuse, surface_scale=1.0, constant=1.0, specular_exponent=1.0, color=(1.0, 1.0, 1.0), edge=BlurEdge.Pad):
    """crh_lighting_texels (host only): the rule of Image.lighting on a (height, width, 4) uint8 array -> a (height, width, 4) uint8 array
    (include/contrast_hip.h crh_image_lighting states the rule)."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 4:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"lighting_texels takes a (height, width, 4) uint8 array, not {pixels.shape} {pixels.dtype}")
    how = _lighting_arguments(light, op, surface_scale, constant, specular_exponent, color, edge)
    out = np.empty_like(pixels)
    check(_ffi.load_library().crh_lighting_texels(pixels.shape[1], pixels.shape[0], pixels.ctypes.data, C.byref(how), out.ctypes.data))
    return out


class TurbulenceKind(IntEnum):  # crh_turbulence_kind
    FractalNoise = 0
    Turbulence = 1


MAX_TURBULENCE_OCTAVES = 12  # CRH_MAX_TURBULENCE_OCTAVES


def _turbulence_arguments(base_frequency, octaves, seed, kind, stitch, opaque, offset):
    """-> TurbulenceC; a scalar base_frequency serves both axes"""
    fx, fy = (base_frequency, base_frequency) if np.isscalar(base_frequency) else base_frequency
    how = _ffi.TurbulenceC()
    how.kind, how.octaves, how.seed, how.stitch, how.opaque = int(kind), int(octaves), int(seed), int(bool(stitch)), int(bool(opaque))
    how.base_frequency = (C.c_float * 2)(float(fx), float(fy))
    how.offset = (C.c_float * 2)(float(offset[0]), float(offset[1]))
    return how


def turbulence_texels(width, height, base_frequency, octaves=1, seed=0, kind=TurbulenceKind.Turbulence, stitch=False, opaque=False, offset=(0, 0)):
    """crh_turbulence_texels (host only): the rule of Image.turbulence -> a (height, width, 4) uint8 array (include/contrast_hip.h
    crh_image_turbulence states the rule)."""
    how = _turbulence_arguments(base_frequency, octaves, seed, kind, stitch, opaque, offset)
    width, height = int(width), int(height)
    if not (0 < width <= 16384 and 0 < height <= 16384):
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"turbulence_texels takes a width and a height in [1, 16384], not {width} x {height}")
    out = np.empty((height, width, 4), dtype=np.uint8)
    check(_ffi.load_library().crh_turbulence_texels(width, height, C.byref(how), out.ctypes.data))
    return out


def turbulence_tables(seed):
    """crh_turbulence_tables (host only) -> (lattice, gradient): the permutation of 0..255 as 256 uint8 and the unit gradients as a
    (4, 256, 2) float64 array, gradient[channel, lattice value] = (x, y), that `seed` gives."""
    lattice, gradient = np.empty(256, dtype=np.uint8), np.empty((4, 256, 2), dtype=np.float64)
    check(_ffi.load_library().crh_turbulence_tables(int(seed), lattice.ctypes.data_as(C.POINTER(C.c_uint8)), gradient.ctypes.data_as(C.POINTER(C.c_double))))
    return lattice, gradient


class Channel(IntEnum):  # crh_channel: the channel of a displacement map that moves an axis
    R = 0
    G = 1
    B = 2
    A = 3


MAX_DISPLACE_SCALE = 1024.0  # CRH_MAX_DISPLACE_SCALE


def _displace_arguments(scale, x_channel, y_channel, filter, edge):
    """-> DisplaceC; a scalar scale serves both axes (SVG has one)"""
    sx, sy = (scale, scale) if np.isscalar(scale) else scale
    how = _ffi.DisplaceC()
    how.scale = (C.c_float * 2)(float(sx), float(sy))
    how.x_channel, how.y_channel, how.filter, how.edge = int(x_channel), int(y_channel), int(filter), int(edge)
    return how


def displace_texels(pixels, map, scale, x_channel=Channel.A, y_channel=Channel.A, filter=Filter.Linear, edge=BlurEdge.Transparent):
    """crh_displace_texels (host only): the rule of Image.displace on two (height, width, 4) uint8 arrays of one size, the source and the
    map -> a (height, width, 4) uint8 array (include/contrast_hip.h crh_image_displace states the rule)."""
    pixels, map = np.ascontiguousarray(pixels), np.ascontiguousarray(map)
    for a in (pixels, map):
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4:
            raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"displace_texels takes (height, width, 4) uint8 arrays, not {a.shape} {a.dtype}")
    if pixels.shape != map.shape:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"displace_texels takes a map of the source's size, not {map.shape} beside {pixels.shape}")
    how = _displace_arguments(scale, x_channel, y_channel, filter, edge)
    out = np.empty_like(pixels)
    check(_ffi.load_library().crh_displace_texels(pixels.shape[1], pixels.shape[0], pixels.ctypes.data, map.ctypes.data, C.byref(how), out.ctypes.data))
    return out


def displace_offset(scale, code_x, code_y, x_channel=Channel.A, y_channel=Channel.A, filter=Filter.Linear, edge=BlurEdge.Transparent):
    """crh_displace_offset (host only) -> (qx, qy): the offsets, in 1/256 texel, that the straight map codes `code_x` and `code_y` (each
    <= 255) give under `scale`."""
    how = _displace_arguments(scale, x_channel, y_channel, filter, edge)
    q = (C.c_int32 * 2)()
    check(_ffi.load_library().crh_displace_offset(C.byref(how), int(code_x), int(code_y), q))
    return int(q[0]), int(q[1])


class DistanceMode(IntEnum):  # crh_distance_mode: what the distance is measured to
    Outside = 0  # to the shape: 255 on it, falling to 0 at the spread (glow, outline, spread)
    Inside = 1   # to what is not the shape: 0 off it, rising into it (chisel, inner glow)


MAX_DISTANCE_SPREAD = 255  # CRH_MAX_DISTANCE_SPREAD


def _distance_arguments(spread, mode, channel, threshold, edge):
    """-> DistanceC"""
    how = _ffi.DistanceC()
    how.mode, how.channel, how.threshold, how.spread, how.edge = int(mode), int(channel), int(threshold), int(spread), int(edge)
    return how


def distance_code(spread, squared_distance, mode=DistanceMode.Outside):
    """crh_distance_code (host only) -> the result byte of one squared distance D2 between texel centres under `spread`: v = 255 - c
    (DistanceMode.Outside) or c (DistanceMode.Inside), c = min(255, floor(255 sqrt(D2) / spread + 1/2)) by the integer statement."""
    how = _distance_arguments(spread, mode, Channel.A, 128, BlurEdge.Transparent)
    code = C.c_uint32()
    check(_ffi.load_library().crh_distance_code(C.byref(how), int(squared_distance), C.byref(code)))
    return int(code.value)


def distance_size(width, height, spread, mode=DistanceMode.Outside, channel=Channel.A, threshold=128, edge=BlurEdge.Transparent):
    """crh_distance_size (host only) -> (width, height) of the result of Image.distance_field on a width x height image: grown by the
    spread on every side for DistanceMode.Outside under BlurEdge.Transparent, else the same. Raises ContrastError for what
    Image.distance_field refuses."""
    how = _distance_arguments(spread, mode, channel, threshold, edge)
    w, h = C.c_uint32(), C.c_uint32()
    check(_ffi.load_library().crh_distance_size(int(width), int(height), C.byref(how), C.byref(w), C.byref(h)))
    return int(w.value), int(h.value)


def distance_texels(pixels, spread, mode=DistanceMode.Outside, channel=Channel.A, threshold=128, edge=BlurEdge.Transparent):
    """crh_distance_texels (host only): the rule of Image.distance_field on a (height, width, 4) uint8 array -> the (height', width', 4)
    uint8 result (include/contrast_hip.h crh_image_distance_field states the rule)."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 4:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"distance_texels takes a (height, width, 4) uint8 array, not {pixels.shape} {pixels.dtype}")
    w, h = distance_size(pixels.shape[1], pixels.shape[0], spread, mode, channel, threshold, edge)
    how = _distance_arguments(spread, mode, channel, threshold, edge)
    out = np.empty((h, w, 4), dtype=np.uint8)
    check(_ffi.load_library().crh_distance_texels(pixels.shape[1], pixels.shape[0], pixels.ctypes.data, C.byref(how), out.ctypes.data))
    return out


class ResizeFilter(IntEnum):  # crh_resize_filter: the reconstruction filter of Image.resize, widened by the ratio when minifying
    Box = 0         # support 0.5: nearest when magnifying, the exact area mean at integer ratios
    Triangle = 1    # support 1: bilinear when magnifying
    CatmullRom = 2  # support 2: the interpolating cubic (B = 0, C = 1/2)
    Mitchell = 3    # support 2: Mitchell-Netravali B = C = 1/3; softer, not interpolating
    Lanczos3 = 4    # support 3: the sharpest, with ringing at hard edges


MAX_RESIZE_TAPS = 512  # CRH_MAX_RESIZE_TAPS


def resize_taps(n, m, filter=ResizeFilter.Lanczos3):
    """crh_resize_taps (host only) -> (first, count, taps) of one axis of Image.resize from n source texels to m: output o reads the source
    indices first[o] .. first[o] + count[o] - 1 with the signed integer taps that follow each other in `taps` (int32, uint16 and int16
    arrays); an output's taps sum to exactly 16384 (include/contrast_hip.h crh_image_resize states the rule). Raises ContrastError for
    what Image.resize refuses of an axis."""
    lib = _ffi.load_library()
    total = C.c_uint64()
    check(lib.crh_resize_taps(int(n), int(m), int(filter), None, None, None, 0, C.byref(total)))
    first, count, taps = np.zeros(int(m), dtype=np.int32), np.zeros(int(m), dtype=np.uint16), np.zeros(int(total.value), dtype=np.int16)
    check(lib.crh_resize_taps(int(n), int(m), int(filter), first.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_uint16)),
                              taps.ctypes.data_as(C.POINTER(C.c_int16)), len(taps), None))
    return first, count, taps


def resize_texels(pixels, width, height, filter=ResizeFilter.Lanczos3):
    """crh_resize_texels (host only): the rule of Image.resize on a (height', width', 4) uint8 array -> the (height, width, 4) uint8 result."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 4:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"resize_texels takes a (height, width, 4) uint8 array, not {pixels.shape} {pixels.dtype}")
    width, height = int(width), int(height)
    legal = 1 <= width <= 16384 and 1 <= height <= 16384  # (a size the library refuses gets a texel's room and the library's status)
    out = np.empty((height, width, 4) if legal else (1, 1, 4), dtype=np.uint8)
    check(_ffi.load_library().crh_resize_texels(pixels.shape[1], pixels.shape[0], pixels.ctypes.data, width & 0xFFFFFFFF, height & 0xFFFFFFFF, int(filter), out.ctypes.data))
    return out


@dataclass(frozen=True, eq=False)
class ImageStatistics:
    """crh_image_stats: `histogram` is a (4, 256) uint32 array, [r, g, b, a][code] = how many texels store that code in that channel,
    over all texels; `bounds` = (x0, y0, x1, y1), half-open, the smallest rectangle that holds every texel inside (stored code of the
    chosen channel >= the threshold), (0, 0, 0, 0) if none is; `count` = the texels inside."""
    histogram: np.ndarray
    bounds: tuple
    count: int


def _statistics_of(stats):
    """ImageStatsC -> ImageStatistics"""
    return ImageStatistics(np.ctypeslib.as_array(stats.histogram).astype(np.uint32).reshape(4, 256), (int(stats.x0), int(stats.y0), int(stats.x1), int(stats.y1)), int(stats.count))


def _int32(v):
    """an offset as the C ABI takes it; what does not fit an int32 is refused here, where ctypes would wrap it"""
    v = int(v)
    if not -2 ** 31 <= v < 2 ** 31:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"an offset is an int32, not {v}")
    return v


def crop_texels(pixels, x, y, width, height):
    """crh_crop_texels (host only): the rule of Image.crop on a (height', width', 4) uint8 array -> the (height, width, 4) uint8 result,
    texel (i, j) = the source's (x + i, y + j), zeros outside the source."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 4:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"crop_texels takes a (height, width, 4) uint8 array, not {pixels.shape} {pixels.dtype}")
    width, height = int(width), int(height)
    legal = 1 <= width <= 16384 and 1 <= height <= 16384  # (a size the library refuses gets a texel's room and the library's status)
    out = np.empty((height, width, 4) if legal else (1, 1, 4), dtype=np.uint8)
    check(_ffi.load_library().crh_crop_texels(pixels.shape[1], pixels.shape[0], pixels.ctypes.data, _int32(x), _int32(y), width & 0xFFFFFFFF, height & 0xFFFFFFFF, out.ctypes.data))
    return out


def statistics_texels(pixels, channel=Channel.A, threshold=1):
    """crh_statistics_texels (host only): the rule of Image.statistics on a (height, width, 4) uint8 array -> ImageStatistics."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 4:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"statistics_texels takes a (height, width, 4) uint8 array, not {pixels.shape} {pixels.dtype}")
    stats = _ffi.ImageStatsC()
    check(_ffi.load_library().crh_statistics_texels(pixels.shape[1], pixels.shape[0], pixels.ctypes.data, int(channel) & 0xFFFFFFFF, int(threshold) & 0xFFFFFFFF, C.byref(stats)))
    return _statistics_of(stats)


def _variable_blur_arguments(sigma, sigma_at_zero, channel, edge):
    """-> VariableBlurC; a scalar sigma serves both axes, as blur() takes sigma_y=None; a pair is (x, y)"""
    x1, y1 = (sigma, sigma) if np.isscalar(sigma) else sigma
    x0, y0 = (sigma_at_zero, sigma_at_zero) if np.isscalar(sigma_at_zero) else sigma_at_zero
    how = _ffi.VariableBlurC()
    how.sigma_x = (C.c_float * 2)(float(x0), float(x1))
    how.sigma_y = (C.c_float * 2)(float(y0), float(y1))
    how.channel, how.edge = int(channel) & 0xFFFFFFFF, int(edge) & 0xFFFFFFFF
    return how


def variable_blur_texels(pixels, mask, sigma, sigma_at_zero=0.0, channel=Channel.A, edge=BlurEdge.Pad):
    """crh_variable_blur_texels (host only): the rule of Image.variable_blur on two (height, width, 4) uint8 arrays of one size, the
    source and the mask -> a (height, width, 4) uint8 array (include/contrast_hip.h crh_image_variable_blur states the rule)."""
    pixels, mask = np.ascontiguousarray(pixels), np.ascontiguousarray(mask)
    for a in (pixels, mask):
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4:
            raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"variable_blur_texels takes (height, width, 4) uint8 arrays, not {a.shape} {a.dtype}")
    if pixels.shape != mask.shape:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"variable_blur_texels takes a mask of the source's size, not {mask.shape} beside {pixels.shape}")
    how = _variable_blur_arguments(sigma, sigma_at_zero, channel, edge)
    out = np.empty_like(pixels)
    check(_ffi.load_library().crh_variable_blur_texels(pixels.shape[1], pixels.shape[0], pixels.ctypes.data, mask.ctypes.data, C.byref(how), out.ctypes.data))
    return out


def variable_blur_sigma(code, sigma, sigma_at_zero=0.0):
    """crh_variable_blur_sigma (host only) -> (sigma_x, sigma_y): the sigmas, as float32 values, of the mask code `code` (<= 255) between
    `sigma_at_zero` at code 0 and `sigma` at code 255, each a scalar or an (x, y) pair."""
    how = _variable_blur_arguments(sigma, sigma_at_zero, Channel.A, BlurEdge.Pad)
    sx, sy = C.c_float(), C.c_float()
    check(_ffi.load_library().crh_variable_blur_sigma(C.byref(how), int(code) & 0xFFFFFFFF, C.byref(sx), C.byref(sy)))
    return float(sx.value), float(sy.value)


class TransformFilter(IntEnum):  # crh_transform_filter
    Nearest = 0
    Linear = 1
    Cubic = 2  # Catmull-Rom over 4 x 4 texels


MAX_TRANSFORM_ENTRY = 2.0 ** 40  # CRH_MAX_TRANSFORM_ENTRY


def _matrix9(matrix):
    """9 floats, row-major, or 6 (an affine matrix: the last row is 0 0 1) -> a C array of 9 doubles"""
    m = [float(v) for v in np.asarray(matrix, dtype=np.float64).reshape(-1)]
    if len(m) == 6:
        m += [0.0, 0.0, 1.0]
    if len(m) != 9:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"a transform matrix has 9 entries (or 6, affine), not {len(m)}")
    return (C.c_double * 9)(*m)


def _transform_arguments(matrix, width, height, filter, edge):
    """-> TransformC"""
    how = _ffi.TransformC()
    how.matrix = _matrix9(matrix)
    how.width, how.height, how.filter, how.edge = int(width) & 0xFFFFFFFF, int(height) & 0xFFFFFFFF, int(filter) & 0xFFFFFFFF, int(edge) & 0xFFFFFFFF
    return how


def transform_fit(width, height, forward, filter=TransformFilter.Linear, edge=BlurEdge.Transparent):
    """crh_transform_fit (host only) -> (matrix, (result width, result height), origin): for a source of width x height and `forward`,
    which maps SOURCE coordinates to the caller's target space (9 floats row-major, or 6 for an affine matrix), the result -> source
    matrix as a (3, 3) float64 array and the size of the smallest result that holds the whole source, and where the target space's
    (0, 0) lies in that result."""
    how, origin = _ffi.TransformC(), (C.c_int32 * 2)()
    check(_ffi.load_library().crh_transform_fit(int(width) & 0xFFFFFFFF, int(height) & 0xFFFFFFFF, _matrix9(forward), int(filter) & 0xFFFFFFFF, int(edge) & 0xFFFFFFFF, C.byref(how), origin))
    return np.array(list(how.matrix), dtype=np.float64).reshape(3, 3), (int(how.width), int(how.height)), (int(origin[0]), int(origin[1]))


def transform_position(matrix, width, height, i, j):
    """crh_transform_position (host only) -> (X, Y, visible): where result texel (i, j) of a width x height result reads the source under
    `matrix` (result -> source), in 1/256 texel, and whether the texel is visible (not behind the horizon of a projective matrix)."""
    how = _transform_arguments(matrix, width, height, TransformFilter.Nearest, BlurEdge.Transparent)
    position, visible = (C.c_int32 * 2)(), C.c_uint32()
    check(_ffi.load_library().crh_transform_position(C.byref(how), int(i) & 0xFFFFFFFF, int(j) & 0xFFFFFFFF, position, C.byref(visible)))
    return int(position[0]), int(position[1]), bool(visible.value)


def transform_texels(pixels, matrix, width, height, filter=TransformFilter.Linear, edge=BlurEdge.Transparent):
    """crh_transform_texels (host only): the rule of Image.resample on a (height', width', 4) uint8 array -> the (height, width, 4) uint8
    result (include/contrast_hip.h crh_image_transform states the rule)."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 4:
        raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"transform_texels takes a (height, width, 4) uint8 array, not {pixels.shape} {pixels.dtype}")
    how = _transform_arguments(matrix, width, height, filter, edge)
    legal = 1 <= how.width <= 16384 and 1 <= how.height <= 16384  # (a size the library refuses gets a texel's room and the library's status)
    out = np.empty((how.height, how.width, 4) if legal else (1, 1, 4), dtype=np.uint8)
    check(_ffi.load_library().crh_transform_texels(pixels.shape[1], pixels.shape[0], pixels.ctypes.data, C.byref(how), out.ctypes.data))
    return out


class Image:
    """crh_image: width x height texels of premultiplied RGBA8 on the device, row 0 = top — the bytes Frame.download() hands out. `pixels` is a
    [height, width, 4] uint8 array, copied before the constructor returns. One level until generate_mipmaps(): an image drawn much smaller than
    its texels aliases unless it has mipmaps and its paint's filter is Filter.NearestMipmap or Filter.LinearMipmap. `origin` = the texel of this
    image that lies over texel (0, 0) of the image it was made from: (0, 0) unless blur(), morphology() or distance_field() grew it, or
    crop(), trim() or from_frame(region=...) cut it: a crop at (x, y) moves the origin by (-x, -y), so it can be negative."""

    origin = (0, 0)

    def __init__(self, renderer: Renderer, pixels):
        pixels = np.asarray(pixels)
        if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 4:
            raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, f"an image takes a (height, width, 4) uint8 array, not {pixels.shape} {pixels.dtype}")
        data = np.ascontiguousarray(pixels)
        self.renderer, self.lib = renderer, renderer.lib
        handle = C.c_void_p()
        check(self.lib.crh_image_create(renderer.handle, data.shape[1], data.shape[0], data.ctypes.data, C.byref(handle)))
        self.handle = handle
        self.width, self.height = int(data.shape[1]), int(data.shape[0])

    @classmethod
    def _adopt(cls, renderer, handle, size=None):
        """A new Image around a handle the library has just returned; `size` = (width, height) where the caller knows it, crh_image_size otherwise."""
        image = cls.__new__(cls)
        image.renderer, image.lib, image.handle = renderer, renderer.lib, handle
        if size is None:
            w, h = C.c_uint32(), C.c_uint32()
            check(image.lib.crh_image_size(handle, C.byref(w), C.byref(h)))
            size = (w.value, h.value)
        image.width, image.height = int(size[0]), int(size[1])
        return image

    @staticmethod
    def from_frame(frame: Frame, region=None):
        """crh_image_create_from_frame: a snapshot of what the frame shows (an RGBA8 or RGBA8-attachment frame, not restricted by
        set_tile_rows), copied on the device; later passes into the frame do not change it. region = (x, y, width, height) is
        crh_image_create_from_frame_region: byte for byte from_frame(frame).crop(x, y, width, height), origin (-x, -y), without the
        full-size copy; the rectangle may leave the frame (zeros there) and only its own size is limited to 16384."""
        handle = C.c_void_p()
        if region is None:
            check(frame.lib.crh_image_create_from_frame(frame.handle, C.byref(handle)))
            return Image._adopt(frame.renderer, handle)
        x, y, width, height = (int(v) for v in region)
        check(frame.lib.crh_image_create_from_frame_region(frame.handle, _int32(x), _int32(y), width & 0xFFFFFFFF, height & 0xFFFFFFFF, C.byref(handle)))
        image = Image._adopt(frame.renderer, handle, (width, height))
        image.origin = (-x, -y)
        return image

    @classmethod
    def turbulence(cls, renderer: Renderer, width, height, base_frequency, octaves=1, seed=0, kind=TurbulenceKind.Turbulence, stitch=False, opaque=False, offset=(0, 0)):
        """crh_image_turbulence -> a new Image of one level, width x height, origin (0, 0): procedural noise made on the device (SVG
        feTurbulence), complete when this returns (a synchronous call). `base_frequency` = lattice cells per texel, a scalar or (x, y), each
        in [0, 4]; `octaves` in [0, MAX_TURBULENCE_OCTAVES], each of twice the frequency and half the weight; TurbulenceKind.FractalNoise is
        signed noise around the middle grey, TurbulenceKind.Turbulence the sum of absolute values; `stitch` makes the image tile with
        itself; `opaque` gives alpha 255 and three channels of noise instead of SVG's four; `offset` = the noise-space position of texel
        (0, 0), so a large texture can be made in pieces. Binary64 arithmetic in a fixed order, so every byte is defined."""
        how = _turbulence_arguments(base_frequency, octaves, seed, kind, stitch, opaque, offset)
        handle = C.c_void_p()
        check(renderer.lib.crh_image_turbulence(renderer.handle, int(width), int(height), C.byref(how), C.byref(handle)))
        return cls._adopt(renderer, handle, (width, height))

    def generate_mipmaps(self):
        """crh_image_generate_mipmaps: the levels below the image, each the rounded 2 x 2 mean of the one above, built on the device; complete
        when this returns. A second call changes nothing. A paint table set before the call keeps drawing the one level."""
        check(self.lib.crh_image_generate_mipmaps(self.handle))

    @property
    def levels(self):
        """crh_image_level_count: 1 until generate_mipmaps(), then floor(log2(max(width, height))) + 1."""
        n = C.c_uint32()
        check(self.lib.crh_image_level_count(self.handle, C.byref(n)))
        return int(n.value)

    def download_level(self, level):
        """crh_image_download_level -> the [height, width, 4] uint8 texels of level `level` (0 = the image itself)."""
        w, h = C.c_uint32(), C.c_uint32()
        check(self.lib.crh_image_download_level(self.handle, int(level), None, C.byref(w), C.byref(h)))
        out = np.empty((int(h.value), int(w.value), 4), dtype=np.uint8)
        check(self.lib.crh_image_download_level(self.handle, int(level), out.ctypes.data, C.byref(w), C.byref(h)))
        return out

    def blur(self, sigma_x, sigma_y=None, edge=BlurEdge.Transparent):
        """crh_image_blur -> a new Image of one level: the separable Gaussian of this image's level 0, integer and bit-exact, built on the
        device and complete when this returns (a synchronous call: one wait per blur). sigma_y=None means sigma_x; both in [0,
        MAX_BLUR_SIGMA]. BlurEdge.Transparent grows the result by the radius ceil(3 sigma) on every side, and the result's `origin` is
        (Rx, Ry); the other edges keep the size. This image is not modified."""
        sigma_x = float(sigma_x)
        sigma_y = sigma_x if sigma_y is None else float(sigma_y)
        handle = C.c_void_p()
        check(self.lib.crh_image_blur(self.handle, sigma_x, sigma_y, int(edge), C.byref(handle)))
        image = Image._adopt(self.renderer, handle)
        if int(edge) == BlurEdge.Transparent:
            image.origin = ((image.width - self.width) // 2, (image.height - self.height) // 2)
        return image

    def composite(self, source, op=CompositeOp.SrcOver, mode=BlendMode.Normal, opacity=1.0, offset=(0, 0)):
        """crh_image_composite, called on the backdrop -> a new Image of one level and of this image's size, origin (0, 0): `source` combined
        with this image texel by texel by a Porter-Duff operator, a blend mode and a group opacity in [0, 1], integer and bit-exact, built on
        the device and complete when this returns. Source texel (0, 0) lies over this image's texel `offset`, any integers; outside the
        source the source is transparent. To place a BlurEdge.Transparent result, which grew by its `origin`, so that the image it was
        blurred from would lie at (dx, dy): offset = (dx - source.origin[0], dy - source.origin[1]). Neither image is modified; `source` may
        be this image."""
        how = _ffi.CompositeC(int(op), int(mode), float(opacity), int(offset[0]), int(offset[1]))
        handle = C.c_void_p()
        check(self.lib.crh_image_composite(self.handle, source.handle, C.byref(how), C.byref(handle)))
        return Image._adopt(self.renderer, handle, (self.width, self.height))

    def color_filter(self, matrix=None, tables=None):
        """crh_image_color_filter -> a new Image of one level, of this image's size and origin: every texel unpremultiplied, through the
        4 x 5 `matrix` (20 floats, row-major, |m| <= COLOR_MATRIX_MAX; ColorMatrix builds the usual ones; None = the identity), then through
        `tables` (1024 uint8: r, g, b, a, 256 entries each; None = the identity), and premultiplied again — integer and bit-exact, built on
        the device and complete when this returns. A blurred snapshot through ColorMatrix.flood(r, g, b, a) is a drop shadow in that colour.
        This image is not modified."""
        m, t = _color_filter_arguments(matrix, tables)
        handle = C.c_void_p()
        check(self.lib.crh_image_color_filter(self.handle, m, None if t is None else t.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(handle)))
        image = Image._adopt(self.renderer, handle, (self.width, self.height))
        image.origin = self.origin
        return image

    def morphology(self, op, radius_x, radius_y=None, edge=BlurEdge.Transparent):
        """crh_image_morphology -> a new Image of one level: per channel the min (MorphologyOp.Erode) or max (MorphologyOp.Dilate) of this
        image's level 0 over the rectangle |dx| <= radius_x, |dy| <= radius_y, exact, built on the device and complete when this returns (a
        synchronous call). radius_y=None means radius_x; both integers in [0, MAX_MORPHOLOGY_RADIUS]. Dilate under BlurEdge.Transparent grows
        the result by the radius on every side, and the result's `origin` is (radius_x, radius_y), by blur()'s convention; everything else
        keeps the size and origin (0, 0). This image is not modified."""
        radius_x = int(radius_x)
        radius_y = radius_x if radius_y is None else int(radius_y)
        handle = C.c_void_p()
        check(self.lib.crh_image_morphology(self.handle, int(op), radius_x, radius_y, int(edge), C.byref(handle)))
        image = Image._adopt(self.renderer, handle)
        if int(op) == MorphologyOp.Dilate and int(edge) == BlurEdge.Transparent:
            image.origin = (radius_x, radius_y)
        return image

    def dilate(self, radius_x, radius_y=None, edge=BlurEdge.Transparent):
        """morphology(MorphologyOp.Dilate, ...): an outline's or a spread's growth."""
        return self.morphology(MorphologyOp.Dilate, radius_x, radius_y, edge)

    def erode(self, radius_x, radius_y=None, edge=BlurEdge.Transparent):
        """morphology(MorphologyOp.Erode, ...): a choke, a negative spread."""
        return self.morphology(MorphologyOp.Erode, radius_x, radius_y, edge)

    def convolve(self, kernel, divisor=None, bias=0.0, target=None, edge=BlurEdge.Pad, preserve_alpha=False):
        """crh_image_convolve -> a new Image of one level, of this image's size and origin: this image's level 0 through the kernel matrix
        `kernel` (a 2-D array of up to 15 x 15 entries, in SVG's orientation; ConvolveKernel has presets), integer and bit-exact, built on
        the device and complete when this returns (a synchronous call). divisor=None means the sum of the entries, or 1 if that is 0;
        target=None means (order_x // 2, order_y // 2); |bias| <= 1 is added in units of the full range. preserve_alpha=True keeps every
        texel's alpha and convolves the unpremultiplied colours. The result has this image's size under every edge. This image is not modified."""
        how, values = _convolve_arguments(kernel, divisor, bias, target, edge, preserve_alpha)
        handle = C.c_void_p()
        check(self.lib.crh_image_convolve(self.handle, C.byref(how), C.byref(handle)))
        image = Image._adopt(self.renderer, handle, (self.width, self.height))
        image.origin = self.origin
        return image

    def lighting(self, light, op=LightingOp.Diffuse, surface_scale=1.0, constant=1.0, specular_exponent=1.0, color=(1.0, 1.0, 1.0), edge=BlurEdge.Pad):
        """crh_image_lighting -> a new Image of one level, of this image's size and origin: this image's alpha as a height field (alpha 255 =
        `surface_scale` texels high) lit by `light` (a DistantLight, a PointLight or a SpotLight) of colour `color`, built on the device and
        complete when this returns (a synchronous call). LightingOp.Diffuse gives opaque texels constant * N.L * colour (MULTIPLY them onto
        a layer); LightingOp.Specular gives premultiplied highlights constant * (N.H) ** specular_exponent * colour (PLUS them onto a
        layer). Binary64 arithmetic in a fixed order, so every byte is defined. This image is not modified; its colours are not read."""
        how = _lighting_arguments(light, op, surface_scale, constant, specular_exponent, color, edge)
        handle = C.c_void_p()
        check(self.lib.crh_image_lighting(self.handle, C.byref(how), C.byref(handle)))
        image = Image._adopt(self.renderer, handle, (self.width, self.height))
        image.origin = self.origin
        return image

    def diffuse_lighting(self, light, surface_scale=1.0, constant=1.0, color=(1.0, 1.0, 1.0), edge=BlurEdge.Pad):
        """lighting(light, LightingOp.Diffuse, ...): SVG feDiffuseLighting."""
        return self.lighting(light, LightingOp.Diffuse, surface_scale, constant, 1.0, color, edge)

    def specular_lighting(self, light, surface_scale=1.0, constant=1.0, specular_exponent=1.0, color=(1.0, 1.0, 1.0), edge=BlurEdge.Pad):
        """lighting(light, LightingOp.Specular, ...): SVG feSpecularLighting."""
        return self.lighting(light, LightingOp.Specular, surface_scale, constant, specular_exponent, color, edge)

    def displace(self, map, scale, x_channel=Channel.A, y_channel=Channel.A, filter=Filter.Linear, edge=BlurEdge.Transparent):
        """crh_image_displace -> a new Image of one level, of this image's size, origin (0, 0): this image read through the per-texel offsets
        of `map`, an Image of the same size and renderer (SVG feDisplacementMap; Image.turbulence makes the usual map), integer and
        bit-exact, built on the device and complete when this returns (a synchronous call). A map texel moves its texel by
        scale * (u / 255 - 1/2) texels on each axis, u = the straight code of `x_channel` / `y_channel`; a scalar `scale` serves both
        axes, each |.| <= MAX_DISPLACE_SCALE. `filter` is Filter.Nearest or Filter.Linear, `edge` what THIS image is outside itself.
        The defaults are SVG's. Neither image is modified; the map may be this image."""
        how = _displace_arguments(scale, x_channel, y_channel, filter, edge)
        handle = C.c_void_p()
        check(self.lib.crh_image_displace(self.handle, map.handle, C.byref(how), C.byref(handle)))
        return Image._adopt(self.renderer, handle, (self.width, self.height))

    def variable_blur(self, mask, sigma, sigma_at_zero=0.0, channel=Channel.A, edge=BlurEdge.Pad):
        """crh_image_variable_blur -> a new Image of one level, of this image's size under every edge, origin (0, 0): blur() with a
        strength that changes across the image. `mask` is an Image of the same size and renderer; the stored code u of its `channel`
        at a texel chooses that texel's own Gaussian: `sigma_at_zero` at u = 0, `sigma` at u = 255, linear in u between (either may be
        the larger), each a scalar or an (x, y) pair in [0, MAX_BLUR_SIGMA]; the taps of a level are blur()'s. Integer and bit-exact,
        built on the device and complete when this returns (a synchronous call). A mask of one value gives blur()'s bytes; a texel
        whose level has sigma 0 comes back exactly. `edge` is what THIS image is outside itself; the default is BlurEdge.Pad because
        the call keeps the size and a backdrop should not darken at its rim. A progressive backdrop blur: a mask whose alpha ramps
        from 0 to 255 down the panel, variable_blur(ramp, 24). Neither image is modified; the mask may be this image."""
        how = _variable_blur_arguments(sigma, sigma_at_zero, channel, edge)
        handle = C.c_void_p()
        check(self.lib.crh_image_variable_blur(self.handle, mask.handle, C.byref(how), C.byref(handle)))
        return Image._adopt(self.renderer, handle, (self.width, self.height))

    def resample(self, matrix, width, height, filter=TransformFilter.Linear, edge=BlurEdge.Transparent):
        """crh_image_transform, the raw call -> a new Image of one level, width x height (each in [1, 16384]), origin (0, 0): this image
        seen through `matrix`, which maps RESULT coordinates (x, y, 1) to coordinates of THIS image (9 floats row-major, or 6 for an
        affine matrix; finite, |.| <= MAX_TRANSFORM_ENTRY; a singular one is legal). Positions in binary64 in a fixed order, then
        integers: every byte is defined (include/contrast_hip.h states the rule). TransformFilter.Nearest and .Linear sample as
        displace() does, .Cubic is Catmull-Rom over 4 x 4 texels; `edge` is what THIS image is outside itself; a texel behind the
        horizon of a projective matrix is transparent. No prefilter: shrink by more than about 2 with resize() first. Built on the device
        and complete when this returns (a synchronous call). This image is not modified."""
        how = _transform_arguments(matrix, width, height, filter, edge)
        handle = C.c_void_p()
        check(self.lib.crh_image_transform(self.handle, C.byref(how), C.byref(handle)))
        return Image._adopt(self.renderer, handle, (int(how.width), int(how.height)))

    def transform(self, forward, filter=TransformFilter.Linear, edge=BlurEdge.Transparent):
        """transform_fit, then resample: this image moved by `forward`, which maps its coordinates to the caller's target space (9 floats
        row-major, or 6 for an affine matrix), in the smallest result that holds all of it. The result's `origin` is where the target
        space's (0, 0) lies in it, by blur()'s and crop()'s convention: composite it at offset = (dx - origin[0], dy - origin[1]) to put
        target point (0, 0) at (dx, dy). A corner behind the horizon, a singular `forward` and a result above 16384 are refused."""
        matrix, (width, height), origin = transform_fit(self.width, self.height, forward, filter, edge)
        image = self.resample(matrix, width, height, filter, edge)
        image.origin = origin
        return image

    def rotate(self, degrees, center=None, filter=TransformFilter.Linear, edge=BlurEdge.Transparent):
        """transform() by a rotation of `degrees`, clockwise on the screen (y points down, as CSS rotate() turns), about `center` (x, y) in
        this image's coordinates, None = its middle. A multiple of 90 uses the entries 0 and +-1 exactly, so a quarter turn permutes the
        texels. The result's `origin` is where this image's texel corner (0, 0) would lie had it not been turned."""
        cx, cy = (self.width / 2.0, self.height / 2.0) if center is None else (float(center[0]), float(center[1]))
        quarter = float(degrees) / 90.0
        if quarter == int(quarter):
            c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(quarter) % 4]
        else:
            c, s = math.cos(math.radians(float(degrees))), math.sin(math.radians(float(degrees)))
        return self.transform((c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy), filter, edge)

    def distance_field(self, spread, mode=DistanceMode.Outside, channel=Channel.A, threshold=128, edge=BlurEdge.Transparent):
        """crh_image_distance_field -> a new Image of one level: for every texel the exact Euclidean distance between texel centres to the
        shape {stored code of `channel` >= `threshold`} (DistanceMode.Outside: 255 on the shape, falling to 0 at `spread` texels) or to
        what is not the shape (DistanceMode.Inside: 0 off the shape, rising into it), one rounding by an integer statement, on all four
        channels; built on the device and complete when this returns (a synchronous call). `spread` is an integer in
        [1, MAX_DISTANCE_SPREAD]. Outside under BlurEdge.Transparent grows the result by the spread on every side, and the result's
        `origin` is (spread, spread), by blur()'s convention; everything else keeps the size and origin (0, 0). A round outline of 8
        texels: distance_field(8), a table through color_filter, composite DstOver at the grown origin. This image is not modified."""
        how = _distance_arguments(spread, mode, channel, threshold, edge)
        handle = C.c_void_p()
        check(self.lib.crh_image_distance_field(self.handle, C.byref(how), C.byref(handle)))
        image = Image._adopt(self.renderer, handle)
        if int(mode) == DistanceMode.Outside and int(edge) == BlurEdge.Transparent:
            image.origin = (int(spread), int(spread))
        return image

    def resize(self, width, height, filter=ResizeFilter.Lanczos3):
        """crh_image_resize -> a new Image of one level, width x height, that holds the whole of this image resampled with `filter`, widened
        by the ratio on an axis that shrinks, so nothing aliases; integer taps per output texel, bit-exact (include/contrast_hip.h
        crh_image_resize states the rule); built on the device and complete when this returns (a synchronous call). Both sides lie in
        [1, 16384]; an axis that shrinks by more than its filter's cap (about 85 under Lanczos3, 500 under Box) is refused: chain two
        calls. The result's origin is (0, 0) whatever this image's is. This image is not modified."""
        handle = C.c_void_p()
        check(self.lib.crh_image_resize(self.handle, int(width) & 0xFFFFFFFF, int(height) & 0xFFFFFFFF, int(filter) & 0xFFFFFFFF, C.byref(handle)))
        return Image._adopt(self.renderer, handle, (int(width), int(height)))

    def crop(self, x, y, width, height):
        """crh_image_crop -> a new Image of one level, width x height (each in [1, 16384]): texel (i, j) is this image's texel
        (x + i, y + j), the bytes as stored, and (0, 0, 0, 0) outside this image; built on the device and complete when this returns (a
        synchronous call). x and y are any int32: a rectangle that misses this image gives a transparent canvas, a larger one the
        transparent backdrop around it. The result's `origin` is (origin[0] - x, origin[1] - y), which can be negative. This image is
        not modified."""
        x, y, width, height = _int32(x), _int32(y), int(width), int(height)
        handle = C.c_void_p()
        check(self.lib.crh_image_crop(self.handle, x, y, width & 0xFFFFFFFF, height & 0xFFFFFFFF, C.byref(handle)))
        image = Image._adopt(self.renderer, handle, (width, height))
        image.origin = (self.origin[0] - x, self.origin[1] - y)
        return image

    def statistics(self, channel=Channel.A, threshold=1):
        """crh_image_statistics -> ImageStatistics: the per-channel histograms of the stored codes over all texels, and the bounds and
        the number of the texels inside — stored code of `channel` >= `threshold` (1..255), distance_field()'s definition. Reduced on
        the device; 4116 bytes come back (a synchronous call). Tables for color_filter (auto-levels, a percentile stretch), "is this
        layer empty" and the covered area all come from it. This image is not modified."""
        stats = _ffi.ImageStatsC()
        check(self.lib.crh_image_statistics(self.handle, int(channel) & 0xFFFFFFFF, int(threshold) & 0xFFFFFFFF, C.byref(stats)))
        return _statistics_of(stats)

    def bounds(self, channel=Channel.A, threshold=1):
        """statistics(channel, threshold).bounds: (x0, y0, x1, y1), half-open, (0, 0, 0, 0) if no texel is inside."""
        return self.statistics(channel, threshold).bounds

    def trim(self, channel=Channel.A, threshold=1, margin=0):
        """statistics(), then crop() to the bounds grown by `margin` texels on every side and clipped to this image: the layer without
        its empty surroundings, with the `origin` that puts it back (by composite()'s rule: offset = (dx - origin[0], dy - origin[1])
        of the result). An image with nothing inside trims to the 1 x 1 crop at (0, 0)."""
        x0, y0, x1, y1 = self.bounds(channel, threshold)
        if x1 == x0:
            return self.crop(0, 0, 1, 1)
        margin = int(margin)
        x0, y0, x1, y1 = max(0, x0 - margin), max(0, y0 - margin), min(self.width, x1 + margin), min(self.height, y1 + margin)
        return self.crop(x0, y0, x1 - x0, y1 - y0)

    def destroy(self):
        """crh_image_destroy. Legal while a Scene's paint table names the image: the table keeps the pixels until it is replaced."""
        if getattr(self, "handle", None):
            self.lib.crh_image_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.destroy()


@dataclass(frozen=True)
class ImagePaint:
    """crh_image_paint: the texels of an Image as the source of a Color cover, times the instance colour (include/contrast_hip.h
    crh_scene_set_paints_with_images states the model). `matrix` = (m0 .. m5) maps path coordinates to texels: u = m0 x + m1 y + m2,
    v = m3 x + m4 y + m5; texel (i, j) covers [i, i + 1) x [j, j + 1), row 0 is the image's top."""
    image: Image
    matrix: Tuple[float, float, float, float, float, float]
    filter: int = Filter.Linear
    spread_x: int = Spread.Pad
    spread_y: int = Spread.Pad

    def __post_init__(self):
        object.__setattr__(self, "matrix", tuple(float(v) for v in self.matrix))
        if len(self.matrix) != 6:
            raise ContrastError(_ffi.ERR_INVALID_ARGUMENT, "an image paint's matrix has six entries")

    @staticmethod
    def fit(image, lower, upper, filter=Filter.Linear, spread_x=Spread.Pad, spread_y=Spread.Pad):
        """The path rectangle [lower, upper] onto the whole image, upright under a transform that does not mirror: path y points up on the
        frame, so y = upper[1] is the image's row 0."""
        sx, sy = image.width / (float(upper[0]) - float(lower[0])), image.height / (float(upper[1]) - float(lower[1]))
        return ImagePaint(image, (sx, 0.0, -sx * float(lower[0]), 0.0, -sy, sy * float(upper[1])), filter, spread_x, spread_y)

    def to_c(self):
        c = _ffi.ImagePaintC()
        c.image = self.image.handle
        c.filter, c.spread_x, c.spread_y = int(self.filter), int(self.spread_x), int(self.spread_y)
        for i in range(6):
            c.m[i] = self.matrix[i]
        return c

    def validate(self):
        """crh_image_paint_validate (host only): raises ContrastError for what Scene.set_paints would refuse."""
        check(_ffi.load_library().crh_image_paint_validate(C.byref(self.to_c())))


def split_paints(paints, instance_paint):
    """A list of Paint and ImagePaint mixed -> (gradients, image paints, association): the C ABI numbers the gradients first and the image
    paints behind them, so the indices of the mixed list are remapped."""
    gradients = [p for p in paints if not isinstance(p, ImagePaint)]
    images = [p for p in paints if isinstance(p, ImagePaint)]
    place, g, m = [], 0, 0
    for p in paints:
        if isinstance(p, ImagePaint):
            place.append(len(gradients) + m)
            m += 1
        else:
            place.append(g)
            g += 1
    which = [int(k) for k in np.asarray(instance_paint, dtype=np.int64).ravel()]
    return gradients, images, [place[k] if 0 <= k < len(place) else k for k in which]


COMM_ID_BYTES = 128


def comm_unique_id(lib=None):
    """Rank 0: the 128-byte id (ncclGetUniqueId) every rank passes to Comm(...); distribute it by any means."""
    lib = lib or _ffi.load_library()
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    check(lib.crh_comm_unique_id(buf))
    return bytes(buf)


def shard_range(n_items, rank, world, lib=None):
    """crh_comm_shard: the contiguous Shape range of a rank (host arithmetic, no GPU)."""
    lib = lib or _ffi.load_library()
    b, e = C.c_uint32(), C.c_uint32()
    check(lib.crh_comm_shard(n_items, rank, world, C.byref(b), C.byref(e)))
    return b.value, e.value


def slab_rows(height, rank, world, lib=None):
    lib = lib or _ffi.load_library()
    b, e = C.c_uint32(), C.c_uint32()
    check(lib.crh_comm_slab_rows(height, rank, world, C.byref(b), C.byref(e)))
    return b.value, e.value


class Comm:
    """One rank of the framebuffer exchange (include/contrast_hip.h, crh_comm_*): RCCL when `unique_id` is given, otherwise a member of an
    in-process loopback group on one device (`rank0` = the group's founder for ranks > 0)."""

    def __init__(self, renderer: Renderer, rank: int, world: int, unique_id: bytes = None, rank0: "Comm" = None):
        self.renderer, self.lib, self.rank, self.world = renderer, renderer.lib, rank, world
        handle = C.c_void_p()
        if unique_id is not None:
            ident = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
            check(self.lib.crh_comm_create(renderer.handle, rank, world, ident, C.byref(handle)))
        else:
            check(self.lib.crh_comm_create_local(renderer.handle, rank, world, rank0.handle if rank0 else None, C.byref(handle)))
        self.handle = handle

    def exchange(self, layer: Frame, result: Frame = None):
        """Collective (RCCL): composites every rank's layer in rank order into rank 0's `result`."""
        check(self.lib.crh_frame_exchange(self.handle, layer.handle, result.handle if result is not None else None))

    def local_exchange(self, layers, result: Frame):
        """Loopback group, called on rank 0's communicator: layers[k] = rank k's frame."""
        arr = (C.c_void_p * len(layers))(*[f.handle for f in layers])
        check(self.lib.crh_comm_local_exchange(self.handle, arr, result.handle))

    def gather_slabs(self, layer: Frame, result: Frame = None):
        """Collective (RCCL), the tile split's exchange: every rank's slab of rows (Frame.set_tile_rows) straight into rank 0's `result`."""
        check(self.lib.crh_frame_gather_slabs(self.handle, layer.handle, result.handle if result is not None else None))

    def local_gather_slabs(self, layers, result: Frame):
        """... over the loopback group, called on rank 0's communicator."""
        arr = (C.c_void_p * len(layers))(*[f.handle for f in layers])
        check(self.lib.crh_comm_local_gather_slabs(self.handle, arr, result.handle))

    def last_traffic(self):
        sent, dense = C.c_uint64(), C.c_uint64()
        check(self.lib.crh_comm_last_traffic(self.handle, C.byref(sent), C.byref(dense)))
        return sent.value, dense.value

    PHASES = ("pack", "allgather_plan", "alltoall", "composite", "gather", "unpack")

    def last_timing(self):
        """GPU milliseconds of the phases of this rank's last exchange (waits for it): dict by phase name."""
        ms = (C.c_float * len(self.PHASES))()
        check(self.lib.crh_comm_last_timing(self.handle, ms))
        return dict(zip(self.PHASES, [float(v) for v in ms]))

    def last_peer_bytes(self):
        """Bytes this rank sent to every peer in the all-to-all of the last exchange."""
        out = (C.c_uint64 * self.world)()
        check(self.lib.crh_comm_last_peer_bytes(self.handle, out))
        return [int(v) for v in out]

    def info(self):
        """{"nranks": ncclCommCount (or the loopback group's size), "rccl_version": ncclGetVersion's code, 0 for a loopback communicator}"""
        n, v = C.c_uint32(), C.c_int32()
        check(self.lib.crh_comm_info(self.handle, C.byref(n), C.byref(v)))
        return {"nranks": int(n.value), "rccl_version": int(v.value)}

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.crh_comm_destroy(self.handle)
            self.handle = None


class Scene:
    """A batch of Shapes in HBM: upload + tessellate once, render many times."""

    def __init__(self, renderer: Renderer, batch: _ffi.PathBatch, tessellate=True, existing: "Scene" = None):
        self.renderer = renderer
        self.lib = renderer.lib
        self.batch = batch
        handle = C.c_void_p()
        check(self.lib.crh_scene_upload(renderer.handle, C.byref(batch.c), existing.handle if existing else None, C.byref(handle)))
        if existing is not None:
            existing.handle = None  # moved in, as `existing_shape` is in renderer.rs:182
        self.handle = handle
        self._pass_paints = getattr(existing, "_pass_paints", None)  # the paint table a RenderPass installed stays with the C scene
        self.n_shapes = batch.n_shapes
        if tessellate:
            self.tessellate()

    def tessellate(self):
        check(self.lib.crh_scene_tessellate(self.handle))

    def status(self):
        return self.lib.crh_scene_status(self.handle)

    def check(self):
        check(self.status())

    def shape(self, index):
        """-> (vertex_offsets[8], index_offsets[3], vertex bytes, index bytes): the byte image of renderer.rs:198-209."""
        vo = (C.c_uint64 * 8)()
        io = (C.c_uint64 * 3)()
        check(self.lib.crh_scene_shape_layout(self.handle, index, vo, io))
        vb = np.zeros(vo[7], dtype=np.uint8)
        ib = np.zeros(io[2], dtype=np.uint8)
        check(self.lib.crh_scene_shape_download(self.handle, index, vb.ctypes.data, ib.ctypes.data))
        return np.array(vo[:], dtype=np.uint64), np.array(io[:], dtype=np.uint64), vb, ib

    def all_shapes(self):
        layout = np.zeros((self.n_shapes, 11), dtype=np.uint64)
        tv, ti = C.c_uint64(), C.c_uint64()
        check(self.lib.crh_scene_layout_all(self.handle, layout.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(tv), C.byref(ti)))
        vb = np.zeros(tv.value, dtype=np.uint8)
        ib = np.zeros(ti.value, dtype=np.uint8)
        check(self.lib.crh_scene_download_all(self.handle, vb.ctypes.data, ib.ctypes.data))
        return layout, vb, ib

    def traffic(self):
        r, w = C.c_uint64(), C.c_uint64()
        check(self.lib.crh_scene_traffic(self.handle, C.byref(r), C.byref(w)))
        return r.value, w.value

    def set_instances(self, transforms, colors):
        t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(self.n_shapes, 16)
        c = np.ascontiguousarray(colors, dtype=np.float32).reshape(self.n_shapes, 4)
        fp = C.POINTER(C.c_float)
        check(self.lib.crh_scene_set_instances(self.handle, t.ctypes.data_as(fp), c.ctypes.data_as(fp)))

    def set_paints(self, paints, instance_paint):
        """crh_scene_set_paints: `paints` = [Paint or ImagePaint, mixed], `instance_paint[i]` = the index of instance i's paint or -1 for its solid colour (instances
        beyond the list are solid). Stays with the Scene until the next call; an empty `paints` clears it. The call waits for the renderer's
        work in flight (the kernels of a pass read the table): set it when it changes, not per frame. A list with an ImagePaint goes through
        crh_scene_set_paints_with_images (gradients first, the indices remapped); the table keeps the pixels of its images."""
        self._install_paints(paints, instance_paint)
        self._pass_paints = None  # the caller's own table: passes without paints leave it alone

    def _install_paints(self, paints, instance_paint):
        if any(isinstance(p, ImagePaint) for p in paints):
            gradients, images, remapped = split_paints(paints, instance_paint)
            table = (_ffi.PaintC * max(1, len(gradients)))(*[p.to_c() for p in gradients])
            image_table = (_ffi.ImagePaintC * len(images))(*[p.to_c() for p in images])
            which = np.ascontiguousarray(remapped, dtype=np.int32).ravel()
            check(self.lib.crh_scene_set_paints_with_images(self.handle, table if gradients else None, len(gradients), image_table, len(images),
                                                            which.ctypes.data_as(C.POINTER(C.c_int32)) if len(which) else None, len(which)))
            return
        table = (_ffi.PaintC * max(1, len(paints)))(*[p.to_c() for p in paints])
        which = np.ascontiguousarray(instance_paint, dtype=np.int32).ravel()
        check(self.lib.crh_scene_set_paints(self.handle, table if len(paints) else None, len(paints), which.ctypes.data_as(C.POINTER(C.c_int32)) if len(which) else None, len(which)))

    def _paints_of_pass(self, paints, instance_paint):
        """What RenderPass.submit asks for in front of its draws: the pass's table (None: the pass has no paints). A table an earlier pass put here
        belongs to that pass's instance numbering, so it is replaced or removed; the call is skipped when the Scene already holds this very table."""
        key = (tuple(paints), tuple(instance_paint)) if paints else None
        if key == getattr(self, "_pass_paints", None):
            return
        if key is None:
            self._install_paints([], [])
        else:
            self._install_paints(paints, instance_paint)
        self._pass_paints = key

    def render(self, frame: Frame, transforms=None, colors=None):
        """Stencil + Color of every shape in index order (the loop of examples/showcase/main.rs:236-250)."""
        self._paints_of_pass(None, None)  # (a table a RenderPass left belongs to that pass's instances)
        if transforms is not None:
            self.set_instances(transforms, colors)
        check(self.lib.crh_scene_render_resident(self.handle, frame.handle))

    def render_draws(self, frame: Frame, transforms, colors, draws, _from_pass=False):
        """A recorded render pass: draws = [(shape, instance, RenderOperation, clip_depth, alpha_layer), ...] — one tuple per
        Shape::render call (renderer.rs:267-273) with the clip depth (Renderer::set_clip_depth, renderer.rs:932-938) and alpha layer
        (save/restore_alpha_context, renderer.rs:941-985) in effect. `instance` indexes transforms / colors (instancing)."""
        if not _from_pass:
            self._paints_of_pass(None, None)  # (a table a RenderPass left belongs to that pass's instances; the caller's own table stays)
        t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 16)
        c = np.ascontiguousarray(colors, dtype=np.float32).reshape(-1, 4)
        assert len(t) == len(c)
        if isinstance(draws, np.ndarray):  # [n, 5] uint32 = crh_draw records: passed as they are (an animation re-submits the same array)
            table = np.ascontiguousarray(draws, dtype=np.uint32).reshape(-1, 5)
        else:
            table = np.zeros((len(draws), 5), dtype=np.uint32)
            for i, d in enumerate(draws):
                table[i, :len(d)] = [int(v) for v in d]
        fp = C.POINTER(C.c_float)
        check(self.lib.crh_scene_render_draws(self.handle, frame.handle, t.ctypes.data_as(fp), c.ctypes.data_as(fp), len(t),
                                              table.ctypes.data_as(C.POINTER(_ffi.DrawC)), len(table)))

    def set_dynamic_stroke_options(self, shape_index, group_index, options):
        c = options.to_c()
        check(self.lib.crh_scene_set_dynamic_stroke_options(self.handle, shape_index, group_index, C.byref(c)))

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.crh_scene_destroy(self.handle)
            self.handle = None


class Shape(Scene):
    """contrast_renderer::renderer::Shape — `Shape.from_paths` mirrors renderer.rs:177-249 (synchronous, raises ContrastError)."""

    @staticmethod
    def from_paths(renderer: Renderer, dynamic_stroke_options, paths, existing_shape: "Shape" = None):
        batch = batch_from_shapes([(list(dynamic_stroke_options), list(paths))])
        shape = Shape.__new__(Shape)
        Scene.__init__(shape, renderer, batch, tessellate=True, existing=existing_shape)
        shape.check()
        return shape

    def buffers(self):
        return self.shape(0)

    def render_in(self, render_pass: "RenderPass", instance_indices, render_operation):
        """Shape::render(&self, &renderer, &mut render_pass, instance_indices, render_operation), renderer.rs:267-273."""
        render_pass.render(self, instance_indices, render_operation, 0)

    def render_instance(self, frame: Frame, transform, color):
        """render(Stencil) followed by render(Color) for one instance."""
        self.render(frame, np.asarray(transform, dtype=np.float32).reshape(1, 16), np.asarray(color, dtype=np.float32).reshape(1, 4))


class RenderPass:
    """wgpu::RenderPass stand-in: records `Shape::render(&renderer, &mut render_pass, instance_indices, operation)` calls (renderer.rs:267-273)
    with the pass state they see — the stencil reference of Renderer::set_clip_depth (renderer.rs:932-938), the layer of save_ / restore_alpha_context
    (renderer.rs:941-985) — and submits them in order. The Shapes may be different objects (a Shape, a Scene): the frame keeps clip nesting counters,
    winding counters, saved alphas and sample colours between the submissions (crh_frame: `carry`), so the documented pattern works as it does in
    the reference (renderer.rs:257-266):

        a.render(pass, range(0, 1), Op.Stencil); pass.set_clip_depth(1); a.render(pass, range(0, 1), Op.Clip)
        b.render(pass, ...Stencil); b.render(pass, ...Color)        # another Shape object, clipped by a
        pass.set_clip_depth(0); a.render(pass, range(0, 1), Op.UnClip)
    """

    def __init__(self, renderer: Renderer, frame: Frame):
        self.renderer, self.frame = renderer, frame
        self.transforms, self.colors, self.draws = [], [], []  # draws: (scene, shape, instance, op, clip_depth, alpha_layer)
        self.paints, self.instance_paint = [], []  # the pass's paints and, per instance, the index of its paint or -1
        self.clip_depth = self.alpha_layer = 0

    def push_instance(self, transform, color, paint=None):
        """Instance data of the pass (the instance buffers bound at slots 0 / 2, renderer.rs:462-466): returns the instance index.
        `paint`: a Paint or an ImagePaint that takes the place of `color` as the source of the instance's Color covers (times `color`)."""
        self.transforms.append(np.asarray(transform, dtype=np.float32).reshape(16))
        self.colors.append(np.asarray(color, dtype=np.float32).reshape(4))
        if paint is None:
            self.instance_paint.append(-1)
        else:
            if paint not in self.paints:
                self.paints.append(paint)
            self.instance_paint.append(self.paints.index(paint))
        return len(self.colors) - 1

    def set_clip_depth(self, clip_depth):  # Renderer::set_clip_depth, renderer.rs:932-938
        if clip_depth >= (1 << self.renderer.config.clip_nesting_counter_bits):
            raise ContrastError(_ffi.ERR_CLIP_STACK_OVERFLOW, "ClipStackOverflow")
        self.clip_depth = int(clip_depth)

    def set_alpha_layer(self, alpha_layer):  # the layer save_alpha_context / restore_alpha_context bind, renderer.rs:941-985
        if alpha_layer >= self.renderer.config.alpha_layer_count:
            raise ContrastError(_ffi.ERR_TOO_MANY_NESTED_OPACITY_GROUPS, "TooManyNestedOpacityGroups")
        self.alpha_layer = int(alpha_layer)

    def render(self, scene: "Scene", instance_indices, operation, shape_index=0):
        for i in instance_indices:
            self.draws.append((scene, int(shape_index), int(i), int(operation), self.clip_depth, self.alpha_layer))

    def submit(self):
        """End of the pass: everything recorded executes in order, one crh_scene_render_draws per run of draws of the same Scene object."""
        if any(d[0] is not self.draws[0][0] for d in self.draws):
            self.frame.keep_pass_state()  # the pass spans objects: every sample's colour and stencil stay with the frame from its first draw on
        begin = 0
        while begin < len(self.draws):
            end = begin
            while end < len(self.draws) and self.draws[end][0] is self.draws[begin][0]:
                end += 1
            # every Scene of the pass draws with the pass's paints; a pass without any removes what an earlier pass installed (whose instance
            # indices are not this pass's) and leaves a table the caller set with Scene.set_paints alone
            self.draws[begin][0]._paints_of_pass(self.paints, self.instance_paint)
            self.draws[begin][0].render_draws(self.frame, np.stack(self.transforms), np.stack(self.colors), [d[1:] for d in self.draws[begin:end]], _from_pass=True)
            begin = end
        self.draws = []

