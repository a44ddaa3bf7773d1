"""ctypes mirror of include/contrast_hip.h (structs, enums) and the loader of libcontrast_hip.so.

Plumbing only: the product is the HIP library behind the C ABI. Nothing here computes geometry, and
nothing here may import `oracle` (the CPU oracle is test infrastructure).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcontrast_hip.so")

# ---- status codes (error.rs:5-16 + panics of the reference surfaced as codes) -------------------------------
OK = 0
ERR_NUMBER_OF_STENCIL_BITS_IS_UNSUPPORTED = 1
ERR_CLIP_STACK_OVERFLOW = 2
ERR_TOO_MANY_NESTED_OPACITY_GROUPS = 3
ERR_TOO_MANY_DASH_INTERVALS = 4
ERR_DYNAMIC_STROKE_OPTIONS_INDEX_OUT_OF_BOUNDS = 5
ERR_NON_FINITE = 6
ERR_DEGENERATE_CUBIC = 7
ERR_UNSUPPORTED = 8
ERR_HIP = 9
ERR_INVALID_ARGUMENT = 10

STATUS_NAMES = {
    0: "Ok",
    1: "NumberOfStencilBitsIsUnsupported",
    2: "ClipStackOverflow",
    3: "TooManyNestedOpacityGroups",
    4: "TooManyDashIntervals",
    5: "DynamicStrokeOptionsIndexOutOfBounds",
    6: "NonFinite (the reference panics: safe_float.rs:46,114)",
    7: "DegenerateCubic (the reference panics: fill.rs:174,178)",
    8: "Unsupported",
    9: "HipError",
    10: "InvalidArgument",
}

SEGMENT_LINE, SEGMENT_INTEGRAL_QUADRATIC, SEGMENT_INTEGRAL_CUBIC, SEGMENT_RATIONAL_QUADRATIC, SEGMENT_RATIONAL_CUBIC = range(5)
SEGMENT_FLOATS = (2, 4, 6, 5, 10)
MAX_DASH_INTERVALS = 4


class StrokeOptionsC(C.Structure):
    _fields_ = [
        ("width", C.c_float),
        ("offset", C.c_float),
        ("miter_clip", C.c_float),
        ("closed", C.c_uint32),
        ("dynamic_stroke_options_group", C.c_uint32),
        ("curve_approximation", C.c_uint32),
        ("steps", C.c_uint32),
        ("angle_step", C.c_float),
    ]


class DashIntervalC(C.Structure):
    _fields_ = [("gap_start", C.c_float), ("gap_end", C.c_float), ("dash_start", C.c_uint32), ("dash_end", C.c_uint32)]


class DynamicStrokeOptionsC(C.Structure):
    _fields_ = [
        ("dashed", C.c_uint32),
        ("join", C.c_uint32),
        ("pattern_len", C.c_uint32),
        ("pattern", DashIntervalC * MAX_DASH_INTERVALS),
        ("phase", C.c_float),
        ("start", C.c_uint32),
        ("end", C.c_uint32),
    ]


class DynamicStrokeDescriptorC(C.Structure):
    _fields_ = [
        ("gap_start", C.c_float * MAX_DASH_INTERVALS),
        ("gap_end", C.c_float * MAX_DASH_INTERVALS),
        ("caps", C.c_uint32),
        ("count_dashed_join", C.c_uint32),
        ("phase", C.c_float),
        ("_padding", C.c_uint32),
    ]


class PathBatchC(C.Structure):
    _fields_ = [
        ("n_shapes", C.c_uint32),
        ("shape_path_begin", C.POINTER(C.c_uint32)),
        ("n_paths", C.c_uint32),
        ("path_segment_begin", C.POINTER(C.c_uint32)),
        ("path_start", C.POINTER(C.c_float)),
        ("path_stroke_options", C.POINTER(C.c_int32)),
        ("n_segments", C.c_uint32),
        ("segment_types", C.POINTER(C.c_uint8)),
        ("control_data", C.POINTER(C.c_float)),
        ("n_control_floats", C.c_uint32),
        ("n_stroke_options", C.c_uint32),
        ("stroke_options", C.POINTER(StrokeOptionsC)),
        ("shape_dynamic_begin", C.POINTER(C.c_uint32)),
        ("n_dynamic_stroke_options", C.c_uint32),
        ("dynamic_stroke_options", C.POINTER(DynamicStrokeOptionsC)),
    ]


class ConfigC(C.Structure):
    _fields_ = [
        ("msaa_sample_count", C.c_uint32),
        ("clip_nesting_counter_bits", C.c_uint32),
        ("winding_counter_bits", C.c_uint32),
        ("alpha_layer_count", C.c_uint32),
        ("cull_mode", C.c_uint32),
        ("depth_compare", C.c_uint32),
        ("depth_write_enabled", C.c_uint32),
    ]


class BlendComponentC(C.Structure):  # crh_blend_component = wgpu::BlendComponent
    _fields_ = [("src_factor", C.c_uint32), ("dst_factor", C.c_uint32), ("operation", C.c_uint32)]


class ColorTargetStateC(C.Structure):  # crh_color_target_state = wgpu::ColorTargetState without the format (+ the blend constant)
    _fields_ = [
        ("blend_enabled", C.c_uint32),
        ("color", BlendComponentC),
        ("alpha", BlendComponentC),
        ("write_mask", C.c_uint32),
        ("constant", C.c_float * 4),
    ]


class KernelTimeC(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_float), ("algorithmic_bytes", C.c_uint64)]


def _ptr(array, ctype):
    return array.ctypes.data_as(C.POINTER(ctype))


class PathBatch:
    """Struct-of-arrays batch of Shapes (see crh_path_batch). Owns numpy arrays; `.c` is the C view."""

    def __init__(self, shape_path_begin, path_segment_begin, path_start, path_stroke_options, segment_types, control_data, stroke_options=(),
                 shape_dynamic_begin=None, dynamic_stroke_options=()):
        self.shape_path_begin = np.ascontiguousarray(shape_path_begin, dtype=np.uint32)
        self.path_segment_begin = np.ascontiguousarray(path_segment_begin, dtype=np.uint32)
        self.path_start = np.ascontiguousarray(path_start, dtype=np.float32).reshape(-1, 2)
        self.path_stroke_options = np.ascontiguousarray(path_stroke_options, dtype=np.int32)
        self.segment_types = np.ascontiguousarray(segment_types, dtype=np.uint8)
        self.control_data = np.ascontiguousarray(control_data, dtype=np.float32).reshape(-1)
        self.n_shapes = len(self.shape_path_begin) - 1
        self.n_paths = len(self.path_segment_begin) - 1
        self.n_segments = len(self.segment_types)
        assert self.path_start.shape[0] == self.n_paths and len(self.path_stroke_options) == self.n_paths
        assert int(self.shape_path_begin[-1]) == self.n_paths and int(self.path_segment_begin[-1]) == self.n_segments
        sizes = np.asarray(SEGMENT_FLOATS, dtype=np.int64)[self.segment_types]
        assert int(sizes.sum()) == self.control_data.size, "control_data does not match segment_types"
        self.stroke_options = (StrokeOptionsC * max(1, len(stroke_options)))(*stroke_options)
        self.n_stroke_options = len(stroke_options)
        if shape_dynamic_begin is None:
            shape_dynamic_begin = np.zeros(self.n_shapes + 1, dtype=np.uint32)
        self.shape_dynamic_begin = np.ascontiguousarray(shape_dynamic_begin, dtype=np.uint32)
        self.dynamic_stroke_options = (DynamicStrokeOptionsC * max(1, len(dynamic_stroke_options)))(*dynamic_stroke_options)
        self.n_dynamic_stroke_options = len(dynamic_stroke_options)
        c = PathBatchC()
        c.n_shapes = self.n_shapes
        c.shape_path_begin = _ptr(self.shape_path_begin, C.c_uint32)
        c.n_paths = self.n_paths
        c.path_segment_begin = _ptr(self.path_segment_begin, C.c_uint32)
        c.path_start = _ptr(self.path_start, C.c_float)
        c.path_stroke_options = _ptr(self.path_stroke_options, C.c_int32)
        c.n_segments = self.n_segments
        c.segment_types = _ptr(self.segment_types, C.c_uint8)
        c.control_data = _ptr(self.control_data, C.c_float)
        c.n_control_floats = self.control_data.size
        c.n_stroke_options = self.n_stroke_options
        c.stroke_options = C.cast(self.stroke_options, C.POINTER(StrokeOptionsC))
        c.shape_dynamic_begin = _ptr(self.shape_dynamic_begin, C.c_uint32)
        c.n_dynamic_stroke_options = self.n_dynamic_stroke_options
        c.dynamic_stroke_options = C.cast(self.dynamic_stroke_options, C.POINTER(DynamicStrokeOptionsC))
        self.c = c

    def input_bytes(self):
        """Algorithmic input bytes of SURVEY.md §8(d): control bytes + 1 type byte per segment, 8 B start (+ 32 B options) per path."""
        stroked = int((self.path_stroke_options >= 0).sum())
        return self.control_data.nbytes + self.n_segments + 8 * self.n_paths + 32 * stroked

    def slice_shapes(self, begin, end):
        """The contiguous shape range [begin, end) as its own batch (path-index sharding)."""
        p0, p1 = int(self.shape_path_begin[begin]), int(self.shape_path_begin[end])
        s0, s1 = int(self.path_segment_begin[p0]), int(self.path_segment_begin[p1])
        sizes = np.asarray(SEGMENT_FLOATS, dtype=np.int64)[self.segment_types]
        offsets = np.concatenate([[0], np.cumsum(sizes)])
        d0, d1 = int(self.shape_dynamic_begin[begin]), int(self.shape_dynamic_begin[end])
        return PathBatch(
            self.shape_path_begin[begin:end + 1] - p0,
            self.path_segment_begin[p0:p1 + 1] - s0,
            self.path_start[p0:p1],
            self.path_stroke_options[p0:p1],
            self.segment_types[s0:s1],
            self.control_data[int(offsets[s0]):int(offsets[s1])],
            [self.stroke_options[i] for i in range(self.n_stroke_options)],
            self.shape_dynamic_begin[begin:end + 1] - d0,
            [self.dynamic_stroke_options[i] for i in range(d0, d1)],
        )


class DrawC(C.Structure):
    _fields_ = [("shape", C.c_uint32), ("instance", C.c_uint32), ("op", C.c_uint32), ("clip_depth", C.c_uint32), ("alpha_layer", C.c_uint32)]


MAX_GRADIENT_STOPS = 8  # CRH_MAX_GRADIENT_STOPS


class GradientStopC(C.Structure):  # crh_gradient_stop
    _fields_ = [("offset", C.c_float), ("color", C.c_float * 4)]


class PaintC(C.Structure):  # crh_paint
    _fields_ = [("kind", C.c_uint32), ("spread", C.c_uint32), ("p0", C.c_float * 2), ("p1", C.c_float * 2), ("n_stops", C.c_uint32),
                ("stops", GradientStopC * MAX_GRADIENT_STOPS)]


class ImagePaintC(C.Structure):  # crh_image_paint
    _fields_ = [("image", C.c_void_p), ("filter", C.c_uint32), ("spread_x", C.c_uint32), ("spread_y", C.c_uint32), ("m", C.c_float * 6)]


class CompositeC(C.Structure):  # crh_composite
    _fields_ = [("op", C.c_uint32), ("mode", C.c_uint32), ("opacity", C.c_float), ("x", C.c_int32), ("y", C.c_int32)]


class ConvolveC(C.Structure):  # crh_convolve
    _fields_ = [("order_x", C.c_uint32), ("order_y", C.c_uint32), ("target_x", C.c_uint32), ("target_y", C.c_uint32), ("kernel", C.POINTER(C.c_float)),
                ("divisor", C.c_float), ("bias", C.c_float), ("edge", C.c_uint32), ("preserve_alpha", C.c_uint32)]


class LightingC(C.Structure):  # crh_lighting
    _fields_ = [("op", C.c_uint32), ("light", C.c_uint32), ("edge", C.c_uint32), ("surface_scale", C.c_float), ("constant", C.c_float), ("specular_exponent", C.c_float),
                ("color", C.c_float * 3), ("azimuth", C.c_float), ("elevation", C.c_float), ("position", C.c_float * 3), ("points_at", C.c_float * 3),
                ("spot_exponent", C.c_float), ("cone_angle", C.c_float)]


class TurbulenceC(C.Structure):  # crh_turbulence
    _fields_ = [("kind", C.c_uint32), ("octaves", C.c_uint32), ("seed", C.c_int32), ("stitch", C.c_uint32), ("opaque", C.c_uint32), ("base_frequency", C.c_float * 2),
                ("offset", C.c_float * 2)]


class DisplaceC(C.Structure):  # crh_displace
    _fields_ = [("scale", C.c_float * 2), ("x_channel", C.c_uint32), ("y_channel", C.c_uint32), ("filter", C.c_uint32), ("edge", C.c_uint32)]


class DistanceC(C.Structure):  # crh_distance
    _fields_ = [("mode", C.c_uint32), ("channel", C.c_uint32), ("threshold", C.c_uint32), ("spread", C.c_uint32), ("edge", C.c_uint32)]


class ImageStatsC(C.Structure):  # crh_image_stats: 4116 bytes
    _fields_ = [("histogram", C.c_uint32 * 1024), ("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32), ("count", C.c_uint32)]


class VariableBlurC(C.Structure):  # crh_variable_blur
    _fields_ = [("sigma_x", C.c_float * 2), ("sigma_y", C.c_float * 2), ("channel", C.c_uint32), ("edge", C.c_uint32)]


class TransformC(C.Structure):  # crh_transform
    _fields_ = [("matrix", C.c_double * 9), ("width", C.c_uint32), ("height", C.c_uint32), ("filter", C.c_uint32), ("edge", C.c_uint32)]


class FontMetricsC(C.Structure):
    _fields_ = [("units_per_em", C.c_uint32), ("number_of_glyphs", C.c_uint32), ("ascender", C.c_int32), ("descender", C.c_int32),
                ("line_gap", C.c_int32), ("height", C.c_int32), ("has_x_height", C.c_int32), ("x_height", C.c_int32),
                ("has_vertical_metrics", C.c_int32), ("vertical_height", C.c_int32), ("vertical_line_gap", C.c_int32), ("has_kerning", C.c_int32)]


class TextLayoutC(C.Structure):
    _fields_ = [("size", C.c_float), ("orientation", C.c_uint32), ("major_alignment", C.c_uint32), ("minor_alignment", C.c_uint32)]


_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so. If this library (linked against the system ROCm) is loaded first and torch
    afterwards, the process holds two HIP runtimes and the second one sees no device. Importing torch first (when it is installed) makes
    the dynamic loader bind libcontrast_hip.so to the runtime torch uses — which bench.py needs anyway to hand frames to RCCL."""
    import importlib.util
    import sys
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


def load_library():
    """Loads the HIP library. Fails loudly when it is missing: there is no CPU fallback in the product."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). contrast_renderer_amd has no CPU fallback.")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    V = C.c_void_p
    sig = {
        "crh_renderer_create": (C.c_int, [C.POINTER(ConfigC), C.c_int, C.POINTER(V)]),
        "crh_renderer_destroy": (None, [V]),
        "crh_renderer_get_config": (C.c_int, [V, C.POINTER(ConfigC)]),
        "crh_renderer_create_blended": (C.c_int, [C.POINTER(ConfigC), C.POINTER(ColorTargetStateC), C.c_int, C.POINTER(V)]),
        "crh_renderer_get_blending": (C.c_int, [V, C.POINTER(ColorTargetStateC)]),
        "crh_convert_dynamic_stroke_options": (C.c_int, [C.POINTER(DynamicStrokeOptionsC), C.POINTER(DynamicStrokeDescriptorC)]),
        "crh_scene_upload": (C.c_int, [V, C.POINTER(PathBatchC), V, C.POINTER(V)]),
        "crh_scene_tessellate": (C.c_int, [V]),
        "crh_scene_status": (C.c_int, [V]),
        "crh_scene_destroy": (None, [V]),
        "crh_shape_from_paths": (C.c_int, [V, C.POINTER(PathBatchC), V, C.POINTER(V)]),
        "crh_scene_shape_layout": (C.c_int, [V, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "crh_scene_shape_download": (C.c_int, [V, C.c_uint32, V, V]),
        "crh_scene_layout_all": (C.c_int, [V, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "crh_scene_download_all": (C.c_int, [V, V, V]),
        "crh_scene_traffic": (C.c_int, [V, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "crh_scene_set_dynamic_stroke_options": (C.c_int, [V, C.c_uint32, C.c_uint32, C.POINTER(DynamicStrokeOptionsC)]),
        "crh_frame_create": (C.c_int, [V, C.c_uint32, C.c_uint32, C.POINTER(V)]),
        "crh_frame_create_format": (C.c_int, [V, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(V)]),
        "crh_frame_format": (C.c_int, [V, C.POINTER(C.c_uint32)]),
        "crh_frame_destroy": (None, [V]),
        "crh_frame_clear": (C.c_int, [V]),
        "crh_frame_keep_pass_state": (C.c_int, [V]),
        "crh_frame_synchronize": (C.c_int, [V]),
        "crh_frame_set_tile_rows": (C.c_int, [V, C.c_uint32, C.c_uint32]),
        "crh_frame_clear_depth": (C.c_int, [V, C.c_float]),
        "crh_frame_upload_depth": (C.c_int, [V, C.POINTER(C.c_float)]),
        "crh_frame_download_depth": (C.c_int, [V, C.POINTER(C.c_float)]),
        "crh_scene_render": (C.c_int, [V, V, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "crh_scene_set_instances": (C.c_int, [V, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "crh_scene_render_resident": (C.c_int, [V, V]),
        "crh_scene_render_draws": (C.c_int, [V, V, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.POINTER(DrawC), C.c_uint32]),
        "crh_paint_validate": (C.c_int, [C.POINTER(PaintC)]),
        "crh_scene_set_paints": (C.c_int, [V, C.POINTER(PaintC), C.c_uint32, C.POINTER(C.c_int32), C.c_uint32]),
        "crh_image_create": (C.c_int, [V, C.c_uint32, C.c_uint32, V, C.POINTER(V)]),
        "crh_image_create_from_frame": (C.c_int, [V, C.POINTER(V)]),
        "crh_image_size": (C.c_int, [V, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "crh_image_destroy": (None, [V]),
        "crh_image_generate_mipmaps": (C.c_int, [V]),
        "crh_image_level_count": (C.c_int, [V, C.POINTER(C.c_uint32)]),
        "crh_image_download_level": (C.c_int, [V, C.c_uint32, V, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "crh_blur_taps": (C.c_int, [C.c_float, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]),
        "crh_image_blur": (C.c_int, [V, C.c_float, C.c_float, C.c_uint32, C.POINTER(V)]),
        "crh_composite_validate": (C.c_int, [C.POINTER(CompositeC)]),
        "crh_composite_texels": (C.c_int, [C.POINTER(CompositeC), V, V, C.c_uint64, V]),
        "crh_image_composite": (C.c_int, [V, V, C.POINTER(CompositeC), C.POINTER(V)]),
        "crh_color_filter_validate": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_uint8)]),
        "crh_color_filter_texels": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_uint8), V, C.c_uint64, V]),
        "crh_image_color_filter": (C.c_int, [V, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(V)]),
        "crh_morphology_size": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "crh_morphology_texels": (C.c_int, [C.c_uint32, C.c_uint32, V, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, V]),
        "crh_image_morphology": (C.c_int, [V, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(V)]),
        "crh_convolve_validate": (C.c_int, [C.POINTER(ConvolveC)]),
        "crh_convolve_coefficients": (C.c_int, [C.POINTER(ConvolveC), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_int32)]),
        "crh_convolve_texels": (C.c_int, [C.c_uint32, C.c_uint32, V, C.POINTER(ConvolveC), V]),
        "crh_image_convolve": (C.c_int, [V, C.POINTER(ConvolveC), C.POINTER(V)]),
        "crh_lighting_validate": (C.c_int, [C.POINTER(LightingC)]),
        "crh_lighting_texels": (C.c_int, [C.c_uint32, C.c_uint32, V, C.POINTER(LightingC), V]),
        "crh_image_lighting": (C.c_int, [V, C.POINTER(LightingC), C.POINTER(V)]),
        "crh_turbulence_validate": (C.c_int, [C.POINTER(TurbulenceC)]),
        "crh_turbulence_tables": (C.c_int, [C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_double)]),
        "crh_turbulence_texels": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(TurbulenceC), V]),
        "crh_image_turbulence": (C.c_int, [V, C.c_uint32, C.c_uint32, C.POINTER(TurbulenceC), C.POINTER(V)]),
        "crh_displace_validate": (C.c_int, [C.POINTER(DisplaceC)]),
        "crh_displace_offset": (C.c_int, [C.POINTER(DisplaceC), C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]),
        "crh_displace_texels": (C.c_int, [C.c_uint32, C.c_uint32, V, V, C.POINTER(DisplaceC), V]),
        "crh_image_displace": (C.c_int, [V, V, C.POINTER(DisplaceC), C.POINTER(V)]),
        "crh_distance_validate": (C.c_int, [C.POINTER(DistanceC)]),
        "crh_distance_code": (C.c_int, [C.POINTER(DistanceC), C.c_uint64, C.POINTER(C.c_uint32)]),
        "crh_distance_size": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(DistanceC), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "crh_distance_texels": (C.c_int, [C.c_uint32, C.c_uint32, V, C.POINTER(DistanceC), V]),
        "crh_image_distance_field": (C.c_int, [V, C.POINTER(DistanceC), C.POINTER(V)]),
        "crh_resize_taps": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_uint16), C.POINTER(C.c_int16), C.c_uint64, C.POINTER(C.c_uint64)]),
        "crh_resize_texels": (C.c_int, [C.c_uint32, C.c_uint32, V, C.c_uint32, C.c_uint32, C.c_uint32, V]),
        "crh_image_resize": (C.c_int, [V, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(V)]),
        "crh_crop_texels": (C.c_int, [C.c_uint32, C.c_uint32, V, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, V]),
        "crh_statistics_texels": (C.c_int, [C.c_uint32, C.c_uint32, V, C.c_uint32, C.c_uint32, C.POINTER(ImageStatsC)]),
        "crh_image_crop": (C.c_int, [V, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(V)]),
        "crh_image_create_from_frame_region": (C.c_int, [V, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(V)]),
        "crh_image_statistics": (C.c_int, [V, C.c_uint32, C.c_uint32, C.POINTER(ImageStatsC)]),
        "crh_variable_blur_validate": (C.c_int, [C.POINTER(VariableBlurC)]),
        "crh_variable_blur_sigma": (C.c_int, [C.POINTER(VariableBlurC), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "crh_variable_blur_texels": (C.c_int, [C.c_uint32, C.c_uint32, V, V, C.POINTER(VariableBlurC), V]),
        "crh_image_variable_blur": (C.c_int, [V, V, C.POINTER(VariableBlurC), C.POINTER(V)]),
        "crh_transform_validate": (C.c_int, [C.POINTER(TransformC)]),
        "crh_transform_fit": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_uint32, C.c_uint32, C.POINTER(TransformC), C.POINTER(C.c_int32)]),
        "crh_transform_position": (C.c_int, [C.POINTER(TransformC), C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]),
        "crh_transform_texels": (C.c_int, [C.c_uint32, C.c_uint32, V, C.POINTER(TransformC), V]),
        "crh_image_transform": (C.c_int, [V, C.POINTER(TransformC), C.POINTER(V)]),
        "crh_image_paint_validate": (C.c_int, [C.POINTER(ImagePaintC)]),
        "crh_scene_set_paints_with_images": (C.c_int, [V, C.POINTER(PaintC), C.c_uint32, C.POINTER(ImagePaintC), C.c_uint32, C.POINTER(C.c_int32), C.c_uint32]),
        "crh_frame_upload": (C.c_int, [V, V]),
        "crh_frame_load_image": (C.c_int, [V, V]),
        "crh_frame_download": (C.c_int, [V, V]),
        "crh_frame_download_f16": (C.c_int, [V, V]),
        "crh_frame_device_pointer": (C.c_int, [V, C.POINTER(V)]),
        "crh_composite_over": (C.c_int, [V, C.POINTER(V), C.c_uint32, C.c_uint64, V]),
        "crh_comm_shard": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "crh_comm_slab_rows": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "crh_comm_unique_id": (C.c_int, [V]),
        "crh_comm_create": (C.c_int, [V, C.c_uint32, C.c_uint32, V, C.POINTER(V)]),
        "crh_comm_create_local": (C.c_int, [V, C.c_uint32, C.c_uint32, V, C.POINTER(V)]),
        "crh_comm_destroy": (None, [V]),
        "crh_frame_exchange": (C.c_int, [V, V, V]),
        "crh_frame_gather_slabs": (C.c_int, [V, V, V]),
        "crh_comm_local_exchange": (C.c_int, [V, C.POINTER(V), V]),
        "crh_comm_local_gather_slabs": (C.c_int, [V, C.POINTER(V), V]),
        "crh_comm_last_traffic": (C.c_int, [V, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "crh_comm_last_timing": (C.c_int, [V, C.POINTER(C.c_float)]),
        "crh_comm_last_peer_bytes": (C.c_int, [V, C.POINTER(C.c_uint64)]),
        "crh_comm_info": (C.c_int, [V, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
        "crh_renderer_synchronize": (C.c_int, [V]),
        "crh_renderer_stream": (V, [V]),
        "crh_renderer_enable_timing": (C.c_int, [V, C.c_int]),
        "crh_renderer_kernel_times": (C.c_int, [V, C.POINTER(KernelTimeC), C.c_uint32, C.POINTER(C.c_uint32)]),
        "crh_selftest_fmath": (C.c_int, [V, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint64]),
        "crh_selftest_srgb": (C.c_int, [V, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_float)]),
        "crh_font_create": (C.c_int, [V, C.c_size_t, C.POINTER(V)]),
        "crh_font_destroy": (None, [V]),
        "crh_font_get_metrics": (C.c_int, [V, C.POINTER(FontMetricsC)]),
        "crh_font_glyph_index": (C.c_int, [V, C.c_uint32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)]),
        "crh_font_glyph_advance": (C.c_int, [V, C.c_uint16, C.c_uint32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)]),
        "crh_font_glyph_bounding_box": (C.c_int, [V, C.c_uint16, C.POINTER(C.c_int16), C.POINTER(C.c_uint32)]),
        "crh_font_glyphs_kerning": (C.c_int, [V, C.c_uint16, C.c_uint16, C.POINTER(C.c_int16), C.POINTER(C.c_uint32)]),
        "crh_paths_of_glyph": (C.c_int, [V, C.c_uint16, C.POINTER(V)]),
        "crh_paths_of_text": (C.c_int, [V, C.POINTER(TextLayoutC), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_float), C.c_size_t, C.POINTER(V)]),
        "crh_text_aligned_positions": (C.c_int, [V, C.POINTER(TextLayoutC), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "crh_path_elliptical_arc": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_uint32, C.c_uint32, C.POINTER(C.c_float),
                                              C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "crh_path_list_transform": (C.c_int, [V, C.c_float, C.POINTER(C.c_float)]),
        "crh_path_list_view": (C.c_int, [V, C.POINTER(PathBatchC)]),
        "crh_path_list_destroy": (None, [V]),
        "crh_last_error": (C.c_char_p, []),
        "crh_version": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here == a symbol of include/contrast_hip.h is not exported
        fn.restype = res
        fn.argtypes = args
    lib._crh_signatures = sig
    _lib = lib
    return lib


class ContrastError(RuntimeError):
    """Mirrors contrast_renderer::error::Error (error.rs:5-16) plus the panics surfaced as codes."""

    def __init__(self, status, detail=""):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}{(': ' + detail) if detail else ''}")


def check(status):
    if status != OK:
        detail = ""
        if status == ERR_HIP and _lib is not None:
            detail = (_lib.crh_last_error() or b"").decode()
        raise ContrastError(status, detail)
