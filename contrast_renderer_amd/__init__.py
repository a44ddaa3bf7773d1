"""contrast_renderer_amd — MI355X-native (gfx950, HIP) tessellate + tile-raster hot path behind
contrast_renderer's Path / Shape / Renderer API. See DESIGN.md and include/contrast_hip.h.

The product is libcontrast_hip.so (hand-written HIP kernels + C ABI). This package is the host-side mirror of
the reference's interface; it has no CPU fallback and never imports the oracle.
"""
from ._ffi import ContrastError, PathBatch  # noqa: F401
from .path import (Cap, CurveApproximation, DashInterval, DynamicStrokeOptions, Join, Path, SegmentType, StrokeOptions,  # noqa: F401
                   batch_from_shapes)
from .renderer import (BlendMode, BlurEdge, ColorMatrix, CompositeOp, ConvolveKernel, DistantLight, Filter, GradientStop, Image, ImagePaint, LightingOp,  # noqa: F401
                       MorphologyOp, Paint, PointLight, SpotLight, Spread, blur_taps, color_filter_texels, composite_texels, convolve_coefficients, convolve_texels,
                       lighting_texels, morphology_size, morphology_texels, TurbulenceKind, turbulence_tables, turbulence_texels, Channel, displace_offset, displace_texels,
                       DistanceMode, distance_code, distance_size, distance_texels, ResizeFilter, resize_taps, resize_texels, ImageStatistics, crop_texels, statistics_texels,
                       variable_blur_sigma, variable_blur_texels, TransformFilter, transform_fit, transform_position, transform_texels)

__all__ = ["ContrastError", "PathBatch", "Cap", "CurveApproximation", "DashInterval", "DynamicStrokeOptions", "Join", "Path", "SegmentType",
           "StrokeOptions", "batch_from_shapes", "GradientStop", "Paint", "Spread", "Filter", "Image", "ImagePaint", "BlurEdge", "blur_taps",
           "CompositeOp", "BlendMode", "composite_texels", "ColorMatrix", "color_filter_texels", "MorphologyOp", "morphology_size", "morphology_texels",
           "ConvolveKernel", "convolve_coefficients", "convolve_texels", "LightingOp", "DistantLight", "PointLight", "SpotLight", "lighting_texels",
           "TurbulenceKind", "turbulence_tables", "turbulence_texels",
           "Channel", "displace_offset", "displace_texels",
           "DistanceMode", "distance_code", "distance_size", "distance_texels",
           "ResizeFilter", "resize_taps", "resize_texels",
           "ImageStatistics", "crop_texels", "statistics_texels",
           "variable_blur_sigma", "variable_blur_texels",
           "TransformFilter", "transform_fit", "transform_position", "transform_texels"]
