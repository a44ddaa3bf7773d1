"""The refusals of the image API (csrc/image.hip) as one literal table, without a device: the call, the status it returns and, where the library
sets one, the exact text of crh_last_error(). Every row returns before the first HIP call. The table holds what the filters' own CPU tests
(tests/test_<filter>_cpu.py) leave out: the seven crh_image_<filter> calls with a null source (or renderer) and with a null `out`, the messages
that only a device entry point produces, and which of two faults a call names when both are present."""
import ctypes as C

import pytest

from contrast_renderer_amd import _ffi

OK, NON_FINITE, UNSUPPORTED, INVALID = _ffi.OK, _ffi.ERR_NON_FINITE, _ffi.ERR_UNSUPPORTED, _ffi.ERR_INVALID_ARGUMENT
NAN = float("nan")


class ImageHead(C.Structure):
    """What a crh_image starts with: its renderer and its size. Enough for the calls below, which refuse before they look at the texels or
    at the renderer behind the pointer (0x10 and 0x20 are never followed)."""
    _fields_ = [("renderer", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("pixels", C.c_void_p * 2)]


def image(width=5, height=3, renderer=0x10):
    return C.addressof(_keep(ImageHead(renderer, width, height)))


_kept = []


def _keep(value):
    _kept.append(value)
    return value


def convolve(**changes):
    fields = dict(order_x=1, order_y=1, target_x=0, target_y=0, kernel=_keep((C.c_float * 1)(1.0)), divisor=1.0, bias=0.0, edge=1, preserve_alpha=0)
    fields.update(changes)
    fields["kernel"] = C.cast(fields["kernel"], C.POINTER(C.c_float))
    return C.pointer(_keep(_ffi.ConvolveC(**fields)))


def lighting(**changes):
    fields = dict(op=0, light=0, edge=1, surface_scale=1.0, constant=1.0, specular_exponent=1.0, color=(C.c_float * 3)(1.0, 1.0, 1.0), azimuth=30.0, elevation=40.0)
    fields.update(changes)
    return C.pointer(_keep(_ffi.LightingC(**fields)))


def turbulence(**changes):
    fields = dict(kind=1, octaves=1, seed=0, stitch=0, opaque=0, base_frequency=(C.c_float * 2)(0.1, 0.1), offset=(C.c_float * 2)(0.0, 0.0))
    fields.update(changes)
    return C.pointer(_keep(_ffi.TurbulenceC(**fields)))


def composite(op=3, mode=0, opacity=1.0):
    return C.pointer(_keep(_ffi.CompositeC(op, mode, opacity, 0, 0)))


OUT = C.pointer(_keep(C.c_void_p(0x1234)))  # a refused call leaves it as it is
TEXELS, RESULT = _keep((C.c_uint8 * 64)()), _keep((C.c_uint8 * 64)())
IN, TO = C.addressof(TEXELS), C.addressof(RESULT)
W, H = C.pointer(_keep(C.c_uint32(7))), C.pointer(_keep(C.c_uint32(9)))
LATTICE, GRADIENT = _keep((C.c_uint8 * 256)()), _keep((C.c_double * 2048)())
TOO_LARGE = _keep((C.c_float * 20)(*([17.0] + [0.0] * 19)))
NOT_FINITE = _keep((C.c_float * 20)(*([NAN] + [0.0] * 19)))
BLUR, SIZE, CONVOLVE, LIGHTING, TURBULENCE = "crh_blur_taps: ", "crh_morphology_size: ", "crh_convolve_validate: ", "crh_lighting_validate: ", "crh_turbulence_validate: "
A_SIZE = "width and height lie in [1, 16384]"

# (the entry point, its arguments, the status, the text of crh_last_error() or None where the call sets none)
CONTRACT = [
    # ---- blur: null arguments and the edge are refused without a text; the sigmas in order, x before y; then the size of the result
    ("crh_image_blur", (None, 1.0, 1.0, 0, OUT), INVALID, None),
    ("crh_image_blur", (image(renderer=None), 1.0, 1.0, 0, OUT), INVALID, None),
    ("crh_image_blur", (image(), 1.0, 1.0, 0, None), INVALID, None),
    ("crh_image_blur", (image(), 1.0, 1.0, 4, OUT), INVALID, None),
    ("crh_image_blur", (image(), NAN, 1.0, 0, OUT), NON_FINITE, None),
    ("crh_image_blur", (image(), 1.0, -float("inf"), 0, OUT), NON_FINITE, None),
    ("crh_image_blur", (image(), -1.0, 1.0, 0, OUT), INVALID, BLUR + "sigma is negative"),
    ("crh_image_blur", (image(), 1.0, 64.5, 0, OUT), INVALID, BLUR + "sigma exceeds CRH_MAX_BLUR_SIGMA"),
    ("crh_image_blur", (image(), -1.0, NAN, 0, OUT), INVALID, BLUR + "sigma is negative"),
    ("crh_image_blur", (image(), 65.0, -1.0, 0, OUT), INVALID, BLUR + "sigma exceeds CRH_MAX_BLUR_SIGMA"),
    ("crh_image_blur", (image(16384, 1), 64.0, 0.0, 0, OUT), UNSUPPORTED, "crh_image_blur: a side of the grown result exceeds 16384"),
    ("crh_image_blur", (image(1, 16001), 0.0, 64.0, 0, OUT), UNSUPPORTED, "crh_image_blur: a side of the grown result exceeds 16384"),
    ("crh_blur_taps", (NAN, None, 0, None), NON_FINITE, None),
    # ---- composite: null arguments without a text, then `how`, then the two renderers
    ("crh_image_composite", (None, image(), composite(), OUT), INVALID, None),
    ("crh_image_composite", (image(renderer=None), image(), composite(), OUT), INVALID, None),
    ("crh_image_composite", (image(), None, composite(), OUT), INVALID, None),
    ("crh_image_composite", (image(), image(), None, OUT), INVALID, None),
    ("crh_image_composite", (image(), image(), composite(), None), INVALID, None),
    ("crh_image_composite", (image(), image(), composite(op=13), OUT), INVALID, "crh_composite_validate: op is above CRH_COMPOSITE_PLUS"),
    ("crh_image_composite", (image(), image(), composite(op=13, mode=9), OUT), INVALID, "crh_composite_validate: op is above CRH_COMPOSITE_PLUS"),
    ("crh_image_composite", (image(), image(), composite(mode=9, opacity=NAN), OUT), INVALID, "crh_composite_validate: mode is above CRH_BLEND_EXCLUSION"),
    ("crh_image_composite", (image(), image(), composite(opacity=NAN), OUT), NON_FINITE, None),
    ("crh_image_composite", (image(), image(), composite(opacity=1.5), OUT), INVALID, "crh_composite_validate: opacity is outside [0, 1]"),
    ("crh_image_composite", (image(), image(renderer=0x20), composite(), OUT), INVALID, "crh_image_composite: the images belong to different renderers"),
    ("crh_image_composite", (image(), image(renderer=0x20), composite(mode=9), OUT), INVALID, "crh_composite_validate: mode is above CRH_BLEND_EXCLUSION"),
    # ---- colour filter: null arguments without a text, then the matrix (a non-finite entry before one that is too large)
    ("crh_image_color_filter", (None, None, None, OUT), INVALID, None),
    ("crh_image_color_filter", (image(renderer=None), None, None, OUT), INVALID, None),
    ("crh_image_color_filter", (image(), None, None, None), INVALID, None),
    ("crh_image_color_filter", (image(), NOT_FINITE, None, OUT), NON_FINITE, None),
    ("crh_image_color_filter", (image(), TOO_LARGE, None, OUT), INVALID, "crh_color_filter_validate: a coefficient is outside [-CRH_COLOR_MATRIX_MAX, CRH_COLOR_MATRIX_MAX]"),
    # ---- morphology: a null argument, then the size before the op before the edge before the radii
    ("crh_image_morphology", (None, 1, 1, 1, 1, OUT), INVALID, SIZE + "a null argument"),
    ("crh_image_morphology", (image(renderer=None), 1, 1, 1, 1, OUT), INVALID, SIZE + "a null argument"),
    ("crh_image_morphology", (image(), 1, 1, 1, 1, None), INVALID, SIZE + "a null argument"),
    ("crh_image_morphology", (image(0, 3), 2, 193, 1, 4, OUT), INVALID, SIZE + A_SIZE),
    ("crh_image_morphology", (image(), 2, 193, 1, 4, OUT), INVALID, SIZE + "op is above CRH_MORPHOLOGY_DILATE"),
    ("crh_image_morphology", (image(), 1, 193, 1, 4, OUT), INVALID, SIZE + "edge is above CRH_BLUR_EDGE_REFLECT"),
    ("crh_image_morphology", (image(), 1, 193, 1, 3, OUT), INVALID, SIZE + "a radius exceeds CRH_MAX_MORPHOLOGY_RADIUS"),
    ("crh_image_morphology", (image(16384, 1), 1, 1, 0, 0, OUT), UNSUPPORTED, SIZE + "a side of the grown result exceeds 16384"),
    ("crh_morphology_size", (0, 3, 2, 193, 1, 4, W, H), INVALID, SIZE + A_SIZE),
    ("crh_morphology_size", (5, 3, 2, 193, 1, 4, W, H), INVALID, SIZE + "op is above CRH_MORPHOLOGY_DILATE"),
    ("crh_morphology_size", (5, 3, 1, 193, 1, 4, W, H), INVALID, SIZE + "edge is above CRH_BLUR_EDGE_REFLECT"),
    ("crh_morphology_size", (0, 3, 2, 1, 1, 1, None, H), INVALID, SIZE + "a null argument"),
    ("crh_morphology_texels", (5, 3, None, 1, 1, 1, 1, None), INVALID, SIZE + "a null argument"),  # (both null: also out_rgba8 == rgba8)
    ("crh_morphology_texels", (0, 3, IN, 2, 1, 1, 1, IN), INVALID, SIZE + "out_rgba8 is rgba8"),
    # ---- convolve: a null argument, then `how` before the size
    ("crh_image_convolve", (None, convolve(), OUT), INVALID, CONVOLVE + "a null argument"),
    ("crh_image_convolve", (image(renderer=None), convolve(), OUT), INVALID, CONVOLVE + "a null argument"),
    ("crh_image_convolve", (image(), convolve(), None), INVALID, CONVOLVE + "a null argument"),
    ("crh_image_convolve", (image(), None, OUT), INVALID, CONVOLVE + "a null argument"),
    ("crh_image_convolve", (image(0, 3), convolve(divisor=0.0), OUT), INVALID, CONVOLVE + "divisor is 0"),
    ("crh_image_convolve", (image(0, 3), convolve(), OUT), INVALID, CONVOLVE + A_SIZE),
    ("crh_image_convolve", (image(5, 16385), convolve(divisor=NAN), OUT), NON_FINITE, None),
    ("crh_convolve_texels", (0, 3, IN, convolve(edge=4), TO), INVALID, CONVOLVE + "edge is above CRH_BLUR_EDGE_REFLECT"),
    ("crh_convolve_texels", (5, 3, None, convolve(), None), INVALID, CONVOLVE + "a null argument"),  # (both null: also out_rgba8 == rgba8)
    ("crh_convolve_texels", (0, 3, IN, convolve(edge=4), IN), INVALID, CONVOLVE + "out_rgba8 is rgba8"),
    ("crh_convolve_validate", (convolve(order_x=0, target_x=9, edge=4, preserve_alpha=2, divisor=0.0, bias=2.0),), INVALID, CONVOLVE + "an order is outside [1, CRH_MAX_CONVOLVE_ORDER]"),
    ("crh_convolve_validate", (convolve(target_x=9, edge=4, preserve_alpha=2, divisor=0.0, bias=2.0),), INVALID, CONVOLVE + "a target is not below its order"),
    ("crh_convolve_validate", (convolve(edge=4, preserve_alpha=2, divisor=0.0, bias=2.0),), INVALID, CONVOLVE + "edge is above CRH_BLUR_EDGE_REFLECT"),
    ("crh_convolve_validate", (convolve(preserve_alpha=2, divisor=0.0, bias=2.0),), INVALID, CONVOLVE + "preserve_alpha is above 1"),
    ("crh_convolve_validate", (convolve(divisor=0.0, bias=2.0),), INVALID, CONVOLVE + "divisor is 0"),
    ("crh_convolve_validate", (convolve(divisor=NAN, bias=2.0),), INVALID, CONVOLVE + "bias is outside [-1, 1]"),
    # ---- lighting: a null argument, then `how` before the size
    ("crh_image_lighting", (None, lighting(), OUT), INVALID, LIGHTING + "a null argument"),
    ("crh_image_lighting", (image(renderer=None), lighting(), OUT), INVALID, LIGHTING + "a null argument"),
    ("crh_image_lighting", (image(), lighting(), None), INVALID, LIGHTING + "a null argument"),
    ("crh_image_lighting", (image(), None, OUT), INVALID, LIGHTING + "a null argument"),
    ("crh_image_lighting", (image(0, 3), lighting(op=2), OUT), INVALID, LIGHTING + "op is above CRH_LIGHTING_SPECULAR"),
    ("crh_image_lighting", (image(0, 3), lighting(), OUT), INVALID, LIGHTING + A_SIZE),
    ("crh_image_lighting", (image(16385, 3), lighting(constant=NAN), OUT), NON_FINITE, None),
    ("crh_lighting_texels", (3, 0, IN, lighting(constant=300.0), TO), INVALID, LIGHTING + "constant is outside [0, 256]"),
    ("crh_lighting_texels", (3, 2, None, lighting(), None), INVALID, LIGHTING + "a null argument"),  # (both null: also out_rgba8 == rgba8)
    ("crh_lighting_texels", (3, 0, IN, lighting(op=2), IN), INVALID, LIGHTING + "out_rgba8 is rgba8"),
    ("crh_lighting_validate", (lighting(op=2, light=3, edge=4, surface_scale=NAN),), INVALID, LIGHTING + "op is above CRH_LIGHTING_SPECULAR"),
    ("crh_lighting_validate", (lighting(light=3, edge=4, surface_scale=NAN),), INVALID, LIGHTING + "light is above CRH_LIGHT_SPOT"),
    ("crh_lighting_validate", (lighting(edge=4, surface_scale=NAN),), INVALID, LIGHTING + "edge is above CRH_BLUR_EDGE_REFLECT"),
    ("crh_lighting_validate", (lighting(surface_scale=300.0, constant=NAN),), NON_FINITE, None),
    # ---- turbulence: a null argument, then the fields before the size
    ("crh_image_turbulence", (None, 5, 3, turbulence(), OUT), INVALID, TURBULENCE + "a null argument"),
    ("crh_image_turbulence", (0x10, 5, 3, turbulence(), None), INVALID, TURBULENCE + "a null argument"),
    ("crh_image_turbulence", (0x10, 5, 3, None, OUT), INVALID, TURBULENCE + "a null argument"),
    ("crh_image_turbulence", (0x10, 0, 3, turbulence(kind=2), OUT), INVALID, TURBULENCE + "kind is above CRH_TURBULENCE_TURBULENCE"),
    ("crh_image_turbulence", (0x10, 0, 3, turbulence(offset=(C.c_float * 2)(NAN, 0.0)), OUT), NON_FINITE, TURBULENCE + "a frequency or an offset is not finite"),
    ("crh_image_turbulence", (0x10, 0, 3, turbulence(), OUT), INVALID, TURBULENCE + A_SIZE),
    ("crh_image_turbulence", (0x10, 5, 16385, turbulence(), OUT), INVALID, TURBULENCE + A_SIZE),
    ("crh_turbulence_texels", (0, 3, turbulence(stitch=2), TO), INVALID, TURBULENCE + "stitch is neither 0 nor 1"),
    ("crh_turbulence_texels", (0, 3, turbulence(stitch=2), None), INVALID, TURBULENCE + "a null argument"),
    ("crh_turbulence_tables", (1, None, GRADIENT), INVALID, TURBULENCE + "a null argument"),
    ("crh_turbulence_tables", (1, LATTICE, None), INVALID, TURBULENCE + "a null argument"),
    # ---- the image itself
    ("crh_image_create", (None, 5, 3, IN, OUT), INVALID, None),
    ("crh_image_create", (0x10, 5, 3, None, OUT), INVALID, None),
    ("crh_image_create", (0x10, 5, 3, IN, None), INVALID, None),
    ("crh_image_create", (0x10, 0, 3, IN, OUT), INVALID, None),
    ("crh_image_create", (0x10, 5, 16385, IN, OUT), INVALID, None),
    ("crh_image_size", (None, W, H), INVALID, None),
    ("crh_image_size", (image(), None, H), INVALID, None),
    ("crh_image_size", (image(), W, None), INVALID, None),
    ("crh_image_generate_mipmaps", (None,), INVALID, None),
    ("crh_image_generate_mipmaps", (image(renderer=None),), INVALID, None),
    ("crh_image_level_count", (None, W), INVALID, None),
    ("crh_image_level_count", (image(), None), INVALID, None),
    ("crh_image_download_level", (None, 0, TO, W, H), INVALID, None),
    ("crh_image_download_level", (image(renderer=None), 0, TO, W, H), INVALID, None),
]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def test_the_table_names_every_filter_with_a_null_source_and_a_null_out():
    calls = {name for name, _, _, _ in CONTRACT}
    filters = {f"crh_image_{f}" for f in ("blur", "composite", "color_filter", "morphology", "convolve", "lighting", "turbulence")}
    assert filters <= calls
    for name in filters:
        rows = [args for n, args, _, _ in CONTRACT if n == name]
        assert any(args[0] is None for args in rows) and any(args[-1] is None for args in rows), name


@pytest.mark.parametrize("row", range(len(CONTRACT)), ids=[f"{i}-{row[0]}" for i, row in enumerate(CONTRACT)])
def test_the_call_returns_the_status_and_sets_the_text(lib, row):
    name, args, status, text = CONTRACT[row]
    # some other text first, so that the one asserted below is this call's
    if text is not None and text.startswith(TURBULENCE):
        assert lib.crh_blur_taps(-1.0, None, 0, None) == INVALID
    else:
        assert lib.crh_turbulence_validate(None) == INVALID
    before = lib.crh_last_error().decode()
    assert getattr(lib, name)(*args) == status
    if text is not None:
        assert before != text and lib.crh_last_error().decode() == text
    assert OUT.contents.value == 0x1234 and (W.contents.value, H.contents.value) == (7, 9) and not any(RESULT)


def test_the_structs_the_table_changes_are_valid_as_they_stand(lib):
    """So that a row's refusal is owed to the change it names."""
    assert lib.crh_convolve_validate(convolve()) == OK and lib.crh_lighting_validate(lighting()) == OK and lib.crh_turbulence_validate(turbulence()) == OK
    assert lib.crh_composite_validate(composite()) == OK
    w, h = C.c_uint32(), C.c_uint32()
    assert lib.crh_image_size(image(5, 3), C.byref(w), C.byref(h)) == OK and (w.value, h.value) == (5, 3)  # (ImageHead is a crh_image's head)
