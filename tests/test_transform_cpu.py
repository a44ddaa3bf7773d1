"""crh_image_transform without a GPU (include/contrast_hip.h states the rule): crh_transform_texels and the Python mirror byte for byte
against the numpy model of tests/transform_model.py over filter x edge x the matrices of the device test, crh_transform_position
against the model, the cubic table's bounds, the rule's consequences with the host rule, crh_transform_fit against an independent
computation, the refused calls with their statuses, texts and order, the mirrors' enums, a C++ harness, and the rule as a stand-alone
program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, ContrastError, TransformFilter, _ffi, crop_texels, transform_fit, transform_position, transform_texels

import transform_model as M
from test_image_api_contract_cpu import ImageHead

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crh_transform_validate", "crh_transform_fit", "crh_transform_position", "crh_transform_texels", "crh_image_transform")
PREFIX = "crh_transform_validate: "
OK, INVALID, NON_FINITE = _ffi.OK, _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_NON_FINITE
IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1)
# (source size, result size): the same, a smaller result, a larger one, one-texel axes
SIZES = (((33, 15), (33, 15)), ((23, 37), (9, 5)), ((9, 5), (40, 21)), ((1, 7), (7, 1)), ((1, 1), (5, 4)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    return _ffi.load_library()


def how_of(matrix=IDENTITY, width=4, height=3, filter=1, edge=0):
    return _ffi.TransformC((C.c_double * 9)(*matrix), width, height, filter, edge)


def test_the_symbols_are_exported(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    assert C.sizeof(_ffi.TransformC) == 88


@pytest.mark.parametrize("sizes", SIZES, ids=[f"{s[0]}x{s[1]}-{r[0]}x{r[1]}" for s, r in SIZES])
@pytest.mark.parametrize("premultiplied", (True, False), ids=("premultiplied", "straight"))
def test_the_host_rule_equals_the_model(lib, sizes, premultiplied):
    (sw, sh), (w, h) = sizes
    src = M.source(sw, sh, 11 + sw, premultiplied)
    seen = set()
    for name, matrix in M.matrices(sw, sh, w, h).items():
        seen |= set(np.unique(M.positions(matrix, w, h)[2]).tolist()) if name == "horizon" else set()
        for filter, edge in itertools.product(M.FILTERS, M.EDGES):
            text = M.first_mismatch(transform_texels(src, matrix, w, h, TransformFilter(filter), BlurEdge(edge)), M.transform(src, matrix, w, h, filter, edge))
            assert text is None, (name, filter, edge, text)
    assert seen == {True, False}  # the horizon crosses every result here: visible and invisible texels both occur


def test_the_c_call_writes_the_same_bytes_at_any_alignment(lib):
    sw, sh, w, h = 9, 4, 11, 6
    src = M.source(sw, sh, 3)
    matrix = M.matrices(sw, sh, w, h)["rotate_30"]
    raw_in, raw_out = (C.c_uint8 * (sw * sh * 4 + 1))(), (C.c_uint8 * (w * h * 4 + 1))()
    C.memmove(C.addressof(raw_in) + 1, src.ctypes.data, sw * sh * 4)
    how = how_of(matrix, w, h, M.CUBIC, M.REFLECT)
    assert lib.crh_transform_texels(sw, sh, C.addressof(raw_in) + 1, C.byref(how), C.addressof(raw_out) + 1) == OK
    assert bytes(raw_out)[1:] == M.transform(src, matrix, w, h, M.CUBIC, M.REFLECT).tobytes()


def test_the_positions_are_the_models(lib):
    """Every texel of small results, among them invisible texels (horizon), both clamps (far: +2^21 in x, -2^21 in y) and a quotient
    that is infinite."""
    w, h = 13, 6
    cases = dict(M.matrices(9, 7, w, h))
    cases["infinite"] = (1, 0, 0, 0, -1, 0, 0, 0, 5e-324)
    cases["largest"] = (2.0 ** 40, 2.0 ** 40, -2.0 ** 40, -2.0 ** 40, 0, 2.0 ** 40, 0, 0, 1)
    position, visible = (C.c_int32 * 2)(), C.c_uint32()
    clamped = set()
    for name, matrix in cases.items():
        X, Y, V = M.positions(matrix, w, h)
        how = how_of(matrix, w, h)
        for j, i in itertools.product(range(h), range(w)):
            assert lib.crh_transform_position(C.byref(how), i, j, position, C.byref(visible)) == OK
            assert (position[0], position[1], visible.value) == (X[j, i], Y[j, i], int(V[j, i])), (name, i, j)
            clamped |= {position[0], position[1]} & {-2 ** 29, 2 ** 29}
        assert transform_position(matrix, w, h, 2, 1) == (X[1, 2], Y[1, 2], bool(V[1, 2]))
    assert clamped == {-2 ** 29, 2 ** 29}
    X, Y, V = M.positions(cases["horizon"], w, h)
    assert V.any() and not V.all()
    assert M.positions(cases["far"], w, h)[0].min() == 2 ** 29 and M.positions(cases["far"], w, h)[1].max() == -2 ** 29
    assert M.positions((1, 0, 0.25, 0, 1, 0, 0, 0, 1), 2, 1)[0].tolist() == [[192, 448]]  # u + 0.25 = 0.75 and 1.75 texels


def test_the_cubic_table_keeps_its_bounds():
    T = M.CUBIC_TABLE
    assert T.min() == -1214 and T.max() == 16384 and (T.sum(axis=1) == 16384).all()
    positive, negative = (T * (T > 0)).sum(axis=1), (T * (T < 0)).sum(axis=1)
    assert positive.max() <= 18432 and negative.min() >= -2048
    h_lo, h_hi = ((255 * negative + 32) >> 6).min(), ((255 * positive + 32) >> 6).max()
    assert -8161 <= h_lo and h_hi <= 73440
    assert (positive * 73440 - negative * 8161).max() + 2 ** 21 <= 1372456960 < 2 ** 31
    assert T[0].tolist() == [0, 16384, 0, 0] and T[128].tolist() == [-1024, 9216, 9216, -1024]
    # a constant image comes back exactly at every phase pair: h = (16384 v + 32) >> 6 = 256 v, then (16384 * 256 v + 2^21) >> 22 = v
    for v in (0, 1, 127, 255):
        h = (T.sum(axis=1) * v + 32) >> 6
        assert ((T.sum(axis=1)[:, None] * h[None, :] + 2 ** 21) >> 22 == v).all()


def test_a_constant_image_comes_back_at_every_phase_pair(lib):
    flat = np.empty((6, 6, 4), dtype=np.uint8)
    flat[:] = (7, 1, 201, 201)
    for fy in range(0, 256, 5):
        matrix = (1 / 256, 0, 2.0, 0, 0, 2 + fy / 256, 0, 0, 1)  # a row of 256 texels walks through every x phase at the y phase fy
        got = transform_texels(flat, matrix, 256, 1, TransformFilter.Cubic, BlurEdge.Pad)
        assert (got == np.array((7, 1, 201, 201), dtype=np.uint8)).all(), fy


@pytest.mark.parametrize("premultiplied", (True, False), ids=("premultiplied", "straight"))
def test_the_consequences(lib, premultiplied):
    sw, sh = 19, 11
    src = M.source(sw, sh, 5, premultiplied)
    clamped = src.copy()
    clamped[..., :3] = np.minimum(src[..., :3], src[..., 3:])
    for edge in BlurEdge:
        # the identity is a copy; under CUBIC of min(rgb, a)
        assert np.array_equal(transform_texels(src, IDENTITY, sw, sh, TransformFilter.Nearest, edge), src)
        assert np.array_equal(transform_texels(src, IDENTITY, sw, sh, TransformFilter.Linear, edge), src)
        assert np.array_equal(transform_texels(src, IDENTITY, sw, sh, TransformFilter.Cubic, edge), clamped)
        for filter in TransformFilter:
            want = clamped if filter == TransformFilter.Cubic else src
            # the quarter turns are np.rot90's permutations (k counts counter-clockwise turns of the array)
            turns = M.matrices(sw, sh, sh, sw)
            assert np.array_equal(transform_texels(src, turns["turn_90"], sh, sw, filter, edge), np.rot90(want, -1)), (filter, edge)
            assert np.array_equal(transform_texels(src, turns["turn_270"], sh, sw, filter, edge), np.rot90(want, 1)), (filter, edge)
            assert np.array_equal(transform_texels(src, M.matrices(sw, sh, sw, sh)["turn_180"], sw, sh, filter, edge), np.rot90(want, 2)), (filter, edge)
            # an all-zero linear part reads one point
            point = transform_texels(src, (0, 0, 2.5, 0, 0, 1.5, 0, 0, 1), 5, 3, filter, edge)
            assert (point == want[1, 2]).all()
            if premultiplied:  # rgb <= a survives
                for name in ("rotate_30", "scale_2.5", "scale_0.4", "shear", "horizon", "translate_half"):
                    got = transform_texels(src, M.matrices(sw, sh, 25, 17)[name], 25, 17, filter, edge)
                    assert (got[..., :3] <= got[..., 3:]).all(), (name, filter, edge)
    # an integer translation under TRANSPARENT is crop's bytes
    for filter, (x, y, w, h) in itertools.product(TransformFilter, ((3, -2, 19, 11), (-4, 5, 30, 9), (40, 0, 3, 3))):
        want = crop_texels(clamped if filter == TransformFilter.Cubic else src, x, y, w, h)
        assert np.array_equal(transform_texels(src, (1, 0, x, 0, 1, y, 0, 0, 1), w, h, filter, BlurEdge.Transparent), want), (filter, x, y)


def test_fit_a_rotation_by_30_degrees(lib):
    """40 x 25 turned by 30 degrees: the size and the origin from the corners computed here with plain trigonometry, the model's
    matrix bit for bit, and every source texel centre inside the result."""
    sw, sh = 40, 25
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    forward = (c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0)
    matrix, (w, h), origin = transform_fit(sw, sh, forward)
    xs = [c * x - s * y for x, y in ((0, 0), (sw, 0), (0, sh), (sw, sh))]
    ys = [s * x + c * y for x, y in ((0, 0), (sw, 0), (0, sh), (sw, sh))]
    assert (w, h) == (math.ceil(max(xs)) - math.floor(min(xs)), math.ceil(max(ys)) - math.floor(min(ys))) == (48, 42)
    assert origin == (-math.floor(min(xs)), -math.floor(min(ys))) == (13, 0)
    want, size, want_origin = M.fit(sw, sh, forward)
    assert matrix.reshape(9).tolist() == want and size == (w, h) and want_origin == origin
    assert matrix[2].tolist() == [0.0, 0.0, 1.0]  # an affine forward: the last row exactly, so the call takes the affine path
    j, i = np.mgrid[0:sh, 0:sw] + 0.5
    tx, ty = c * i - s * j + origin[0], s * i + c * j + origin[1]  # a source texel centre in the result
    assert tx.min() >= 0 and tx.max() <= w and ty.min() >= 0 and ty.max() <= h
    # and the result -> source matrix brings that point back to the centre it came from
    back_x, back_y = matrix[0, 0] * tx + matrix[0, 1] * ty + matrix[0, 2], matrix[1, 0] * tx + matrix[1, 1] * ty + matrix[1, 2]
    assert np.abs(back_x - i).max() < 1e-9 and np.abs(back_y - j).max() < 1e-9
    # Image.transform's placement: a fitted NEAREST result holds every texel of an opaque source
    src = M.source(sw, sh, 2)
    src[..., 3] = 255
    assert (transform_texels(src, matrix, w, h, TransformFilter.Nearest)[..., 3] == 255).sum() >= sw * sh * 0.95


def test_fit_other_matrices_and_its_refusals(lib):
    for forward in ((0, -1, 0, 1, 0, 0, 0, 0, 1), (0.75, -0.5, 3, 0.5, 0.75, -1, 0, 0, 1), (2, 0, -7.5, 0, 0.5, 100.25, 0, 0, 1), (-1, 0, 0, 0, 1, 0, 0, 0, 1),
                    (1, 0.2, 0, 0.1, 1, 0, 0.001, 0.002, 1), (1, 0, 0, 0, 1, 0, 0, 0, 2), (1e-3, 0, 0, 0, 1e-3, 0, 0, 0, 1)):
        matrix, size, origin = transform_fit(31, 17, forward)
        want = M.fit(31, 17, forward)
        assert (matrix.reshape(9).tolist(), size, origin) == want, forward
        if forward[6] == 0 and forward[7] == 0 and forward[8] == 1:
            assert matrix[2].tolist() == [0.0, 0.0, 1.0], forward
    assert transform_fit(40, 25, (0, -1, 0, 1, 0, 0))[1:] == ((25, 40), (25, 0))  # six entries: an affine matrix
    out, origin = how_of(width=77, height=78), (C.c_int32 * 2)(-5, -6)
    fwd = lambda *m: (C.c_double * 9)(*m)  # noqa: E731

    def refused(status, code, text):
        assert status == code and lib.crh_last_error().decode() == PREFIX + text, (status, lib.crh_last_error())
        assert (out.width, out.height, list(out.matrix), list(origin)) == (77, 78, list(IDENTITY), [-5, -6])

    refused(lib.crh_transform_fit(4, 4, None, 1, 0, C.byref(out), origin), INVALID, "a null argument")
    refused(lib.crh_transform_fit(4, 4, fwd(*IDENTITY), 1, 0, None, origin), INVALID, "a null argument")
    refused(lib.crh_transform_fit(4, 4, fwd(*IDENTITY), 1, 0, C.byref(out), None), INVALID, "a null argument")
    refused(lib.crh_transform_fit(4, 4, fwd(*IDENTITY), 3, 0, C.byref(out), origin), INVALID, "filter is above CRH_TRANSFORM_CUBIC")
    refused(lib.crh_transform_fit(4, 4, fwd(*IDENTITY), 1, 4, C.byref(out), origin), INVALID, "edge is above CRH_BLUR_EDGE_REFLECT")
    refused(lib.crh_transform_fit(4, 4, fwd(1, 0, float("inf"), 0, 1, 0, 0, 0, 1), 1, 0, C.byref(out), origin), NON_FINITE, "an entry of the matrix is not finite")
    refused(lib.crh_transform_fit(4, 4, fwd(1, 0, 2e12, 0, 1, 0, 0, 0, 1), 1, 0, C.byref(out), origin), INVALID, "an entry of the matrix is above 2^40 in magnitude")
    refused(lib.crh_transform_fit(0, 4, fwd(*IDENTITY), 1, 0, C.byref(out), origin), INVALID, "width and height lie in [1, 16384]")
    refused(lib.crh_transform_fit(4, 4, fwd(1, 2, 0, 2, 4, 0, 0, 0, 1), 1, 0, C.byref(out), origin), INVALID, "forward is singular")
    refused(lib.crh_transform_fit(4, 4, fwd(0, 0, 0, 0, 0, 0, 0, 0, 1), 1, 0, C.byref(out), origin), INVALID, "forward is singular")
    refused(lib.crh_transform_fit(4, 4, fwd(1, 0, 0, 0, 1, 0, -0.25, 0, 1), 1, 0, C.byref(out), origin), INVALID, "a corner is behind the horizon")  # W = 0 at x = 4
    refused(lib.crh_transform_fit(4, 4, fwd(1, 0, 0, 0, 1, 0, 0, 0, -1), 1, 0, C.byref(out), origin), INVALID, "a corner is behind the horizon")
    refused(lib.crh_transform_fit(4, 4, fwd(5000, 0, 0, 0, 1, 0, 0, 0, 1), 1, 0, C.byref(out), origin), INVALID, "the result is outside [1, 16384]")
    refused(lib.crh_transform_fit(4, 4, fwd(1, 0, 0, 0, 1, 0, 0, 0, 1e-300), 1, 0, C.byref(out), origin), INVALID, "the result is outside [1, 16384]")
    refused(lib.crh_transform_fit(4, 4, fwd(1, 0, 2.0 ** 31, 0, 1, 0, 0, 0, 1), 1, 0, C.byref(out), origin), INVALID, "the origin is beyond 2^30")
    assert M.fit(4, 4, (1, 2, 0, 2, 4, 0, 0, 0, 1)) == "forward is singular" and M.fit(4, 4, (1, 0, 0, 0, 1, 0, -0.25, 0, 1)) == "a corner is behind the horizon"
    assert M.fit(4, 4, (5000, 0, 0, 0, 1, 0, 0, 0, 1)) == "the result is outside [1, 16384]"
    assert lib.crh_transform_fit(4, 4, fwd(4096, 0, 0, 0, 1, 0, 0, 0, 1), 1, 0, C.byref(out), origin) == OK and (out.width, out.height) == (16384, 4)
    with pytest.raises(ContrastError):
        transform_fit(4, 4, (1, 2, 0, 2, 4, 0))


def test_the_refusals(lib):
    out = C.c_void_p(0x1234)
    texels, result = (C.c_uint8 * 64)(), (C.c_uint8 * 64)(*([0xAB] * 64))
    IN, TO = C.addressof(texels), C.addressof(result)
    position, visible = (C.c_int32 * 2)(-7, -8), C.c_uint32(9)
    good = how_of()
    # fake image heads, never followed: every call below returns before it looks at the texels or at the renderer behind 0x10
    heads = [ImageHead(0x10, 5, 3), ImageHead(0, 5, 3)]
    src, no_renderer = (C.addressof(head) for head in heads)

    def refused(status, code, text):
        assert status == code, (status, text)
        assert lib.crh_last_error().decode() == PREFIX + text
        assert out.value == 0x1234 and bytes(result) == b"\xAB" * 64 and (position[0], position[1], visible.value) == (-7, -8, 9)

    # 1: a null argument
    refused(lib.crh_transform_validate(None), INVALID, "a null argument")
    for arguments in ((None, 0, 0, position, C.byref(visible)), (C.byref(good), 0, 0, None, C.byref(visible)), (C.byref(good), 0, 0, position, None)):
        refused(lib.crh_transform_position(*arguments), INVALID, "a null argument")
    for arguments in ((2, 2, None, C.byref(good), TO), (2, 2, IN, None, TO), (2, 2, IN, C.byref(good), None)):
        refused(lib.crh_transform_texels(*arguments), INVALID, "a null argument")
    for arguments in ((None, C.byref(good), C.byref(out)), (src, None, C.byref(out)), (src, C.byref(good), None), (no_renderer, C.byref(good), C.byref(out))):
        refused(lib.crh_image_transform(*arguments), INVALID, "a null argument")
    # 2 to 4: the fields, by all four entry points, and the order when two faults are present
    nan, inf, big = float("nan"), float("inf"), 2.0 ** 40 * (1 + 2.0 ** -52)
    entry = lambda k, v: tuple(v if at == k else e for at, e in enumerate(IDENTITY))  # noqa: E731
    fields = [(how_of(filter=3), INVALID, "filter is above CRH_TRANSFORM_CUBIC"), (how_of(edge=4), INVALID, "edge is above CRH_BLUR_EDGE_REFLECT"),
              (how_of(filter=3, edge=4, matrix=entry(0, nan)), INVALID, "filter is above CRH_TRANSFORM_CUBIC"),
              (how_of(edge=9, matrix=entry(0, nan), width=0), INVALID, "edge is above CRH_BLUR_EDGE_REFLECT")]
    fields += [(how_of(matrix=entry(k, v)), NON_FINITE, "an entry of the matrix is not finite") for k in range(9) for v in (nan, inf, -inf)]
    fields += [(how_of(matrix=entry(k, v)), INVALID, "an entry of the matrix is above 2^40 in magnitude") for k in range(9) for v in (big, -big, 1e300)]
    fields += [(how_of(matrix=(big, 0, 0, 0, 1, 0, 0, nan, 1), width=0), NON_FINITE, "an entry of the matrix is not finite"),
               (how_of(matrix=entry(4, -big), width=0), INVALID, "an entry of the matrix is above 2^40 in magnitude")]
    fields += [(how_of(width=w, height=h), INVALID, "width and height lie in [1, 16384]") for w, h in ((0, 2), (2, 0), (16385, 1), (1, 16385))]
    for how, code, text in fields:
        refused(lib.crh_transform_validate(C.byref(how)), code, text)
        refused(lib.crh_transform_position(C.byref(how), 99, 99, position, C.byref(visible)), code, text)
        refused(lib.crh_transform_texels(0, 2, IN, C.byref(how), IN), code, text)
        refused(lib.crh_image_transform(src, C.byref(how), C.byref(out)), code, text)
    for legal in (how_of(entry(2, 2.0 ** 40), 16384, 1, 2, 3), how_of(entry(8, -2.0 ** 40), 1, 16384, 0, 0), how_of((0,) * 9), how_of((1, 2, 0, 2, 4, 0, 0, 0, 1))):
        assert lib.crh_transform_validate(C.byref(legal)) == OK  # the largest entries and sizes; singular matrices
    # then the entry points' own
    refused(lib.crh_transform_position(C.byref(good), 4, 0, position, C.byref(visible)), INVALID, "a texel is outside the result")
    refused(lib.crh_transform_position(C.byref(good), 0, 3, position, C.byref(visible)), INVALID, "a texel is outside the result")
    for w, h in ((0, 2), (2, 0), (16385, 1), (1, 16385)):
        refused(lib.crh_transform_texels(w, h, IN, C.byref(good), IN), INVALID, "width and height lie in [1, 16384]")
    refused(lib.crh_transform_texels(2, 2, TO, C.byref(good), TO), INVALID, "out_rgba8 is rgba8")
    assert lib.crh_transform_texels(2, 2, IN, C.byref(good), TO) == OK and bytes(result)[:48] == bytes(48)
    # the Python mirror
    pixels = np.zeros((2, 2, 4), dtype=np.uint8)
    for bad in (dict(matrix=IDENTITY, width=0, height=1), dict(matrix=entry(3, nan), width=1, height=1), dict(matrix=entry(3, 1e13), width=1, height=1),
                dict(matrix=IDENTITY, width=1, height=1, filter=3), dict(matrix=IDENTITY, width=1, height=1, edge=7), dict(matrix=(1, 2, 3), width=1, height=1)):
        with pytest.raises(ContrastError):
            transform_texels(pixels, **bad)
    with pytest.raises(ContrastError):
        transform_position(IDENTITY, 2, 2, 2, 0)


def test_the_mirrors_name_the_enum_alike():
    assert [(f.name, int(f)) for f in TransformFilter] == [("Nearest", 0), ("Linear", 1), ("Cubic", 2)]
    header = open(os.path.join(ROOT, "include", "contrast_hip.h")).read()
    assert "CRH_TRANSFORM_NEAREST = 0, CRH_TRANSFORM_LINEAR = 1, CRH_TRANSFORM_CUBIC = 2" in header and "#define CRH_MAX_TRANSFORM_ENTRY 1099511627776.0" in header
    cpp = open(os.path.join(ROOT, "include", "contrast_renderer.hpp")).read()
    assert "enum class TransformFilter : uint32_t { Nearest = CRH_TRANSFORM_NEAREST, Linear = CRH_TRANSFORM_LINEAR, Cubic = CRH_TRANSFORM_CUBIC };" in cpp
    rust = open(os.path.join(ROOT, "rust", "contrast_renderer_hip", "src", "lib.rs")).read()
    assert re.search(r"pub enum TransformFilter \{\s*Nearest = 0,\s*Linear = 1,\s*(///[^\n]*\s*)?Cubic = 2,\s*\}", rust)
    for name in ("transform_validate", "transform_fit", "transform_position", "transform_texels"):
        assert f"inline " in cpp and f" {name}(" in cpp and f"pub fn {name}(" in rust, name
    for name in ("resample", "transform", "rotate"):
        assert f"    Image {name}(" in cpp and f"    pub fn {name}(&self" in rust, name
    from contrast_renderer_amd.renderer import MAX_TRANSFORM_ENTRY, Image
    assert MAX_TRANSFORM_ENTRY == 1099511627776.0 and all(hasattr(Image, name) for name in ("resample", "transform", "rotate"))


def test_the_cpp_mirror_compiles_links_and_agrees():
    """tests/cpp/transform_harness.cpp against the C ABI: transform_fit, transform_texels and transform_position of the C++ mirror on an
    image this test writes, compared with the model; its device side is only compiled."""
    lib_dir = os.path.join(ROOT, "contrast_renderer_amd")
    w, h = 19, 7
    src = M.source(w, h, 4)
    with tempfile.TemporaryDirectory() as tmp:
        binary, texels = os.path.join(tmp, "transform_harness"), os.path.join(tmp, "texels.bin")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "transform_harness.cpp"),
               "-o", binary, "-L", lib_dir, "-lcontrast_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        with open(texels, "wb") as f:
            f.write(src.tobytes())
        done = subprocess.run([binary, texels, str(w), str(h)], capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr)
    lines = done.stdout.splitlines()
    assert len(lines) == 7
    matrix, (rw, rh), origin = M.fit(w, h, (0.75, -0.5, 3.0, 0.5, 0.75, -1.0, 0.0, 0.0, 1.0))
    assert lines[0].split() == [str(rw), str(rh), str(origin[0]), str(origin[1])]
    assert [float.fromhex(v) for v in lines[1].split()] == matrix
    for line, filter in zip(lines[2:5], M.FILTERS):
        assert line == M.transform(src, matrix, rw, rh, filter, M.REFLECT).tobytes().hex(), filter
    X, Y, V = M.positions((1, 0, 0, 0, 1, 0, -0.25, 0, 1), 8, 2)
    assert [line.split() for line in lines[5:]] == [[str(X[1, i]), str(Y[1, i]), str(int(V[1, i]))] for i in (1, 6)] and V[1, 1] and not V[1, 6]


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers():
    """A stand-alone program (its own main, no library, nothing loaded into python) around csrc/transform.hpp, the rule that
    crh_transform_texels runs: compiled as host code with the two sanitizers (the flag goes to the host compilation alone) and run
    once. It checks the cubic table's bounds and runs every filter and edge on heap buffers sized exactly."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        binary = os.path.join(tmp, "transform_sanitize")
        # -x c++ and -Xarch_host: plain host C++, the sanitizers on the host alone (no device pass; clang links the sanitizers' runtime statically, so the program needs nothing preloaded)
        cmd = [hipcc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall",
               "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), "-I", os.path.join(ROOT, "contrast_renderer_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "transform_sanitize.cpp"), "-o", binary]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        done = subprocess.run([binary], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert re.search(r"\d+ texels, 0 failures$", done.stdout.strip())
