"""crh_image_variable_blur (include/contrast_hip.h) on the GPU: k_image_variable_blur_h and k_image_variable_blur_v byte for byte against
the numpy model of tests/variable_blur_model.py, with no tolerance and no excluded texel — the sizes at which the kernels can go wrong
under every edge, masks that put every lane on its own level (the per-lane tap loads), masks that are constant along a wave (the
wave-uniform tap loads) and masks in between, the sigma pairs from the identity to radius 192 — then against the existing device blur
for masks of one value, the rule's consequences on the device, the mask as its own source, and a refused call."""
import ctypes as C

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, Channel, ContrastError, _ffi
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Image

import blur_model as B
import variable_blur_model as M
from test_gpu_blending import no_pins  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


@pytest.fixture(scope="module")
def uploaded(renderer):
    """-> image(bytes): an array uploaded once per module and kept"""
    kept = {}

    def image(pixels):
        if id(pixels) not in kept:
            kept[id(pixels)] = (Image(renderer, pixels), pixels)
        return kept[id(pixels)][0]
    return image


def check(image, expect, levels, what):
    assert (image.width, image.height) == (expect.shape[1], expect.shape[0]) and image.origin == (0, 0) and image.levels == 1, (what, image.width, image.height, image.origin)
    got = image.download_level(0)
    text = M.first_mismatch(got, expect, levels)
    assert text is None, f"{what}: {text}"
    return got


def run_case(uploaded, case):
    kind, w, h, pair, edge, channel = case
    sx, sy = M.PAIRS[pair]
    mask = M.mask(kind, w, h)
    result = uploaded(M.source(w, h)).variable_blur(uploaded(mask), (sx[1], sy[1]), (sx[0], sy[0]), Channel(channel), BlurEdge(edge))
    check(result, M.expected(*case), mask[..., channel], case)
    result.destroy()


@pytest.mark.parametrize("size", M.SIZES, ids=[f"{w}x{h}" for w, h in M.SIZES])
def test_every_size_under_every_edge_equals_the_model(size, uploaded, no_pins):
    """Radius 192 beside the identity (ascending on x, descending on y) on a noise mask and on a checkerboard of codes 0 and 255."""
    for case in M.size_cases(*size):
        run_case(uploaded, case)


@pytest.mark.parametrize("kind", M.MASKS)
@pytest.mark.parametrize("size", M.LARGE, ids=[f"{w}x{h}" for w, h in M.LARGE])
def test_every_mask_with_every_sigma_pair_equals_the_model(size, kind, uploaded, no_pins):
    for case in M.mask_cases(kind, *size):
        run_case(uploaded, case)


def test_a_mask_of_one_value_gives_the_device_blur(renderer, uploaded, no_pins):
    """Consequence 1, device against device: no model between them. Under Transparent the blur grows and is cropped back."""
    w, h = 257, 31
    src = M.source(w, h)
    source = uploaded(src)
    for u in (0, 1, 128, 255):
        mask = np.random.RandomState(u).randint(0, 256, (h, w, 4)).astype(np.uint8)
        mask[..., 1] = u
        mask_image = Image(renderer, mask)
        sx, sy = float(M.sigma_of(1.5, 40.0, u)), float(M.sigma_of(40.0, 1.5, u))
        for edge in BlurEdge:
            got = source.variable_blur(mask_image, (40.0, 1.5), (1.5, 40.0), Channel.G, edge)
            blurred = source.blur(sx, sy, edge)
            if edge == BlurEdge.Transparent:
                assert blurred.origin == (B.radius_of(sx), B.radius_of(sy))
                blurred = blurred.crop(blurred.origin[0], blurred.origin[1], w, h)
            check(got, blurred.download_level(0), mask[..., 1], ("the blur", u, edge))


def test_the_consequences_on_the_device(renderer, uploaded, no_pins):
    w, h = 257, 31
    src, checker, noise = M.source(w, h), M.mask("checker", w, h), M.mask("noise", w, h)
    # 2: a texel whose level has sigma 0 on both axes comes back exactly, beside neighbours at radius 192
    for edge in BlurEdge:
        got = uploaded(src).variable_blur(uploaded(checker), 64.0, 0.0, Channel.A, edge).download_level(0)
        sharp = checker[..., 3] == 0
        assert np.array_equal(got[sharp], src[sharp]) and not np.array_equal(got[~sharp], src[~sharp]), edge
    # 3: a constant image comes back exactly under the three same-size edges
    flat = np.empty((h, w, 4), dtype=np.uint8)
    flat[:] = (30, 200, 7, 201)
    for edge in (BlurEdge.Pad, BlurEdge.Repeat, BlurEdge.Reflect):
        assert np.array_equal(Image(renderer, flat).variable_blur(uploaded(noise), (64.0, 9.0), (0.3, 64.0), Channel.R, edge).download_level(0), flat), edge
    # 4: rgb <= a survives
    for edge in BlurEdge:
        got = uploaded(src).variable_blur(uploaded(noise), (13.0, 64.0), (2.0, 0.0), Channel.R, edge).download_level(0)
        assert (got[..., :3] <= got[..., 3:]).all(), edge


def test_the_mask_may_be_the_source_and_neither_is_modified(renderer, no_pins):
    w, h = 65, 33
    src, mask = M.source(w, h).copy(), M.mask("noise", w, h).copy()
    source, mask_image = Image(renderer, src), Image(renderer, mask)
    check(source.variable_blur(source, 5.0, edge=BlurEdge.Reflect), M.variable_blur(src, src, (0.0, 5.0), (0.0, 5.0), 3, M.REFLECT), src[..., 3], "the source as its own mask")
    result = source.variable_blur(mask_image, (4.0, 7.0), 1.0, Channel.R)
    check(result, M.variable_blur(src, mask, (1.0, 4.0), (1.0, 7.0), 0, M.PAD), mask[..., 0], "the defaults")
    assert np.array_equal(source.download_level(0), src) and np.array_equal(mask_image.download_level(0), mask)
    result.generate_mipmaps()
    assert result.levels == 7 and result.download_level(6).shape == (1, 1, 4)


def test_a_mask_of_another_size_is_refused_and_the_renderer_stays_usable(renderer, no_pins):
    lib = _ffi.load_library()
    w, h = 40, 9
    src, mask = M.source(40, 1).repeat(9, axis=0), np.full((h, w, 4), 255, dtype=np.uint8)
    source, small = Image(renderer, src), Image(renderer, mask[:4])
    with pytest.raises(ContrastError) as refused:
        source.variable_blur(small, 3.0)
    assert refused.value.status == _ffi.ERR_INVALID_ARGUMENT and lib.crh_last_error().decode() == "crh_variable_blur_validate: the mask is of another size"
    out = C.c_void_p(0x1234)
    how = _ffi.VariableBlurC((C.c_float * 2)(0.0, 3.0), (C.c_float * 2)(0.0, 3.0), 3, 1)
    assert lib.crh_image_variable_blur(source.handle, small.handle, C.byref(how), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    check(source.variable_blur(Image(renderer, mask), 3.0), B.blur_sigma(src, 3.0, 3.0, B.PAD), mask[..., 3], "a good call after the refused one")
