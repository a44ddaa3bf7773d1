"""crh_image_convolve (include/contrast_hip.h) on the GPU: k_image_convolve byte for byte against the numpy model of tests/convolve_model.py —
every size that crosses a tile border, every order, target, edge and alpha mode of the CPU test, both ends of the accumulator — chains on the
device, and the way from a rendered frame through a sharpen to an image paint and back into a frame."""
import ctypes as C

import numpy as np
import pytest

from contrast_renderer_amd import BlurEdge, CompositeOp, ContrastError, ConvolveKernel, Path, _ffi, batch_from_shapes, convolve_texels
from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Filter, Image, ImagePaint

import composite_model as CM
import convolve_model as M
import mip_model
from test_gpu_blending import no_pins, stack  # noqa: F401

pytestmark = pytest.mark.gpu

SIZE = mip_model.SIZE
# k_image_convolve's tile is 64 x 16 texels and its halo order - 1 texels per axis: 14 at order 15, 4 at order 5, 2 at order 3. (1, 1), (1, 7)
# and (7, 1) lie inside one tile; (3, 2) is smaller than the halo of order 15 in both axes, so the staged texels take several wrap periods;
# (64, 16) fills one tile exactly. (300, 70) crosses the fourth tile border in x by 44 texels (more than any halo) and the fourth in y by 6
# (less than the halo of order 15, more than that of order 5); (70, 300) crosses in x by 6 and in y by 12; (67, 31) crosses in x by 3 (less
# than the halo of order 5) and in y by 15 (more than the halo of order 15: the most a 16-row tile allows).
SMALL = [(1, 1), (1, 7), (7, 1), (3, 2), (64, 16)]
LARGE = [(300, 70), (70, 300), (67, 31)]
ORDERS = [(1, 1), (3, 3), (2, 4), (5, 5), (15, 1), (1, 15), (15, 15)]
EDGES = [BlurEdge.Transparent, BlurEdge.Pad, BlurEdge.Repeat, BlurEdge.Reflect]
MODES = (False, True)


def targets_of(order):
    return [(order[0] // 2, order[1] // 2), (0, 0), (order[0] - 1, order[1] - 1)]


@pytest.fixture(scope="module")
def renderer():
    return R.Renderer(R.Configuration(), device=0)


_made = {}


def made_once(key, make):
    if key not in _made:
        _made[key] = make()
        if isinstance(_made[key], np.ndarray):
            _made[key].setflags(write=False)
    return _made[key]


def pixels_of(w, h):
    """Random texels of a size (some colours above their alpha), made once and never written."""
    return made_once((w, h), lambda: M.random_pixels(np.random.RandomState(w + 3 * h), w, h))


def kernel_of(order):
    return made_once(("kernel", order), lambda: M.random_kernel(np.random.RandomState(31 * order[0] + order[1]), *order))


def check(image, expect, source, what):
    assert (image.height, image.width) == expect.shape[:2] and image.origin == source.origin, (what, image.width, image.height, image.origin)
    assert image.levels == 1, what
    got = image.download_level(0)
    bad = (got != expect).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (row, column) {tuple(np.argwhere(bad)[0])}: {got[tuple(np.argwhere(bad)[0])]}, the model {expect[tuple(np.argwhere(bad)[0])]}"


def run_and_check(source, pixels, kernel, divisor, bias, target, edge, mode, what):
    expect = M.convolve(pixels, kernel, divisor, bias, target, int(edge), mode)
    check(source.convolve(kernel, divisor, bias, target, edge, mode), expect, source, what)
    return expect


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
@pytest.mark.parametrize("size", SMALL, ids=[f"{w}x{h}" for w, h in SMALL])
def test_the_convolution_equals_the_model(size, edge, renderer, no_pins):
    """Every order, target and alpha mode of the CPU test."""
    pixels = pixels_of(*size)
    source = Image(renderer, pixels)
    for order in ORDERS:
        kernel, divisor = kernel_of(order)
        for target in targets_of(order):
            for mode in MODES:
                run_and_check(source, pixels, kernel, divisor, 0.1, target, edge, mode, (size, order, target, edge.name, mode))
    assert np.array_equal(source.download_level(0), pixels) and source.levels == 1  # the source is untouched


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
@pytest.mark.parametrize("size", LARGE, ids=[f"{w}x{h}" for w, h in LARGE])
def test_sizes_that_cross_tile_borders(size, edge, renderer, no_pins):
    """Every order and both alpha modes, the three targets in turn."""
    pixels = pixels_of(*size)
    source = Image(renderer, pixels)
    for n, order in enumerate(ORDERS):
        kernel, divisor = kernel_of(order)
        for mode in MODES:
            target = targets_of(order)[(n + int(edge) + int(mode)) % 3]
            run_and_check(source, pixels, kernel, divisor, -0.05, target, edge, mode, (size, order, target, edge.name, mode))
    assert np.array_equal(source.download_level(0), pixels) and source.levels == 1


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
def test_the_widest_index_range(edge, renderer, no_pins):
    """(16384, 2) and (2, 16384): 256 tiles in x, 1024 in y, the largest row and column indices."""
    wide = pixels_of(16384, 2)
    tall = made_once("tall", lambda: np.ascontiguousarray(pixels_of(16384, 2).transpose(1, 0, 2)))
    kernel, divisor = kernel_of((15, 15))
    mode = int(edge) % 2 == 1
    for pixels, what in ((wide, "16384x2"), (tall, "2x16384")):
        source = Image(renderer, pixels)
        run_and_check(source, pixels, kernel, divisor, 0.0, (14, 0) if edge == BlurEdge.Pad else None, edge, mode, (what, edge.name, mode))
        run_and_check(source, pixels, ConvolveKernel.sharpen(0.5), 1.0, 0.0, None, edge, not mode, (what, "sharpen", edge.name))


def test_both_ends_of_the_accumulator(renderer, no_pins):
    white = made_once("white", lambda: np.full((20, 70, 4), 255, dtype=np.uint8))
    source = Image(renderer, white)
    for sign, kernel in ((+1, [[1.0] * 8] * 8), (-1, [[-1.0] * 8] * 8), (+1, [[64.0]]), (-1, [[-64.0]])):
        for edge in EDGES:
            for mode in MODES:
                expect = run_and_check(source, white, kernel, 1.0, float(sign), None, edge, mode, ("extreme", sign, edge.name, mode))
                if edge != BlurEdge.Transparent:
                    assert (expect[..., :3] == (255 if sign > 0 else 0)).all()


def test_a_sparse_and_a_dense_kernel_of_one_order(renderer, no_pins):
    pixels = pixels_of(300, 70)
    source = Image(renderer, pixels)
    dense = [[1.0, 2.0, 1.0], [2.0, -3.0, 2.0], [1.0, 2.0, 1.0]]
    for kernel, divisor, bias in ((ConvolveKernel.sobel_x(), 1.0, 0.5), (ConvolveKernel.sobel_y(), 1.0, 0.5), (ConvolveKernel.laplacian(), 1.0, 0.0), (dense, 9.0, 0.0),
                                  (ConvolveKernel.emboss(), 1.0, 0.0), (ConvolveKernel.box(3), 9.0, 0.0)):
        for edge in EDGES:
            for mode in MODES:
                run_and_check(source, pixels, kernel, divisor, bias, None, edge, mode, (kernel, edge.name, mode))
    # divisor=None: the sum of the entries, or 1 if that is 0
    check(source.convolve(dense), M.convolve(pixels, dense, 9.0), source, "divisor None")
    check(source.convolve(ConvolveKernel.sobel_x(), bias=0.5, preserve_alpha=True), M.convolve(pixels, ConvolveKernel.sobel_x(), 1.0, 0.5, None, M.PAD, True), source, "a sum of 0")


def test_chains_on_the_device(renderer, no_pins):
    pixels = pixels_of(67, 31)
    source = Image(renderer, pixels)
    # a single tap is a translation: under TRANSPARENT, composite COPY onto a transparent backdrop at the stated offset, on the device
    backdrop = Image(renderer, np.zeros_like(pixels))
    order_x, order_y, target = 3, 2, (0, 1)
    for r in range(order_y):
        for c in range(order_x):
            kernel = np.zeros((order_y, order_x), dtype=np.float32)
            kernel[r, c] = 1.0
            offset = (c + target[0] - (order_x - 1), r + target[1] - (order_y - 1))
            moved = source.convolve(kernel, 1.0, 0.0, target, BlurEdge.Transparent)
            placed = backdrop.composite(source, CompositeOp.Copy, offset=offset)
            assert np.array_equal(moved.download_level(0), placed.download_level(0)), (r, c)
            assert np.array_equal(moved.download_level(0), CM.composite(np.zeros_like(pixels), pixels, CM.COPY, CM.NORMAL, 255, *offset)), (r, c)
    # two convolutions one after the other, and only level 0 of a source with mipmaps is read
    chained = Image(renderer, pixels)
    chained.generate_mipmaps()
    first = chained.convolve(ConvolveKernel.box(5), edge=BlurEdge.Reflect)
    second = first.convolve(ConvolveKernel.sharpen(1.0), edge=BlurEdge.Reflect, preserve_alpha=True)
    model = M.convolve(M.convolve(pixels, ConvolveKernel.box(5), 25.0, 0.0, None, M.REFLECT, False), ConvolveKernel.sharpen(1.0), 1.0, 0.0, None, M.REFLECT, True)
    check(second, model, chained, "box then sharpen")
    # the result is an image like any other: mipmaps, blur, morphology and the colour filter work on it
    second.generate_mipmaps()
    chain = mip_model.chain(model)
    assert second.levels == len(chain) and all(np.array_equal(second.download_level(l), v) for l, v in enumerate(chain))
    assert first.blur(1.0).levels == 1 and first.dilate(1).width == 69 and first.color_filter().width == 67
    # convolve -> Frame.load_image -> download
    frame = R.Frame(renderer, 67, 31)
    frame.load_image(first)
    assert np.array_equal(frame.download(), M.convolve(pixels, ConvolveKernel.box(5), 25.0, 0.0, None, M.REFLECT, False))


def _minified(r, image):
    """One rectangle over a frame of half the image's size, the image drawn at half scale with trilinear minification."""
    w, h = image.width // 2, image.height // 2
    scene = R.Scene(r, batch_from_shapes([([], [Path.from_rect((w / 2.0, h / 2.0), (w / 2.0, h / 2.0))])]))
    t = np.zeros(16, dtype=np.float32)
    t[0], t[5], t[10], t[15], t[12], t[13] = 2.0 / w, -2.0 / h, 1.0, 1.0, -1.0, 1.0
    scene.set_paints([ImagePaint(image, (2.0, 0.0, 0.0, 0.0, 2.0, 0.0), Filter.LinearMipmap)], [0])
    frame = R.Frame(r, w, h)
    frame.clear()
    scene.render(frame, t.reshape(1, 16), np.float32([(1.0, 1.0, 1.0, 1.0)]))
    return frame.download()


def test_a_snapshot_is_sharpened_and_drawn_as_an_image_paint(no_pins):
    """snapshot of a drawn frame -> convolve (sharpen) -> generate_mipmaps -> image paint -> frame, against the same chain with the host
    function (crh_convolve_texels) in the middle; and the sharpened snapshot against the model."""
    r = R.Renderer(R.Configuration(), device=0)
    shapes, transforms, colours, _ = stack(seed=7, size=SIZE, n=12, radius=(16, 36))
    scene = R.Scene(r, batch_from_shapes(shapes))
    source = R.Frame(r, SIZE, SIZE)
    source.clear()
    scene.render(source, transforms, colours)
    drawn = source.download()
    assert (drawn[..., 3] > 0).mean() > 0.3
    snapshot = Image.from_frame(source)
    sharpen = ConvolveKernel.sharpen(1.0)
    on_device = snapshot.convolve(sharpen, edge=BlurEdge.Pad, preserve_alpha=True)
    host = convolve_texels(drawn, sharpen, edge=BlurEdge.Pad, preserve_alpha=True)
    check(on_device, M.convolve(drawn, sharpen, 1.0, 0.0, None, M.PAD, True), snapshot, "the sharpened snapshot")
    assert np.array_equal(host, on_device.download_level(0)) and not np.array_equal(host, drawn)
    on_host = Image(r, host)
    on_device.generate_mipmaps()
    on_host.generate_mipmaps()
    got, expect = _minified(r, on_device), _minified(r, on_host)
    assert np.array_equal(got, expect) and (got[..., 3] > 0).mean() > 0.3


def test_the_convolution_refuses_what_it_cannot_do(renderer, no_pins):
    lib = _ffi.load_library()
    pixels = pixels_of(7, 1)
    source = Image(renderer, pixels)
    out = C.c_void_p(0x1234)
    values = (C.c_float * 3)(0.0, 1.0, 0.0)

    def how_of(order=(3, 1), target=(1, 0), kernel=values, divisor=1.0, bias=0.0, edge=1, preserve_alpha=0):
        return _ffi.ConvolveC(order[0], order[1], target[0], target[1], C.cast(kernel, C.POINTER(C.c_float)) if kernel is not None else None, divisor, bias, edge, preserve_alpha)

    good = how_of()
    assert lib.crh_image_convolve(None, C.byref(good), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_convolve(source.handle, None, C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234
    assert lib.crh_image_convolve(source.handle, C.byref(good), None) == _ffi.ERR_INVALID_ARGUMENT
    for how, text in ((how_of(order=(16, 1)), "an order is outside [1, CRH_MAX_CONVOLVE_ORDER]"), (how_of(order=(3, 0)), "an order is outside [1, CRH_MAX_CONVOLVE_ORDER]"),
                      (how_of(target=(3, 0)), "a target is not below its order"), (how_of(divisor=0.0), "divisor is 0"), (how_of(bias=1.5), "bias is outside [-1, 1]"),
                      (how_of(edge=4), "edge is above CRH_BLUR_EDGE_REFLECT"), (how_of(preserve_alpha=2), "preserve_alpha is above 1"), (how_of(kernel=None), "a null argument"),
                      (how_of(divisor=1.0 / 65.0), "the kernel over the divisor exceeds CRH_CONVOLVE_MAX_GAIN: sum |k| is above 64 * 65536")):
        assert lib.crh_image_convolve(source.handle, C.byref(how), C.byref(out)) == _ffi.ERR_INVALID_ARGUMENT and out.value == 0x1234, text
        assert lib.crh_last_error().decode() == "crh_convolve_validate: " + text
    assert lib.crh_image_convolve(source.handle, C.byref(how_of(divisor=float("nan"))), C.byref(out)) == _ffi.ERR_NON_FINITE and out.value == 0x1234
    with pytest.raises(ContrastError):
        source.convolve([[1.0]], edge=4)
    with pytest.raises(ContrastError):
        source.convolve(np.ones((1, 16)))
    check(source.convolve(np.full((15, 15), 64.0 / 225.0), 1.0, -1.0, (14, 14), BlurEdge.Reflect, True),
          M.convolve(pixels, np.full((15, 15), 64.0 / 225.0), 1.0, -1.0, (14, 14), M.REFLECT, True), source, "the limits themselves")
    assert np.array_equal(source.download_level(0), pixels)
