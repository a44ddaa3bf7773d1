"""k_raster_fill's colour update of a cover (csrc/raster_edges.hip, blend_rows: one asm statement that holds the translucent blend and the opaque
move, chosen by a scalar branch inside it, under the four row groups' lane masks as EXEC) and its walk of a tile's curve triangles, directed.

Small frames — 64 x 64, and 72 x 40 whose width and height are no multiple of the tile — at msaa 1, three to a few dozen pixel-aligned rectangles
(and one case of curved outlines), pinned to the edge pass so that k_raster_fill draws. Every frame is compared byte for byte with the same draws
through the per-sample edge kernel (CRH_FILL_KERNEL=0), through the triangle pass (CRH_TRIANGLE_PASS=1) and with the oracle. The cases are the
smallest that reach each way through the statement: both variants in one tile's list, row groups whose mask is zero (a lane owns the pixel rows
rq, rq + 4, rq + 8, rq + 12 of its tile, so a cover over rows 0-3 or 12-15 leaves three of the four masks empty), an opaque source that must take
the arithmetic (a -0 component; a pass whose colours are not all tame), the attachment's rounding behind the blend, a list that runs across a
chunk boundary with covers as entries 63 and 64, and the late start's verification failing (debug bit 25), within a chunk and across chunks."""
import numpy as np
import pytest

from contrast_renderer_amd import Path, batch_from_shapes, scenes
from contrast_renderer_amd import renderer as R

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (72, 40)]
PATHS = {"fill": [("CRH_EDGE_PASS", "1")], "edges": [("CRH_EDGE_PASS", "1"), ("CRH_FILL_KERNEL", "0")], "triangles": [("CRH_TRIANGLE_PASS", "1")]}


def rect(x0, row0, x1, row1):
    """Pixel columns [x0, x1) and pixel rows [row0, row1) of the image (row 0 is the top; the instance transform is y-up)."""
    return ("rect", (x0, row0, x1, row1))


def shapes_of(case, height):
    out = []
    for kind, v in case["shapes"]:
        if kind == "rect":
            x0, row0, x1, row1 = v
            out.append(([], [Path.from_rect((0.5 * (x0 + x1), height - 0.5 * (row0 + row1)), (0.5 * (x1 - x0), 0.5 * (row1 - row0)))]))
        else:
            out.append(([], [v(height)]))
    return out


def tile_stack(n, rng, opaque=()):
    """n rectangles that each hold the whole of tile (1, 1) (pixels 16..31 both ways) and more: one cover entry each in that tile's list."""
    shapes, colors = [], []
    for k in range(n):
        shapes.append(rect(int(rng.randint(0, 15)), int(rng.randint(0, 15)), int(rng.randint(33, 40)), int(rng.randint(33, 40))))
        colors.append([rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0, 1), 1.0 if k in opaque else rng.uniform(0.05, 0.3)])
    return shapes, colors


def curved(points_of):
    return ("path", points_of)


def curve_shapes():
    """Outlines of every curve kind through tile (1, 1), each once counter-clockwise and once clockwise: the curve triangles of both facings."""
    def quad(flip):
        def make(h):
            a, c, b = (18.0, h - 18.0), (40.0, h - 24.0), (20.0, h - 30.0)
            p = Path(start=a)
            if flip:
                p.push_integral_quadratic_curve(c, b)
                p.push_line((12.0, h - 25.0))
            else:
                p.push_line((12.0, h - 25.0))
                p.push_line(b)
                p.push_integral_quadratic_curve(c, a)
            return p
        return make

    def cubic(flip):
        def make(h):
            a, c1, c2, b = (17.0, h - 17.0), (30.0, h - 12.0), (36.0, h - 34.0), (19.0, h - 31.0)
            p = Path(start=a)
            if flip:
                p.push_integral_cubic_curve(c1, c2, b)
            else:
                p.push_line(b)
                p.push_integral_cubic_curve(c2, c1, a)
            return p
        return make

    def rational_quad(flip):
        def make(h):
            a, c, b = (22.0, h - 16.5), (44.0, h - 23.0), (23.0, h - 31.5)
            p = Path(start=a)
            if flip:
                p.push_rational_quadratic_curve(2.5, c, b)
            else:
                p.push_line(b)
                p.push_rational_quadratic_curve(2.5, c, a)
            return p
        return make

    def rational_cubic(flip):
        def make(h):
            a, c1, c2, b = (16.5, h - 20.0), (24.0, h - 6.0), (38.0, h - 30.0), (18.0, h - 29.0)
            p = Path(start=a)
            w = (1.0, 2.0, 0.5, 1.0)
            if flip:
                p.push_rational_cubic_curve(w, c1, c2, b)
            else:
                p.push_line(b)
                p.push_rational_cubic_curve(w[::-1], c2, c1, a)
            return p
        return make

    circle = lambda h: Path.from_circle((24.0, h - 24.0), 6.5)
    return [curved(f(flip)) for f in (quad, cubic, rational_quad, rational_cubic) for flip in (False, True)] + [curved(circle)]


def cases():
    rng = np.random.RandomState(11)
    out = {}
    # both variants in one tile's list, with and without the late start (the opaque cover is whole-tile, behind two whole-tile resets) and with its
    # verification failing; the rectangles' own edges give the neighbouring tiles partial masks
    stack = [rect(3, 2, 45, 38), rect(0, 0, 40, 40), rect(5, 9, 37, 36), rect(10, 12, 47, 33), rect(20, 20, 28, 28)]
    stack_colors = [[0.9, 0.2, 0.1, 0.5], [0.1, 0.8, 0.3, 0.25], [0.2, 0.3, 0.9, 1.0], [0.7, 0.7, 0.1, 0.4], [0.3, 0.9, 0.8, 1.0]]
    out["translucent-opaque-translucent"] = dict(shapes=stack, colors=stack_colors)
    out["late-start-verification-fails"] = dict(shapes=stack, colors=stack_colors, debug=1 << 25)
    # pixel rows 0-3 and 12-15 of tile row 1 (image rows 16..19 and 28..31), a translucent and an opaque cover each: three of a lane's four masks are zero
    out["rows-0-3-and-12-15"] = dict(shapes=[rect(2, 16, 14, 20), rect(18, 16, 30, 20), rect(2, 28, 14, 32), rect(18, 28, 30, 32), rect(33, 16, 47, 20), rect(33, 28, 47, 32)],
                                     colors=[[0.2, 0.9, 0.4, 0.6], [0.9, 0.1, 0.6, 1.0], [0.3, 0.5, 0.9, 0.35], [0.8, 0.8, 0.2, 1.0], [0.5, 0.5, 0.5, 0.5], [0.1, 0.2, 0.3, 1.0]])
    # an opaque source with a -0 component: through the arithmetic -0 + dst * 0 is +0, so it must not take the move (the binary16 frame keeps the sign)
    out["opaque-source-with-minus-zero"] = dict(shapes=[rect(1, 1, 39, 39), rect(4, 4, 36, 36), rect(17, 2, 30, 38)],
                                                colors=[[0.4, 0.6, 0.2, 0.7], [-0.0, 0.5, -0.0, 1.0], [0.25, -0.0, 0.75, 1.0]], f16=True)
    # an opaque source in a pass whose colours are not all tame: no move, no late start (r.occlude is 0). One Shape far outside the frame has a component
    # beyond the 1e30 the host allows a tame colour; a component that is not finite never reaches a kernel (the upload refuses it: NonFinite)
    out["opaque-source-pass-not-tame"] = dict(shapes=[rect(1, 1, 39, 39), rect(0, 0, 40, 40), rect(17, 2, 30, 38), rect(-900, 5, -880, 25)],
                                              colors=[[0.4, 0.6, 0.2, 0.7], [0.9, 0.5, 0.1, 1.0], [0.25, 0.1, 0.75, 1.0], [1e31, 0.0, 0.0, 1.0]])
    # the attachment's rounding behind the blend, two translucent covers (and an opaque one) on one sample
    out["attachment-rounds-every-blend"] = dict(shapes=[rect(2, 3, 38, 37), rect(9, 0, 33, 40), rect(16, 16, 40, 30), rect(20, 18, 44, 26)],
                                                colors=[[0.93, 0.21, 0.17, 0.37], [0.11, 0.83, 0.29, 0.61], [0.6, 0.4, 0.2, 1.0], [0.23, 0.37, 0.91, 0.43]], fmt=R.FORMAT_RGBA8_ATTACHMENT)
    # more than 64 entries in tile (1, 1): three Shapes with edges in it in front, then 72 whole-tile covers — entries 63 and 64 are covers, the group
    # loop runs on across the chunk boundary; then the same with opaque covers in both chunks, and with the late start's verification failing across chunks
    front = [rect(18, 18, 50, 50), rect(0, 0, 24, 27), rect(20, 5, 29, 45)]
    front_colors = [[0.5, 0.1, 0.9, 0.5], [0.9, 0.9, 0.1, 0.3], [0.1, 0.9, 0.9, 1.0]]
    shapes, colors = tile_stack(72, rng)
    out["covers-across-the-chunk-boundary"] = dict(shapes=front + shapes, colors=front_colors + colors)
    shapes, colors = tile_stack(72, rng, opaque=(20, 58, 61, 66))
    out["opaque-covers-in-both-chunks"] = dict(shapes=front + shapes, colors=front_colors + colors)
    out["late-start-fails-across-chunks"] = dict(shapes=front + shapes, colors=front_colors + colors, debug=1 << 25)
    # curve triangles of every kind and both facings in one tile, under translucent and opaque covers
    curves = curve_shapes()
    out["curve-triangles-both-facings"] = dict(shapes=[rect(0, 0, 40, 40)] + curves,
                                               colors=[[0.2, 0.2, 0.2, 1.0]] + [[rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0, 1), (1.0, 0.45)[k % 2]] for k in range(len(curves))])
    return out


CASES = cases()
_drawn = {}


def drawn(name, size, path, monkeypatch):
    """The frames of the case through one raster path: [the verified pass, the pass with the lists in place] and, for an f16 case, the binary16 frame."""
    key = (name, size, path)
    if key in _drawn:
        return _drawn[key]
    import torch
    assert torch.cuda.is_available()
    from test_gpu_fuzz import _no_path_pins, last_pass
    case = CASES[name]
    width, height = size
    _no_path_pins(monkeypatch)
    for pin in PATHS[path]:
        monkeypatch.setenv(*pin)
    if case.get("debug"):
        monkeypatch.setenv("CRH_RASTER_DEBUG", str(case["debug"]))
    batch = batch_from_shapes(shapes_of(case, height))
    n = batch.n_shapes
    transforms = scenes.place(width, height, np.zeros(n), np.zeros(n), np.ones(n))
    colors = np.float32(case["colors"])
    r = R.Renderer(R.Configuration(msaa_sample_count=1, clip_nesting_counter_bits=0, winding_counter_bits=4), device=0)
    scene = R.Scene(r, batch)
    assert scene.status() == 0
    images = []
    for fmt in [case.get("fmt", R.FORMAT_RGBA8)] + ([R.FORMAT_RGBA16F] if case.get("f16") else []):
        frame = R.Frame(r, width, height, fmt)
        for k in range(2):
            frame.clear()
            scene.render(frame, transforms, colors)
            images.append(frame.download())
            t = last_pass(frame)
            ran = {"fill": t["formulation"] == 1 and t["raster"] == "fill", "edges": t["formulation"] == 1 and t["raster"] in ("edges", "edges-long"),
                   "triangles": t["formulation"] == 2 and t["raster"] == "tile"}[path]
            assert t["general"] == 0 and ran, (name, size, path, k, t)
    _drawn[key] = images
    return images


def oracle_image(name, size, oracle_lib):
    key = (name, size, "oracle")
    if key not in _drawn:
        case = CASES[name]
        width, height = size
        batch = batch_from_shapes(shapes_of(case, height))
        n = batch.n_shapes
        o = oracle_lib.Oracle(batch)
        assert o.status() == 0, o.status()
        _drawn[key] = o.render(width, height, 1, 4, scenes.place(width, height, np.zeros(n), np.zeros(n), np.ones(n)), np.float32(case["colors"]),
                               attachment8=case.get("fmt") == R.FORMAT_RGBA8_ATTACHMENT)
    return _drawn[key]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("size", SIZES, ids=["64x64", "72x40"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fill_kernel_covers_equal_the_other_paths_and_the_oracle(name, size, oracle_lib, monkeypatch):
    expect = oracle_image(name, size, oracle_lib)
    fill = drawn(name, size, "fill", monkeypatch)
    assert expect.any(), "the case draws nothing"
    for k, image in enumerate(fill[:2]):
        assert same(image, expect), f"{name} {size} pass {k}: {(image != expect).any(axis=2).sum()} pixels differ from the oracle"
    for other in ("edges", "triangles"):
        images = drawn(name, size, other, monkeypatch)
        assert len(images) == len(fill)
        for k, (a, b) in enumerate(zip(fill, images)):
            assert same(a, b), f"{name} {size} frame {k}: {(a.view(np.uint16 if a.dtype == np.float16 else np.uint8) != b.view(np.uint16 if b.dtype == np.float16 else np.uint8)).any(axis=2).sum()} pixels differ from the {other} path"


def test_the_minus_zero_source_keeps_the_arithmetic_in_the_binary16_frame(monkeypatch):
    """The second rectangle's red and blue are -0 and it is opaque: src + dst * 0 is +0 where the move would leave -0 (sign bit 0x8000 in binary16)."""
    for size in SIZES:
        f16 = drawn("opaque-source-with-minus-zero", size, "fill", monkeypatch)[2]
        assert f16.dtype == np.float16
        inside = f16[5:35, 5:16].view(np.uint16)  # the second rectangle over the first alone (image rows 4..35, columns 4..16 — the third begins at column 17)
        assert inside.size and not (inside == 0x8000).any()
