"""k_bin_flat's LDS tables at their limits (csrc/bin_edges.hip): the kernel runs at four waves per SIMD because its tables are small —
both backdrop sums of a pool cell in one word, sixteen bits each; a pair stage of 64 entries; the edges' flags in 16-bit words; the edges in LDS
from the set-up on. Every scene here sits where one of those can go wrong, and every frame is the oracle's, bit for bit, at msaa 1 and 4, with the
default workgroup and with CRH_BIN_FLAT_THREADS=64.

What a batch holds (items, triangles, edges, tile cells) is read from the library (crh_debug_flat_batches), what an item takes of it from the kernel
itself (the costs a frame's first pass leaves, crh_debug_frame_bin_dump): the scenes are packed from a catalogue of Shapes whose costs were read
that way, and every test asserts that the packed scene reached the limit it aims at. CRH_BIN_ITEMS=32 makes the first pass take a full batch of items
per workgroup (the kernel's own fitting: what does not fit waits for the workgroup's next turn); the later passes take the runs the host cut by cost.

Frames are 256 x 256, but for the item wider than the pool: a frame of 256 tiles cannot exceed a pool of 384 cells."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_parity import gpu, make_renderer  # noqa: F401 (the module-scoped fixture and the helper of the parity tests)

pytestmark = pytest.mark.gpu

SIZE = 256
TILE = 16  # pixels (renderer.py Frame.set_tile_rows: "whole 16-pixel tile rows"); only placements use it — every cell count is read back
TOO_WIDE, NOT_BINNED = 0xFFFFFFFF, 0x80000000
SHAPES = [pytest.param(None, id="default-threads"), pytest.param("64", id="64-threads")]
MSAA = [1, 4]


# ---------------------------------------------------------------------------------------------- Shapes (local units, clockwise: scenes.py _blob_points)
def ring(q, bulge=1.5):
    """q integral quadratic segments around the unit circle, control points at radius `bulge`: q triangles, q fill edges, a hull of the q control points."""
    from contrast_renderer_amd.path import Path
    on = [(math.cos(-2.0 * math.pi * k / q), math.sin(-2.0 * math.pi * k / q)) for k in range(q)]
    ctl = [(bulge * math.cos(-2.0 * math.pi * (k + 0.5) / q), bulge * math.sin(-2.0 * math.pi * (k + 0.5) / q)) for k in range(q)]
    path = Path(start=on[0])
    for k in range(q):
        path.push_integral_quadratic_curve(ctl[k], on[(k + 1) % q])
    return [path]


def polygon(k, dent=None):
    """A regular k-gon: k fill edges and a hull of k vertices; `dent`: vertex 1 pulled to that radius, inside the hull of the others (one hull vertex less)."""
    from contrast_renderer_amd.path import Path
    pts = [(math.cos(-2.0 * math.pi * i / k), math.sin(-2.0 * math.pi * i / k)) for i in range(k)]
    if dent is not None:
        pts[1] = (dent * pts[1][0], dent * pts[1][1])
    return [Path.from_polygon(pts)]


def bump():
    """A triangle with one curved side: ONE curve triangle."""
    from contrast_renderer_amd.path import Path
    path = Path(start=(1.0, 0.0))
    path.push_line((-0.5, -0.8))
    path.push_line((-0.5, 0.8))
    path.push_integral_quadratic_curve((0.9, 0.9), (1.0, 0.0))
    return [path]


def rect(x0, y0, x1, y1):
    from contrast_renderer_amd.path import Path
    return [Path.from_polygon([(x0, y0), (x0, y1), (x1, y1), (x1, y0)])]


class Item:
    """A Shape with its place: what it costs a batch does not change when it is drawn in another scene."""

    def __init__(self, paths, cx, cy, scale, color=None):
        self.paths, self.cx, self.cy, self.scale, self.color = paths, cx, cy, scale, color


def scene_of(items, size=(SIZE, SIZE)):
    from contrast_renderer_amd import scenes
    from contrast_renderer_amd.path import batch_from_shapes
    rng = np.random.RandomState(len(items))
    batch = batch_from_shapes([([], it.paths) for it in items])
    transforms = scenes.place(size[0], size[1], np.array([it.cx for it in items], dtype=np.float64), np.array([it.cy for it in items], dtype=np.float64),
                              np.array([it.scale for it in items], dtype=np.float64))
    colors = np.array([it.color if it.color is not None else (rng.uniform(), rng.uniform(), rng.uniform(), 1.0 if k % 3 == 0 else rng.uniform(0.3, 0.9))
                       for k, it in enumerate(items)], dtype=np.float32)
    return batch, transforms, colors


# ---------------------------------------------------------------------------------------------- the library's limits and the kernel's costs
def batch_limits(lib):
    """(items, triangles, edges, tile cells) of a batch of the kernel a small pass takes (flat_batch_limits: follows CRH_BIN_FLAT_THREADS)."""
    lib.crh_debug_flat_batches.restype = C.c_int
    lib.crh_debug_flat_batches.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    limits = (C.c_uint32 * 4)()
    runs = (C.c_uint32 * 2)()
    lib.crh_debug_flat_batches(None, 0, runs, 1, limits)
    return tuple(int(v) for v in limits)


def cost_words(frame, n):
    """The two cost words per item that the frame's latest verified pass left (RasterParams::item_cost), as crh_debug_flat_batches takes them."""
    from contrast_renderer_amd import _ffi
    lib = frame.lib
    lib.crh_debug_frame_bin_dump.restype = C.c_int
    lib.crh_debug_frame_bin_dump.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]
    words = (C.c_uint32 * (2 * n))()
    _ffi.check(lib.crh_debug_frame_bin_dump(frame.handle, words, 2 * n))
    return words


def item_costs(frame, n):
    """Per item (triangles, edges, tile cells) as the frame's first pass counted them (RasterParams::item_cost)."""
    words = cost_words(frame, n)
    out = []
    for i in range(n):
        cells, w = int(words[2 * i]), int(words[2 * i + 1])
        out.append((0, 0, cells) if w & NOT_BINNED else (w & 0x1FF, (w >> 9) & 0x3FF, cells))
    return out


@pytest.fixture
def flat(request, monkeypatch, gpu):  # noqa: F811
    """The environment of these tests around one kernel shape: the edge pass, k_bin_flat, full batches in the first pass; -> (renderer module, limits)."""
    threads = request.param
    monkeypatch.setenv("CRH_EDGE_PASS", "1")
    monkeypatch.setenv("CRH_BIN_ITEMS", "32")
    monkeypatch.setenv("CRH_BIN_FLAT", "1")  # (k_bin_flat also where the average item is beyond half a batch: the pass would go item by item)
    for var in ("CRH_BIN_ITEMWISE", "CRH_NO_BIN_BATCHES", "CRH_BIN_BATCH_ITEMS", "CRH_BIN_BATCH_TICKS"):
        monkeypatch.delenv(var, raising=False)
    if threads is None:
        monkeypatch.delenv("CRH_BIN_FLAT_THREADS", raising=False)
    else:
        monkeypatch.setenv("CRH_BIN_FLAT_THREADS", threads)
    from contrast_renderer_amd import _ffi
    return gpu, batch_limits(_ffi.load_library())


def measure(gpu, items, msaa, size=(SIZE, SIZE)):  # noqa: F811
    """The items' costs: one pass into a new frame."""
    batch, transforms, colors = scene_of(items, size)
    r = make_renderer(gpu, msaa, 4)
    scene = gpu.Scene(r, batch)
    assert scene.status() == 0
    frame = gpu.Frame(r, size[0], size[1])
    frame.clear()
    scene.render(frame, transforms, colors)
    return item_costs(frame, len(items))


def draw_against_oracle(gpu, oracle_lib, items, msaa, size=(SIZE, SIZE), config=None, transforms=None, passes=3):  # noqa: F811
    """Three passes into one frame (the kernel's own fitting, then twice the host's runs), each the oracle's image -> the first pass' costs."""
    batch, placed, colors = scene_of(items, size)
    transforms = placed if transforms is None else transforms
    winding_bits = config.winding_counter_bits if config else 4
    oracle = oracle_lib.Oracle(batch, 4)
    assert oracle.status() == 0
    expect = oracle.render(size[0], size[1], msaa, winding_bits, transforms, colors)
    r = gpu.Renderer(config, device=0) if config else make_renderer(gpu, msaa, 4)
    scene = gpu.Scene(r, batch)
    assert scene.status() == 0
    frame = gpu.Frame(r, size[0], size[1])
    costs = None
    for k in range(passes):
        frame.clear()
        scene.render(frame, transforms, colors)
        if k == 0:
            costs = item_costs(frame, len(items))
        got = frame.download()
        assert np.array_equal(got, expect), f"pass {k}: {(got != expect).any(axis=2).sum()} pixels differ"
    assert scene.status() == 0
    return costs


def pack(values, target, most):
    """Indices (repeats allowed, at most `most`) of `values` that sum to `target` exactly, the fewest that do; None: no such choice."""
    best = {0: []}
    for _ in range(most):
        nxt = dict(best)
        for total, chosen in best.items():
            for i, v in enumerate(values):
                t = total + v
                if v > 0 and t <= target and (t not in nxt or len(nxt[t]) > len(chosen) + 1):
                    nxt[t] = chosen + [i]
        best = nxt
        if target in best:
            return best[target]
    return best.get(target)


def fill_table(gpu, oracle_lib, limits, msaa, dim, catalogue, last):  # noqa: F811
    """Two scenes of at most one batch's items from `catalogue` with `last` behind them: the first fills table `dim` (0 triangles, 1 edges, 2 tile cells)
    exactly, `last` included — one turn; in the second `last` overflows it by ONE element and has to wait for the workgroup's next turn. The other
    tables stay below their limits, so the table under test decides."""
    max_items, limit = limits[0], limits[1 + dim]
    costs = measure(gpu, catalogue + [last], msaa)
    assert all(c[2] != TOO_WIDE for c in costs)
    mine, of_last = [c[dim] for c in costs[:-1]], costs[-1][dim]
    assert of_last >= 1
    for over in (0, 1):
        chosen = pack(mine, limit + over - of_last, max_items - 1)
        assert chosen is not None, f"the catalogue cannot make {limit + over - of_last} in {max_items - 1} items: {sorted(set(mine))}"
        items = [catalogue[i] for i in chosen] + [last]
        got = draw_against_oracle(gpu, oracle_lib, items, msaa)
        assert got == [costs[i] for i in chosen] + [costs[-1]], "an item costs the same wherever it is drawn"
        sums = [sum(c[d] for c in got) for d in range(3)]
        assert sums[dim] == limit + over and sum(c[dim] for c in got[:-1]) <= limit
        assert all(sums[d] < limits[1 + d] for d in range(3) if d != dim), (sums, limits)


def spots(n, scale):
    """n places on the frame's tile centres, row by row: a Shape of radius < TILE / 2 there takes one tile cell."""
    per_row = SIZE // TILE
    return [(TILE * (k % per_row) + TILE / 2, TILE * ((k // per_row) % per_row) + TILE / 2, scale) for k in range(n)]


# ---------------------------------------------------------------------------------------------- exact fit of each table
@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", SHAPES, indirect=True)
def test_triangle_table_filled_exactly_and_overflowing_by_one(flat, oracle_lib, msaa):
    gpu, limits = flat  # noqa: F811
    qs = list(range(3, 14))
    catalogue = [Item(ring(q), x, y, s) for q, (x, y, s) in zip(qs, spots(len(qs), 4.5))]
    fill_table(gpu, oracle_lib, limits, msaa, 0, catalogue, Item(bump(), SIZE - TILE / 2, SIZE - TILE / 2, 6.0))


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", SHAPES, indirect=True)
def test_edge_table_filled_exactly_and_overflowing_by_one(flat, oracle_lib, msaa):
    gpu, limits = flat  # noqa: F811
    kinds = [(k, None) for k in range(3, 30, 2)] + [(k, 0.4) for k in range(5, 30, 4)]  # (even sums from the convex ones, odd ones with a dented one)
    catalogue = [Item(polygon(k, dent), x, y, s) for (k, dent), (x, y, s) in zip(kinds, spots(len(kinds), 7.0))]
    fill_table(gpu, oracle_lib, limits, msaa, 1, catalogue, Item(polygon(3), SIZE - TILE / 2, SIZE - TILE / 2, 6.0))


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", SHAPES, indirect=True)
def test_tile_cell_pool_filled_exactly_and_overflowing_by_one(flat, oracle_lib, msaa):
    gpu, limits = flat  # noqa: F811
    spans = [1, 2, 3, 5, 8, 11, 16]  # tiles
    catalogue = [Item(rect(1.0, 1.0, TILE * a - 1.0, TILE * b - 1.0), 0.0, 0.0, 1.0) for a in spans for b in (1, 3, 16) if a * b > 1]
    fill_table(gpu, oracle_lib, limits, msaa, 2, catalogue, Item(polygon(5), SIZE - TILE / 2, TILE / 2, 6.0))


# ---------------------------------------------------------------------------------------------- the queue
@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", SHAPES, indirect=True)
def test_an_item_wider_than_the_pool_is_handed_to_the_queue_kernel(flat, oracle_lib, msaa):
    gpu, limits = flat  # noqa: F811
    side = TILE * (math.isqrt(limits[3]) + 1)  # the smallest square frame with more tiles than the pool has cells
    items = [Item(ring(7), 40.0, 40.0, 20.0), Item(rect(2.0, 2.0, side - 2.0, side - 2.0), 0.0, 0.0, 1.0), Item(polygon(6), side - 50.0, 60.0, 30.0)]
    costs = draw_against_oracle(gpu, oracle_lib, items, msaa, size=(side, side))
    assert costs[1][2] == TOO_WIDE and costs[0][2] != TOO_WIDE and costs[2][2] != TOO_WIDE, costs


# ---------------------------------------------------------------------------------------------- the pair stage
@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", SHAPES, indirect=True)
def test_one_wavefront_stages_more_than_a_stage_holds_in_one_tile_row(flat, oracle_lib, msaa):
    """A batch's edge table full of edges that all lie in ONE tile row: every edge brings at least one entry, so each of the workgroup's wavefronts
    (64 lanes of the `tris` a batch holds) appends edges / wavefronts = 192 entries to that row — three stages' worth, with a flush between them."""
    gpu, limits = flat  # noqa: F811
    max_items, _, max_edges, _ = limits
    k = max_edges // (2 * (max_items - 1))  # (a convex k-gon: 2 k edges)
    items = [Item(polygon(k), TILE + (SIZE - 2 * TILE) * i / (max_items - 2), 5 * TILE + TILE / 2, 7.0) for i in range(max_items - 1)]
    costs = draw_against_oracle(gpu, oracle_lib, items, msaa)
    assert max_edges - 2 * (max_items - 1) < sum(c[1] for c in costs) <= max_edges
    wavefronts = limits[1] // 64
    assert sum(c[1] for c in costs) // wavefronts > 128, "more than the largest stage the kernel has had"


# ---------------------------------------------------------------------------------------------- sixteen-bit backdrop sums
@pytest.mark.parametrize("sign", [1, -1], ids=["clockwise", "counter-clockwise"])
@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", SHAPES, indirect=True)
def test_backdrop_sums_of_a_batch_full_of_edges_left_of_one_column(flat, oracle_lib, msaa, sign):
    """ONE Shape of as many nested triangles as a batch has edges for, all wound the same way: every one has its downward edges left of the frame's
    middle column and its upward edge right of it, so along a tile row the backdrop sum of the Shape's cells climbs by one per triangle — to a third
    of the batch's edges, the most closed chains reach (as many of a chain's crossings of a row run up as down, and a triangle's third edge crosses
    no row the others do not) —, positive or negative by the winding. Eight winding bits: the oracle's counter does not wrap below 255."""
    from contrast_renderer_amd.path import Path
    gpu, limits = flat  # noqa: F811
    max_edges = limits[2]
    m = min((max_edges - 3) // 3, 127)
    paths = []
    for i in range(m):
        inset = 0.9 * i / m  # the outermost triangle is the hull
        a, b, c = (-1.0 + inset, -0.9 + 0.5 * inset), (0.0, 0.9 - 0.5 * inset), (1.0 - inset, -0.9 + 0.5 * inset)
        paths.append(Path.from_polygon([a, b, c] if sign > 0 else [a, c, b]))
    # (a tile and a half wide on either side of a tile boundary: a handful of cells, so that one workgroup's entries stay a few thousand)
    items = [Item(paths, SIZE / 2, SIZE / 2, 1.5 * TILE, color=(0.9, 0.4, 0.1, 0.7)), Item(polygon(5), 40.0, 200.0, 25.0)]
    config = gpu.Configuration(msaa_sample_count=msaa, clip_nesting_counter_bits=0, winding_counter_bits=8)
    costs = draw_against_oracle(gpu, oracle_lib, items, msaa, config=config)
    assert costs[0][1] == 3 * m + 3 and costs[0][1] + 6 > max_edges - 3 and costs[0][2] != TOO_WIDE, costs


# ---------------------------------------------------------------------------------------------- the set-up's order
@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", SHAPES, indirect=True)
def test_rejected_triangles_and_edges_leave_nothing_behind(flat, oracle_lib, msaa):
    """Thin, degenerate and off-frame primitives among ordinary ones: curve triangles with a zero determinant (the control point on the chord) and
    with a tiny one, Shapes whose pixel boxes are clipped to nothing (beyond each side of the frame, and astride a corner), a repeated vertex (an
    edge without length), and — in the second scene — an instance whose transform overflows, so that its vertices are not finite on the frame
    (inf - inf: NaN determinants). A rejected primitive writes no record and moves no box: its item's rectangle is what the others make it."""
    from contrast_renderer_amd.path import Path
    gpu, limits = flat  # noqa: F811
    flat_curve = Path(start=(-1.0, 0.0))  # control points on the chords
    flat_curve.push_integral_quadratic_curve((0.0, 0.0), (1.0, 0.0))
    flat_curve.push_integral_quadratic_curve((0.5, -0.5), (0.0, -1.0))
    flat_curve.push_integral_quadratic_curve((-0.5, -0.5), (-1.0, 0.0))
    thin = Path(start=(-1.0, 0.0))
    thin.push_integral_quadratic_curve((0.0, 1.0e-6), (1.0, 0.0))
    thin.push_line((0.0, -0.002))
    doubled = Path.from_polygon([(1.0, 0.0), (0.0, -1.0), (0.0, -1.0), (-1.0, 0.0), (0.0, 1.0)])
    items = [Item(ring(6), 60.0, 60.0, 30.0), Item([flat_curve], 128.0, 128.0, 40.0), Item([thin], 128.0, 40.0, 60.0), Item([doubled], 200.0, 200.0, 30.0),
             Item(ring(5), -80.0, 100.0, 30.0), Item(ring(5), SIZE + 80.0, 100.0, 30.0), Item(polygon(7), 100.0, -90.0, 30.0), Item(polygon(7), 100.0, SIZE + 90.0, 30.0),
             Item(ring(8), 2.0, SIZE - 2.0, 25.0), Item([flat_curve, thin], 200.0, 60.0, 35.0), Item(bump(), 60.0, 200.0, 1.0e-4), Item(ring(4), 128.0, 200.0, 35.0)]
    costs = draw_against_oracle(gpu, oracle_lib, items, msaa)
    for off_frame in (4, 5, 6, 7):
        assert costs[off_frame][2] == 0, costs  # nothing drawn: no rectangle
    assert costs[1][0] == 3 and costs[1][2] != 0
    # ... and one instance that is not finite on the frame (the frame is then the triangle pass', whatever the binning kernel left)
    _, transforms, _ = scene_of(items)
    transforms = transforms.copy()
    transforms[8, 0] *= 3e38
    transforms[8, 5] *= -3e38
    draw_against_oracle(gpu, oracle_lib, items, msaa, transforms=transforms)
