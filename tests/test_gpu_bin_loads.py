"""The global loads of the binning kernels, issued in groups (csrc/bin_edges.hip: load_edge_flags / edge_where / load_edge_verts / finish_edge,
issue_plain_triangle / finish_plain_triangle, and the direct tile lists of a batch that replays). A fill edge's target vertex is
computed from three flags with selects, a hull edge's from its position; every lane loads at indices clamped to its item's own vertices; a triangle's
vertices are loaded as word pairs whatever its kind; a direct pass stores its keys at addresses pass 2a left in the pool cells. Every scene here sits
where one of those index computations can go wrong — the first and the last record of a stream, strips of every short length, the edge at which a
workgroup's lanes start their next round, every kind of triangle in one wavefront — and every frame is compared byte for byte with the oracle's.

Each scene is drawn four times into one frame (the first pass through the pair stream, from the third on with the lists in place: asserted from the
binning word) by the 128-thread kernel with and without the replay, by the 64-thread kernel and by the item-wise kernel, at msaa 1 and 4."""
import math

import numpy as np
import pytest

from test_gpu_bin_footprint import Item, item_costs, polygon
from test_gpu_bin_lanes import bin_word
from test_gpu_bin_replay import DIRECT, pinned
from test_gpu_bin_replay_limits import saw
from test_gpu_parity import gpu, make_renderer  # noqa: F401 (the module-scoped fixture and the helper of the parity tests)

pytestmark = pytest.mark.gpu

PASSES = 4
MSAA = [1, 4]
KERNELS = {"replay": {}, "walk-again": dict(CRH_BIN_REPLAY=0), "64-threads": dict(CRH_BIN_FLAT_THREADS=64), "itemwise": dict(CRH_BIN_ITEMWISE=1)}
NOT_BINNED = 0x80000000


def as_scene(items, size):
    """test_gpu_bin_footprint.py's scene_of, with the stroke options an Item may carry (`dyn`)."""
    from contrast_renderer_amd import scenes
    from contrast_renderer_amd.path import batch_from_shapes
    rng = np.random.RandomState(len(items))
    batch = batch_from_shapes([(getattr(it, "dyn", []), it.paths) for it in items])
    transforms = scenes.place(size[0], size[1], np.array([it.cx for it in items], dtype=np.float64), np.array([it.cy for it in items], dtype=np.float64),
                              np.array([it.scale for it in items], dtype=np.float64))
    colors = np.array([it.color if it.color is not None else (rng.uniform(), rng.uniform(), rng.uniform(), 1.0 if k % 3 == 0 else rng.uniform(0.3, 0.9))
                       for k, it in enumerate(items)], dtype=np.float32)
    return dict(batch=batch, transforms=transforms, colors=colors, width=size[0], height=size[1], n_items=len(items))


_ORACLE = {}


def oracle_image(oracle_lib, name, sc, msaa):
    """The oracle's image of a scene: rendered once per (scene, msaa), shared by the kernels' runs and never written to."""
    if (name, msaa) not in _ORACLE:
        oracle = oracle_lib.Oracle(sc["batch"], 4)
        assert oracle.status() == 0
        image = oracle.render(sc["width"], sc["height"], msaa, 4, sc["transforms"], sc["colors"])
        assert image.any(), "the scene draws something"
        image.setflags(write=False)
        _ORACLE[(name, msaa)] = image
    return _ORACLE[(name, msaa)]


def draw(gpu, sc, msaa, expect, **env):  # noqa: F811
    """PASSES passes into one new frame, each the oracle's image -> the costs the first pass left (None: the kernel leaves none), the binning words."""
    with pinned(**dict(dict(CRH_BIN_ITEMS=32), **env)):
        r = make_renderer(gpu, msaa, 4)
        scene = gpu.Scene(r, sc["batch"])
        assert scene.status() == 0
        frame = gpu.Frame(r, sc["width"], sc["height"])
        costs, words = None, []
        for k in range(PASSES):
            frame.clear()
            if k == 0:
                scene.render(frame, sc["transforms"], sc["colors"])
            else:
                scene.render(frame)
            got = frame.download()
            assert np.array_equal(got, expect), f"{env}, pass {k}: {(got != expect).any(axis=2).sum()} pixels differ"
            words.append(bin_word(frame)[0])
            if k == 0 and "CRH_BIN_ITEMWISE" not in env:
                costs = item_costs(frame, sc["n_items"])
        assert scene.status() == 0
    assert not (words[0] & DIRECT) and all(w & DIRECT for w in words[2:]), [hex(w) for w in words]
    return costs


def every_kernel(gpu, oracle_lib, name, items, size, msaa, **env):  # noqa: F811
    """The scene through all four kernels -> the costs of the default one's first pass."""
    sc = as_scene(items, size)
    expect = oracle_image(oracle_lib, name, sc, msaa)
    costs = None
    for kernel, pins in KERNELS.items():
        got = draw(gpu, sc, msaa, expect, **pins, **env)
        if kernel == "replay":
            costs = got
    return costs


# ---------------------------------------------------------------------------------------------- chain topology
def two_sub_paths():
    """A fill of two sub-paths — a quadrilateral and a triangle inside it, wound the other way: the strip restarts at the triangle's first vertex,
    where the flag of the vertex in front (the last of the first strip) decides that the edge is a strip's first."""
    from contrast_renderer_amd.path import Path
    return [Path.from_polygon([(-1.0, -1.0), (-1.0, 1.0), (1.0, 1.0), (1.0, -1.0)]), Path.from_polygon([(-0.5, -0.4), (0.5, -0.4), (0.0, 0.6)])]


CHAINS = {
    "3-vertices": (lambda: polygon(3), 3, 3),  # (fill edges, hull vertices)
    "4-vertices": (lambda: polygon(4), 4, 4),
    "5-vertices": (lambda: polygon(5), 5, 5),
    "two-sub-paths": (two_sub_paths, 7, 4),
}


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_a_scene_of_one_short_chain(gpu, oracle_lib, chain, msaa):  # noqa: F811
    """ONE Shape: its fill chain begins at the first vertex of the Scene's streams — the clamped g - 1 and g - 2 of its first two edges — and ends at their
    last record — the clamped g + 1 and g + 2 —, and so does its hull chain of three or four vertices: position 0, the even positions' pos - 2, and
    both end-of-strip targets (pos + 1 == n and pos + 2 == n) of the odd ones; a strip triangle only where pos + 2 < n."""
    paths, fill_edges, hull = CHAINS[chain]
    costs = every_kernel(gpu, oracle_lib, f"one-{chain}", [Item(paths(), 31.0, 33.0, 22.0, color=(0.9, 0.3, 0.2, 0.8))], (64, 64), msaa)
    assert costs == [(0, fill_edges + hull, costs[0][2])], costs


@pytest.mark.parametrize("msaa", MSAA)
def test_short_chains_side_by_side(gpu, oracle_lib, msaa):  # noqa: F811
    """The same chains as neighbours in the streams, in both orders: a clamp that reached into the neighbour's vertices would be seen."""
    names = list(CHAINS)
    for order, label in ((names, "ascending"), (names[::-1], "descending")):
        items = [Item(CHAINS[c][0](), 20.0 + 30.0 * (k % 4), 24.0 + 44.0 * (k // 4), 13.0) for k, c in enumerate(order * 2)]
        costs = every_kernel(gpu, oracle_lib, f"chains-{label}", items, (128, 96), msaa)
        assert [c[1] for c in costs] == [CHAINS[c][1] + CHAINS[c][2] for c in order * 2], costs


# ---------------------------------------------------------------------------------------------- round boundaries
@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("edges", [128, 129, 256, 257, 384])
def test_one_item_whose_edges_end_at_a_round_boundary(gpu, oracle_lib, edges, msaa):  # noqa: F811
    """A workgroup of 128 lanes takes its batch's edges in rounds of 128 (64 lanes: rounds of 64, and an item beyond 192 edges goes to the item-wise
    kernel's queue): one item with exactly as many fill + hull edges as one, two and three rounds hold, and with one more. The hull of a saw is its
    four corners, so the hull chain — the item's last four edges — straddles the boundary or begins the next round alone."""
    costs = every_kernel(gpu, oracle_lib, f"saw-{edges}", [Item(saw(edges - 4), 64.0, 64.0, 50.0, color=(0.2, 0.5, 0.9, 0.6))], (128, 128), msaa)
    assert costs[0][:2] == (0, edges), costs


@pytest.mark.parametrize("msaa", MSAA)
def test_two_items_whose_edges_straddle_a_round_boundary(gpu, oracle_lib, msaa):  # noqa: F811
    """126 edges of a saw, then a pentagon's ten: edges 126 and 127 are the pentagon's first in the first round, the other eight the second round's first."""
    items = [Item(saw(122), 40.0, 64.0, 30.0), Item(polygon(5), 100.0, 60.0, 20.0)]
    costs = every_kernel(gpu, oracle_lib, "straddle", items, (128, 128), msaa)
    assert [c[1] for c in costs] == [126, 10], costs


def open_stroke(points=((-1.0, -0.5), (0.0, 0.6), (1.0, -0.5))):
    """An open stroked polyline: line triangles and joints, nothing filled."""
    from contrast_renderer_amd.path import CurveApproximation, Path, StrokeOptions
    path = Path(start=points[0])
    for p in points[1:]:
        path.push_line(p)
    path.stroke_options = StrokeOptions(0.25, 0.0, 4.0, False, 0, CurveApproximation.UniformlySpacedParameters(2))
    return path


def solid_options():
    from contrast_renderer_amd.path import Cap, DynamicStrokeOptions, Join
    return [DynamicStrokeOptions.Solid(Join.Miter, Cap.Butt, Cap.Butt)]


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("points,edges", [(((-1.0, -0.5), (0.0, 0.6), (1.0, -0.5)), 5), (((-1.0, -0.5), (1.0, 0.6)), 4)], ids=["polyline", "segment"])
def test_a_batch_of_a_single_item_without_a_fill_chain(gpu, oracle_lib, points, edges, msaa):  # noqa: F811
    """An open stroke alone in its Scene: no fill edge — no lane of the batch asks for a flag, and the fill streams of the Scene are EMPTY, so an index
    clamped into them would already be out of bounds. Its only edges are its hull chain's: five for the polyline, four for a single segment."""
    items = [Item([open_stroke(points)], 32.0, 32.0, 20.0, color=(0.1, 0.8, 0.3, 1.0))]
    items[0].dyn = solid_options()
    costs = every_kernel(gpu, oracle_lib, f"stroke-alone-{edges}", items, (64, 64), msaa)
    assert costs[0][0] > 0 and costs[0][1] == edges, costs


@pytest.mark.parametrize("msaa", MSAA)
def test_batches_of_a_single_item_without_any_edge(gpu, oracle_lib, msaa):  # noqa: F811
    """One item per workgroup in every pass (CRH_BIN_ITEMS=1 for a frame's first, runs of one item from then on): a Shape without a path — no triangle, no fill edge, no hull: its batch runs
    no round of edges, and every lane of it is one that must not load — and a Shape of ONE vertex, a strip whose first vertex is its last (no edge
    either, but a flag to read), between two ordinary polygons."""
    from contrast_renderer_amd.path import Path
    items = [Item(polygon(5), 20.0, 20.0, 12.0), Item([], 32.0, 32.0, 10.0), Item([Path(start=(0.0, 0.0))], 32.0, 32.0, 10.0), Item(polygon(4), 44.0, 44.0, 12.0)]
    costs = every_kernel(gpu, oracle_lib, "edge-less", items, (64, 64), msaa, CRH_BIN_ITEMS=1, CRH_BIN_BATCH_ITEMS=1)
    assert [c[:2] for c in costs] == [(0, 10), (0, 0), (0, 1), (0, 8)] and costs[1][2] == 0 and costs[2][2] == 0, costs


# ---------------------------------------------------------------------------------------------- kinds
def curve_shape(kind):
    """A closed path of three segments of one kind around the origin."""
    from contrast_renderer_amd.path import Path
    on = [(math.cos(-2.0 * math.pi * k / 3.0), math.sin(-2.0 * math.pi * k / 3.0)) for k in range(3)]
    path = Path(start=on[0])
    for k in range(3):
        a, b = on[k], on[(k + 1) % 3]
        mid = (0.9 * (a[0] + b[0]), 0.9 * (a[1] + b[1]))
        c0, c1 = (0.6 * a[0] + 0.4 * mid[0] * 1.6, 0.6 * a[1] + 0.4 * mid[1] * 1.6), (0.6 * b[0] + 0.4 * mid[0] * 1.6, 0.6 * b[1] + 0.4 * mid[1] * 1.6)
        if kind == "iq":
            path.push_integral_quadratic_curve(mid, b)
        elif kind == "ic":
            path.push_integral_cubic_curve(c0, c1, b)
        elif kind == "rq":
            path.push_rational_quadratic_curve(1.7, mid, b)
        else:
            path.push_rational_cubic_curve((1.0, 1.6, 0.7, 1.0), c0, c1, b)
    return [path]


def kinds_items():
    """One Shape per vertex stream a triangle can come from, few enough triangles for one wavefront: stroke lines and joints, the four curve lists,
    and a plain polygon (with CRH_RASTER_DEBUG=4 every hull strip is binned as cover triangles: the seventh stream)."""
    stroke = Item([open_stroke()], 0.0, 0.0, 1.0)
    stroke.dyn = solid_options()
    shapes = [("stroke", stroke)] + [(k, Item(curve_shape(k), 0.0, 0.0, 1.0)) for k in ("iq", "ic", "rq", "rc")] + [("polygon", Item(polygon(5), 0.0, 0.0, 1.0))]
    return shapes


@pytest.mark.parametrize("folded", [False, True], ids=["hull-chains", "folded-hulls"])
@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("last", ["stroke", "iq", "ic", "rq", "rc", "polygon"])
def test_every_kind_of_triangle_in_one_wavefront_each_stream_ending_with_the_last_shape(gpu, oracle_lib, last, msaa, folded):  # noqa: F811
    """Six Shapes in one batch — stroke lines, joints, integral and rational quadratics and cubics in one wavefront, the hull strips' cover triangles
    with them when the strips are folded —, rotated so that each Shape in turn is the Scene's last: its stream then ENDS with the last triangle's last
    vertex, and a load that reached beyond a vertex would leave the stream."""
    shapes = kinds_items()
    at = [name for name, _ in shapes].index(last)
    order = shapes[at + 1:] + shapes[:at + 1]
    items = []
    for k, (_, it) in enumerate(order):
        placed = Item(it.paths, 24.0 + 40.0 * (k % 3), 26.0 + 44.0 * (k // 3), 15.0)
        placed.dyn = getattr(it, "dyn", [])
        items.append(placed)
    env = dict(CRH_RASTER_DEBUG=4) if folded else {}
    costs = every_kernel(gpu, oracle_lib, f"kinds-{last}", items, (128, 96), msaa, **env)
    assert sum(c[0] for c in costs) <= 64 and all(c[0] > 0 for (name, _), c in zip(order, costs) if name != "polygon"), costs


# ---------------------------------------------------------------------------------------------- direct lists at their limit
LIMIT_SIZE = 128
N_EACH = 12  # triangles and quadrilaterals: 2 k + 1 entries each in the tile that holds one (k fill edges, k hull edges, the COVER entry)


def tile_place(frame, tile):
    """(first entry, first entry of the next tile's place) of the list of `tile` in the pass to come, and the entries the frame's last pass counted in the
    tile (crh_debug_frame_tile_place)."""
    import ctypes as C
    from contrast_renderer_amd import _ffi
    lib = frame.lib
    lib.crh_debug_frame_tile_place.restype = C.c_int
    lib.crh_debug_frame_tile_place.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    out = (C.c_uint32 * 3)()
    _ffi.check(lib.crh_debug_frame_tile_place(frame.handle, tile, out))
    return int(out[0]), int(out[1]), int(out[2])


def limit_scene():
    """Twelve triangles and twelve quadrilaterals of radius 5 px, one per tile centre (tile 16 px): Shape 0, a triangle, on the tile under test."""
    per_row = LIMIT_SIZE // 16
    spots_ = [(16.0 * (k % per_row) + 8.0, 16.0 * (k // per_row) + 8.0) for k in range(2 * N_EACH)]
    items = [Item(polygon(3 if k < N_EACH else 4), x, y, 5.0, color=(0.1 + 0.03 * k, 0.9 - 0.03 * k, 0.4, 0.5)) for k, (x, y) in enumerate(spots_)]
    return items, spots_[0]


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_a_tile_list_one_below_at_and_one_above_the_room_of_its_place(gpu, oracle_lib, kernel, msaa):  # noqa: F811
    """Shapes spread one per tile until the lists are in place, then some of them moved (set_instances) onto ONE tile so that its list has one entry
    less than the room its place has, exactly that many, and one more — the room and the count are read from the frame
    (crh_debug_frame_tile_place). Up to "exactly" the pass stays as it was drawn, with the lists in place; one more is noticed and the pass is drawn
    again the verified way (the binning word of the frame's last pass then lacks the bit). All frames are the oracle's."""
    from contrast_renderer_amd import scenes
    items, (tx, ty) = limit_scene()
    sc = as_scene(items, (LIMIT_SIZE, LIMIT_SIZE))
    spread, colors = sc["transforms"], sc["colors"]
    tile = int((LIMIT_SIZE - ty) // 16) * (LIMIT_SIZE // 16) + int(tx // 16)
    on_tile = scenes.place(LIMIT_SIZE, LIMIT_SIZE, np.full(len(items), tx), np.full(len(items), ty), np.full(len(items), 5.0))
    oracle = oracle_lib.Oracle(sc["batch"], 4)
    assert oracle.status() == 0
    images = {}

    def expect(t, key):
        if key not in images:
            images[key] = oracle.render(LIMIT_SIZE, LIMIT_SIZE, msaa, 4, t, colors)
        return images[key]

    with pinned(CRH_BIN_ITEMS=32, **KERNELS[kernel]):
        r = make_renderer(gpu, msaa, 4)
        scene = gpu.Scene(r, sc["batch"])
        frame = gpu.Frame(r, LIMIT_SIZE, LIMIT_SIZE)

        def one_pass(t, key):
            scene.set_instances(t, colors)
            frame.clear()
            scene.render(frame)
            got = frame.download()
            want = expect(t, key)
            assert np.array_equal(got, want), f"{key}: {(got != want).any(axis=2).sum()} pixels differ"
            return bin_word(frame)[0]

        for delta in (-1, 0, 1):
            for _ in range(4):  # (the places of a pass follow the counts of the pass before it: spread again, until the lists are in place)
                word = one_pass(spread, "spread")
            first, end, count = tile_place(frame, tile)
            assert word & DIRECT and count == 7, (hex(word), count)
            room = end - first
            want = room + delta
            choice = [(a, b) for b in range(N_EACH + 1) for a in range(1, N_EACH + 1) if 7 * a + 9 * b == want]
            assert choice, f"no {want} entries from triangles of 7 and quadrilaterals of 9"
            a, b = choice[0]
            moved = spread.copy()
            chosen = list(range(a)) + list(range(N_EACH, N_EACH + b))
            moved[chosen] = on_tile[chosen]
            word = one_pass(moved, (a, b))
            count = tile_place(frame, tile)[2]
            print(f"{kernel}, msaa {msaa}: room {room}, {a} triangles + {b} quadrilaterals = {want} entries, {count} counted, binning word {word:#x}")
            assert count == want, (count, want)
            assert bool(word & DIRECT) == (delta <= 0), (delta, hex(word))
        assert scene.status() == 0
