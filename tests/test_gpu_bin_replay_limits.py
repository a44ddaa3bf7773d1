"""The fall-backs of k_bin_flat's replay that a scene reaches WITHOUT a test knob (csrc/bin_edges.hip, k_bin_flat<S, 128, true>). Pass 1
keeps every hit as a 32-bit LDS record (9 bits of index, 10 of pool cell, 13 of key relative to the first slot of the batch's first item) and pass 3
replays them. A batch walks again instead when (1) a wavefront keeps more records than CRH_BIN_REPLAY_CAP allows — the knob test_gpu_bin_replay.py
turns —, (2) its two wavefronts together find more than hit_room = 800 + 4 * (384 - n_edges) records (they fill one table from opposite ends), or
(3) a hit's key lies 8 192 slots or more behind the batch's first slot. This module reaches (2) and (3) with scenes alone, in a workgroup's first and
second turn, through the pair stream of a verified pass and with the lists in place, and draws glyphs, strokes and folded hull strips under a cap.

Every frame drawn here is compared byte for byte with the oracle's image — also those of the passes that only measure costs and of the capped runs
of a bisection —, and every scene's passes are drawn as well under CRH_BIN_REPLAY=0 (the walk again) and under CRH_BIN_FLAT_THREADS=64, frame for frame
the same image. The kernel's own counters (the flag words of a pass: overflow[77] batches that walked again,
overflow[76] extra turns of workgroups that took a run the host had cut) decide only whether a scene reached the path it aims at; the bound that
excludes the OTHER reason is asserted from the costs a frame's first pass leaves (crh_debug_frame_bin_dump) with the slot layout of edge_slots.hpp.
The environment is the footprint tests' (CRH_EDGE_PASS=1, CRH_BIN_FLAT=1, CRH_BIN_ITEMS=32: a fresh frame's first pass takes sixteen candidates per
workgroup and fits them itself; the later passes take the runs the host cut by cost). Four passes into one frame, the instances set for the first
and resident from then on: the first a verified one through the pair stream, from the third on the lists in place — asserted from the binning word.

A comb is a zig-zag band inside ONE tile column, h tile rows tall: all its edges but two run from its top to its bottom, so every one of them
enters every cell of the item's 1 x h rectangle — a batch with a full edge table (hit_room = 800) then has about 384 * h hits.

Recorded on an MI355X (gfx950, ROCm 7.0.2; `pytest -m gpu -s tests/test_gpu_bin_replay_limits.py`, the parent's kernel unchanged), msaa 1 and 4 alike:
  1. a full edge table (384 edges in 12 combs, hit_room 800), h = 1 .. 6 tile rows: fell back [0, 0, 1, 1, 1, 1] in every pass — the batch walks again
     from THREE tile rows on (hits <= 768 at two, <= 1 152 at three). Twelve combs of four tile rows, 3 .. 13 points per side: they walk again from
     ELEVEN points on (336 edges, 960 <= hits <= 1 344 for hit_room 992); at ten (312 edges, 864 <= hits <= 1 248, hit_room 1 088) they replay, more than
     800 records. Beside two ordinary batches: 1 of 3 runs falls back (1 of 4 workgroups in the first pass); slots <= 5 548.
  2. (a) fifteen octagons behind a saw of v vertices: the largest key is 8 191 behind key0 for v = 7 233 .. 7 236 (fell back 0 in every pass) and 8 195 for
     v = 7 237 .. 7 240 (fell back 1 in every pass), where the layout puts it; hits <= 240. The last follower a pentagon: 8 188 (0) and 8 192 exactly (1) at
     the same v. A saw of 960 vertices: 0. (b) twelve rings of 928 slots
     outside the slab: fell back 1 in every pass with hits <= 64; without the slab twelve runs, fell back 0.
  3. combs of 11 points, their turn has >= 1 440 hits for <= 992 records: fell back 1 in every pass, in either order; overflow[76] is 0 in all four
     passes of a fresh frame (two turns in the first, by the costs: 840 cells for a pool of 768) and 1 in the pass that takes a stale run of sixteen.
  4. the largest wavefront (first pass / steady pass, msaa 1): fills and strokes 268 / 301, folded 240 / 236; glyphs 306 / 308, folded 235 / 227; the
     cubic scene of test_gpu_bin_replay.py 565, as recorded there."""
import collections
import ctypes as C

import numpy as np
import pytest

from test_gpu_bin_footprint import SIZE, TILE, Item, batch_limits, cost_words, flat, item_costs, pack, polygon, rect, ring, scene_of, spots  # noqa: F401 (flat: a fixture)
from test_gpu_bin_lanes import bin_word
from test_gpu_bin_replay import DIRECT, FALLBACK_WORD, FELL_BACK, LARGEST_WAVE_HITS, REPLAYED, cubic_scene, flag_words, pinned
from test_gpu_parity import gpu, make_renderer  # noqa: F401 (the module-scoped fixture and the helper of the parity tests)

pytestmark = pytest.mark.gpu

PASSES = 4
EXTRA_TURNS_WORD = 76  # of the frame's flag words (kExtraTurnsWord): turns beyond the first of workgroups that took a run the host cut (r.bin_batches)
HIT_REGION, EDGES_PER_RECORDS = 800, 4  # hit_room = 800 + 4 * (the edge table's free places)
KEY_RANGE = 1 << 13  # kHitKeyBits = 13
MSAA = [1, 4]
DEFAULT = [pytest.param(None, id="128-threads")]  # (the `flat` environment around the kernel that replays; the 64-thread one is a reference here)
Pass = collections.namedtuple("Pass", "image word fell_back extra_turns")


# ---------------------------------------------------------------------------------------------- Shapes
def comb(col, row, h, n, height=SIZE):
    """A zig-zag band of n points per side in tile column `col`, tile rows row .. row + h - 1 (image rows: y grows downwards there, upwards in the
    scene): 2 n fill edges, of which 2 n - 2 run from the top tile row to the bottom one; 12 px wide, 2 px inside its tiles on every side. The
    Shape is the same in every column and row (local pixels from its top left corner), so its hull is."""
    from contrast_renderer_amd.path import Path
    wide, tall, gap = 12.0, TILE * h - 4.0, 6.0
    upper = [(wide * i / (n - 1), 0.0 if i % 2 == 0 else tall - gap) for i in range(n)]
    lower = [(x, y + gap) for x, y in reversed(upper)]
    return Item([Path.from_polygon([(x, -y) for x, y in upper + lower])], TILE * col + 2.0, height - (TILE * row + 2.0), 1.0)


def saw(v):
    """A square whose top side is a saw of v - 4 points, all of them well inside the square: v fill edges, a hull of the FOUR corners whatever v is
    (the hull of a regular polygon of thousands of vertices would depend on the margin the hull's turns are decided with)."""
    from contrast_renderer_amd.path import Path
    m = v - 4
    teeth = [(-1.0 + 2.0 * (j + 1) / (m + 1), 0.6 if j % 2 == 0 else 0.2) for j in range(m)]
    return [Path.from_polygon([(-1.0, -1.0), (-1.0, 1.0)] + teeth + [(1.0, 1.0), (1.0, -1.0)])]


def slots(tris, fill_edges, hull):
    """The slots an item owns (edge_slots.hpp item_slots): 4 per triangle | the fill edges rounded up to 4 | 4 | 4 * (hull - 2) | 28."""
    return 4 * tris + ((fill_edges + 3) & ~3) + 4 + (4 * (hull - 2) if hull else 0) + 28


def slots_bound(costs):
    """... and a bound on it from the costs alone (edges = fill edges + hull vertices)."""
    return sum(4 * t + 4 * e + 36 for t, e, _ in costs)


def hits_bound(costs):
    """Every edge and every triangle of an item enters a cell of the item's rectangle once at most."""
    return sum((e + t) * cells for t, e, cells in costs)


def as_scene(items, size=(SIZE, SIZE)):
    batch, transforms, colors = scene_of(items, size)
    return dict(batch=batch, transforms=transforms, colors=colors, width=size[0], height=size[1], winding_bits=4, n_items=len(items))


# ---------------------------------------------------------------------------------------------- passes and their counters
def host_runs(frame, n):
    """The runs the host cuts the frame's items into by the costs of its latest verified pass (crh_debug_flat_batches), in item order."""
    lib = frame.lib
    batch_limits(lib)  # (declares the function)
    runs, limits = (C.c_uint32 * (2 * n))(), (C.c_uint32 * 4)()
    count = lib.crh_debug_flat_batches(cost_words(frame, n), n, runs, n, limits)
    assert count >= 1
    return sorted((int(runs[2 * k]), int(runs[2 * k + 1])) for k in range(count))


def one_pass(scene, frame, sc, upload=True):
    """upload: the instances are set for this pass; otherwise it draws the resident ones (a frame whose passes see new instances every time sizes
    the places of its lists for a moving camera, and a scene with thousands of entries in a few tiles then outgrows them once)."""
    frame.clear()
    if upload:
        scene.render(frame, sc["transforms"], sc["colors"])
    else:
        scene.render(frame)
    image = frame.download()
    word, words = bin_word(frame)[0], flag_words(frame)
    return Pass(image, word, words[FALLBACK_WORD], words[EXTRA_TURNS_WORD])


def draw(gpu, sc, msaa, passes=PASSES, rows=None, then_rows=None, **env):  # noqa: F811
    """`passes` passes of the scene into one new frame -> ([Pass], the costs its first pass left, the runs the host cut by them: of the scenes
    packed here, one draw item per Item). rows: the frame's slab; then_rows: its slab from the second pass on."""
    n = sc.get("n_items")
    with pinned(CRH_BIN_ITEMS=32, **env):
        r = make_renderer(gpu, msaa, sc["winding_bits"])
        scene = gpu.Scene(r, sc["batch"])
        assert scene.status() == 0
        frame = gpu.Frame(r, sc["width"], sc["height"])
        if rows is not None:
            frame.set_tile_rows(*rows)
        out, costs, runs = [], None, None
        for k in range(passes):
            out.append(one_pass(scene, frame, sc, upload=k == 0))
            if k == 0 and n is not None:
                costs, runs = item_costs(frame, n), host_runs(frame, n)
            if k == 0 and then_rows is not None:
                frame.set_tile_rows(*then_rows)
        assert scene.status() == 0
    return out, costs, runs


def oracle_image(oracle_lib, sc, msaa, rows=None):
    oracle = oracle_lib.Oracle(sc["batch"], 4)
    assert oracle.status() == 0
    expect = oracle.render(sc["width"], sc["height"], msaa, sc["winding_bits"], sc["transforms"], sc["colors"])
    assert expect.any(), "the scene draws something"
    if rows is not None:
        masked = np.zeros_like(expect)
        masked[rows[0]:rows[1]] = expect[rows[0]:rows[1]]
        expect = masked
    return expect


def assert_frames(run, expect, what):
    for k, p in enumerate(run):
        assert np.array_equal(p.image, expect), f"{what}, pass {k}: {(p.image != expect).any(axis=2).sum()} pixels differ"


def references(gpu, oracle_lib, sc, msaa, rows=None, passes=PASSES, **env):  # noqa: F811
    """The oracle's image of the scene (masked to the slab) — once the two other references have drawn exactly it in every pass: the walk again
    and the 64-thread workgroup. What then equals this image equals all three."""
    expect = oracle_image(oracle_lib, sc, msaa, rows)
    walk, _, _ = draw(gpu, sc, msaa, passes, rows, CRH_BIN_REPLAY=0, **env)
    narrow, _, _ = draw(gpu, sc, msaa, passes, rows, CRH_BIN_FLAT_THREADS=64, **env)
    assert_frames(walk, expect, "CRH_BIN_REPLAY=0")
    assert_frames(narrow, expect, "CRH_BIN_FLAT_THREADS=64")
    assert all(not (p.word & (REPLAYED | FELL_BACK)) and p.fell_back == 0 for p in walk + narrow), [(hex(p.word), p.fell_back) for p in walk + narrow]
    return expect


def replayed(gpu, sc, msaa, expect, what, rows=None, passes=PASSES, **env):  # noqa: F811
    """The passes with the kernel that replays, every frame `expect`: the first through the pair stream, from the third on the lists in place."""
    run, costs, runs = draw(gpu, sc, msaa, passes, rows, **env)
    assert_frames(run, expect, what)
    assert all(p.word & REPLAYED for p in run), [hex(p.word) for p in run]
    for p in run:  # (bit 12 of the binning word says what the counter says)
        assert bool(p.word & FELL_BACK) == (p.fell_back > 0), (hex(p.word), p.fell_back)
    assert not (run[0].word & DIRECT), hex(run[0].word)
    assert all(p.word & DIRECT for p in run[2:]), [hex(p.word) for p in run]
    return run, costs, runs


def measured(gpu, oracle_lib, items, msaa):  # noqa: F811
    """The items' costs: one pass into a new frame, which draws the oracle's image."""
    sc = as_scene(items)
    run, costs, _ = draw(gpu, sc, msaa, 1)
    assert_frames(run, oracle_image(oracle_lib, sc, msaa), "a pass that measures")
    return costs


def both_kinds(run):
    """A verified pass through the pair stream and the passes with the lists in place."""
    return [run[0]] + run[2:]


# ---------------------------------------------------------------------------------------------- 1. the table is full
_COMB_EDGES = {}


def comb_edges(gpu, oracle_lib, h):  # noqa: F811
    """Edges (fill edges + hull vertices) of the combs of h tile rows with n = 3 .. 14 points, as a frame's first pass counts them: measured once per h
    (the hull's turns are decided with a margin, so how many of the band's outer points it keeps depends on the comb's proportions)."""
    if h not in _COMB_EDGES:
        ns = list(range(3, 15))
        costs = measured(gpu, oracle_lib, [comb(c, 0, h, n) for c, n in enumerate(ns)], 1)
        for n, (tris, edges, cells) in zip(ns, costs):
            assert tris == 0 and cells == h and 2 * n + 3 <= edges <= 2 * n + 12, (n, tris, edges, cells)  # (the band's hull: some of its n + 2 outer points)
        _COMB_EDGES[h] = {n: edges for n, (_, edges, _) in zip(ns, costs)}
    return dict(_COMB_EDGES[h])


def full_table_of_combs(gpu, oracle_lib, limits, h):  # noqa: F811
    """Combs of h tile rows, one per tile column from column 0 on, whose edges fill a batch's edge table exactly."""
    max_items, _, max_edges, _ = limits
    edges = comb_edges(gpu, oracle_lib, h)
    ns = sorted(edges)
    chosen = pack([edges[n] for n in ns], max_edges, max_items)
    assert chosen is not None, f"no choice of combs makes {max_edges} edges: {edges}"
    return [comb(col, 0, h, ns[i]) for col, i in enumerate(chosen)]


def assert_one_full_batch(costs, runs, limits, h, n_combs):
    """The combs are ONE batch with a full edge table, in the first pass (sixteen candidates that all fit) and in the host's runs; keys stay in range."""
    max_items, max_tris, max_edges, max_pool = limits
    mine = costs[:n_combs]
    assert n_combs <= max_items and all(t == 0 and cells == h for t, _, cells in mine), mine
    assert sum(e for _, e, _ in mine) == max_edges and sum(t for t, _, _ in mine) <= max_tris and sum(c for _, _, c in mine) <= max_pool
    assert (0, n_combs) in runs, runs
    assert slots_bound(costs) < KEY_RANGE, "no key of this scene is out of a record's range"


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", DEFAULT, indirect=True)
def test_a_full_edge_table_of_combs_walks_again_from_some_height_on(flat, oracle_lib, msaa):
    """Graded: the same full batch of combs, one tile row taller per step. At one and two tile rows the hits cannot exceed the 800 records of a full
    table (384 * 2 = 768: asserted from the costs), so the batch replays; some steps later it walks again, and from then on at every step."""
    gpu, limits = flat  # noqa: F811
    steps = list(range(1, 7))
    fell, bounds = {}, {}
    for h in steps:
        items = full_table_of_combs(gpu, oracle_lib, limits, h)
        sc = as_scene(items)
        expect = references(gpu, oracle_lib, sc, msaa)
        run, costs, runs = replayed(gpu, sc, msaa, expect, f"combs of {h} tile rows")
        assert_one_full_batch(costs, runs, limits, h, len(items))
        assert runs == [(0, len(items))]
        bound = bounds[h] = hits_bound(costs)
        fell[h] = [p.fell_back for p in run]
        print(f"msaa {msaa}: combs of {h} tile rows: {len(items)} items, {sum(e for _, e, _ in costs)} edges, hits <= {bound}, slots <= {slots_bound(costs)}, "
              f"fell back per pass {fell[h]}")
        if bound <= HIT_REGION:
            assert fell[h] == [0] * PASSES, (h, fell[h])
        assert len(set(fell[h][k] > 0 for k in (0, 2, 3))) == 1, f"both kinds of pass decide alike: {fell[h]}"
    assert bounds[steps[0]] <= HIT_REGION and fell[steps[0]] == [0] * PASSES, "the light end replays"
    assert all(n == 1 for n in fell[steps[-1]]), f"the heavy end walks again, its one batch in every pass: {fell[steps[-1]]}"
    switch = min(h for h in steps if fell[h][0] > 0)
    print(f"msaa {msaa}: the full batch walks again from {switch} tile rows on")
    assert all(all(n == 1 for n in fell[h]) for h in steps if h >= switch), fell
    assert all(fell[h] == [0] * PASSES for h in steps if h < switch), fell


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", DEFAULT, indirect=True)
def test_combs_of_four_rows_walk_again_from_some_number_of_teeth_on(flat, oracle_lib, msaa):
    """Graded the other way: twelve combs of four tile rows, one point more per side on every comb per step, as long as they are one batch. The edge
    table is NOT full here, so the records continue into the edge places the batch leaves free (hit_room = 800 + 4 * (384 - edges)): the steps in
    the middle replay more than 800 records. Where the host's bound on the hits is within hit_room the batch must replay, where the long edges
    alone ((2 n - 2) per comb, four cells each) exceed it the batch must walk again; in between the kernel's count decides, once."""
    gpu, limits = flat  # noqa: F811
    h, n_combs = 4, 12
    edges = comb_edges(gpu, oracle_lib, h)
    steps = [n for n in sorted(edges) if n_combs * edges[n] <= limits[2]]
    fell, must_replay, must_walk = {}, [], []
    for n in steps:
        sc = as_scene([comb(col, 0, h, n) for col in range(n_combs)])
        expect = references(gpu, oracle_lib, sc, msaa)
        run, costs, runs = replayed(gpu, sc, msaa, expect, f"combs of {n} points")
        assert all(c == (0, edges[n], h) for c in costs) and runs == [(0, n_combs)] and slots_bound(costs) < KEY_RANGE, (costs, runs)
        room = HIT_REGION + EDGES_PER_RECORDS * (limits[2] - n_combs * edges[n])
        at_most, at_least = hits_bound(costs), n_combs * (2 * n - 2) * h
        fell[n] = [p.fell_back for p in run]
        print(f"msaa {msaa}: combs of {n} points: {n_combs * edges[n]} edges, {at_least} <= hits <= {at_most}, hit_room {room}, fell back per pass {fell[n]}")
        if at_most <= room:
            must_replay.append(n)
            assert fell[n] == [0] * PASSES, (n, fell[n])
        if at_least > room:
            must_walk.append(n)
            assert fell[n] == [1] * PASSES, (n, fell[n])
        assert fell[n] in ([0] * PASSES, [1] * PASSES), f"every pass decides alike: {fell[n]}"
    assert steps[0] in must_replay and steps[-1] in must_walk, (steps, must_replay, must_walk)
    switch = min(n for n in steps if fell[n][0])
    print(f"msaa {msaa}: twelve combs of four tile rows walk again from {switch} points per side on")
    assert all(fell[n] == ([1] * PASSES if n >= switch else [0] * PASSES) for n in steps), fell


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", DEFAULT, indirect=True)
def test_a_heavy_batch_beside_ordinary_ones(flat, oracle_lib, msaa):
    """The full batch of six-row combs above two batches of the footprint catalogue's polygons and rings (one to four tiles each, on other tile
    rows): the heavy batch walks again, the others replay — in one pass, into the same lists."""
    gpu, limits = flat  # noqa: F811
    h = 6
    combs = full_table_of_combs(gpu, oracle_lib, limits, h)
    kinds = [polygon(k) for k in range(3, 19)] + [ring(q) for q in range(3, 11)]
    others = [Item(kinds[i % len(kinds)], x, y + 2.0 * (i % 3), 7.0 if i % 4 else 12.0) for i, (x, y, _) in enumerate(spots(2 * limits[0], 7.0))]
    sc = as_scene(combs + others)
    expect = references(gpu, oracle_lib, sc, msaa)
    run, costs, runs = replayed(gpu, sc, msaa, expect, "combs beside ordinary batches")
    every, _, _ = replayed(gpu, sc, msaa, expect, "... with every batch walking again", CRH_BIN_REPLAY_CAP=0)
    assert_one_full_batch(costs, runs, limits, h, len(combs))
    assert all(0 < c[2] <= 16 for c in costs[len(combs):]), costs[len(combs):]
    print(f"msaa {msaa}: {len(costs)} items in the runs {runs}, slots <= {slots_bound(costs)}; fell back {[p.fell_back for p in run]} of {[p.fell_back for p in every]} batches")
    for p, q in zip(both_kinds(run), both_kinds(every)):
        assert 0 < p.fell_back < q.fell_back, (p.fell_back, q.fell_back)
    assert all(p.fell_back == 1 and q.fell_back == len(runs) for p, q in zip(run[2:], every[2:])), "of the host's runs exactly the combs' walks again"


# ---------------------------------------------------------------------------------------------- 2. a key out of the record's range
FOLLOWER_SIDES = 8  # a follower: a regular octagon inside one tile — 8 fill edges, 8 hull edges, one cell


def followers(n, last_sides=FOLLOWER_SIDES):
    """n one-tile polygons on the tile centres of the frame's bottom row: octagons, the last one a polygon of `last_sides`."""
    return [Item(polygon(FOLLOWER_SIDES if i + 1 < n else last_sides), x, y, s) for i, (x, y, s) in enumerate(spots(n, 6.0))]


def largest_relative_key(filler_slots, n_followers, last_sides=FOLLOWER_SIDES):
    """The largest key of a batch of one filler and n one-tile polygons behind it, relative to the filler's first slot: the last hull edge of the last
    follower (a regular polygon around a tile's centre: every one of its edges crosses that tile). Its fill edges come first, rounded up to 4,
    then 4 backdrop slots, then the hull's edges."""
    hull0 = ((last_sides + 3) & ~3) + 4
    return filler_slots + (n_followers - 1) * slots(0, FOLLOWER_SIDES, FOLLOWER_SIDES) + hull0 + last_sides - 1


def filler_scene(v, n_followers, last_sides=FOLLOWER_SIDES):
    return [Item(saw(v), SIZE / 2, SIZE / 2, 56.0)] + followers(n_followers, last_sides)


def assert_followers_only(costs, last_sides=FOLLOWER_SIDES):
    """The filler is not binned by k_bin_flat (it is queued: more edges than a batch holds); the followers cannot outgrow any table of records."""
    assert costs[0] == (0, 0, 0), costs[0]
    assert all(c == (0, 2 * FOLLOWER_SIDES, 1) for c in costs[1:-1]) and costs[-1] == (0, 2 * last_sides, 1), costs[1:]
    assert hits_bound(costs) <= HIT_REGION, "a fall-back of this batch can only be a key out of range"


@pytest.mark.parametrize("last_sides", [8, 5], ids=["8191-8195", "8188-8192"])
@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", DEFAULT, indirect=True)
def test_an_oversize_item_in_front_pushes_its_followers_keys_out_of_range(flat, oracle_lib, msaa, last_sides):
    """Item 0 is a polygon of v vertices that the queue kernel draws — it counts as empty in its batch but owns its slots, and key0 is ITS first
    slot. Fifteen one-tile polygons follow in the same batch. Eight consecutive v around the one at which the last follower's largest key reaches
    8 192 behind key0 (the slot layout says where; the fill edges are rounded up to 4, so the figure moves by 4 every fourth v). The last follower
    decides which figures the sweep meets: behind an octagon the largest key goes from 8 191 (the last one a record holds: the batch replays) to
    8 195, behind a pentagon from 8 188 to 8 192 exactly (ONE hit of the batch is out of range, by one) — together, 8 191 fits and 8 192 does not."""
    gpu, limits = flat  # noqa: F811
    n_followers = limits[0] - 1
    # the filler's hull is its four corners: read from a sibling small enough to be binned
    sibling = measured(gpu, oracle_lib, filler_scene(100, n_followers, last_sides), msaa)
    assert sibling[0][:2] == (0, 100 + 4) and sibling[1:-1] == [(0, 2 * FOLLOWER_SIDES, 1)] * (n_followers - 1) and sibling[-1] == (0, 2 * last_sides, 1), sibling
    largest = lambda v: largest_relative_key(slots(0, v, 4), n_followers, last_sides)  # noqa: E731
    first = next(v for v in range(400, 10000) if largest(v) >= KEY_RANGE)
    assert (largest(first - 1), largest(first)) == {8: (KEY_RANGE - 1, KEY_RANGE + 3), 5: (KEY_RANGE - 4, KEY_RANGE)}[last_sides] and first > limits[2], first
    fell = {}
    for v in range(first - 4, first + 4):
        sc = as_scene(filler_scene(v, n_followers, last_sides))
        expect = references(gpu, oracle_lib, sc, msaa)
        run, costs, runs = replayed(gpu, sc, msaa, expect, f"a filler of {v} vertices")
        assert_followers_only(costs, last_sides)
        assert runs == [(0, limits[0])], runs
        fell[v] = [p.fell_back for p in run]
        print(f"msaa {msaa}: filler of {v} vertices, {slots(0, v, 4)} slots, largest key {largest(v)} behind key0, hits <= {hits_bound(costs)}: fell back per pass {fell[v]}")
    for v, per_pass in fell.items():
        assert per_pass == [1 if v >= first else 0] * PASSES, f"the batch walks again from {first} vertices on: {fell}"


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", DEFAULT, indirect=True)
def test_an_oversize_item_of_a_thousand_slots_keeps_its_followers_in_range(flat, oracle_lib, msaa):
    gpu, limits = flat  # noqa: F811
    n_followers = limits[0] - 1
    v = 960
    assert v > limits[2] and largest_relative_key(slots(0, v, 4), n_followers) < KEY_RANGE // 4
    sc = as_scene(filler_scene(v, n_followers))
    expect = references(gpu, oracle_lib, sc, msaa)
    run, costs, runs = replayed(gpu, sc, msaa, expect, "a filler of 1 000 slots")
    assert_followers_only(costs)
    assert [p.fell_back for p in run] == [0] * PASSES


SLAB_SIZE = (SIZE, 2 * SIZE)  # (width, height)
SLAB_ROWS = (SIZE, 2 * SIZE)  # the lower half, in image rows
RING_SEGMENTS, N_RINGS, N_INSIDE = 100, 12, 4


def slab_scene():
    """Twelve rings of 100 quadratic segments in the upper half of a 256 x 512 frame (more than a tile row above the lower half), then four one-tile
    octagons in the lower half: sixteen consecutive items."""
    w, height = SLAB_SIZE
    rings = [Item(ring(RING_SEGMENTS), 50.0 + 52.0 * (i % 4), height - (70.0 + 35.0 * (i // 4)), 30.0) for i in range(N_RINGS)]
    inside = [Item(polygon(FOLLOWER_SIDES), TILE * (2 + 3 * i) + TILE / 2, height - (SLAB_ROWS[0] + TILE * (2 + i) + TILE / 2), 6.0) for i in range(N_INSIDE)]
    return as_scene(rings + inside, SLAB_SIZE)


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", DEFAULT, indirect=True)
def test_items_outside_a_slab_push_the_keys_of_those_inside_out_of_range(flat, oracle_lib, msaa):
    """A slab pass over the lower half: the rings have no tile row in it (`elsewhere`: neither binned nor queued, empty in their batch), yet they
    own about 900 slots each, so the octagons behind twelve of them have keys beyond 13 bits. Without the slab every item is binned, the batches are
    cut by cost (a ring fills the triangle table nearly alone), and nothing walks again."""
    gpu, limits = flat  # noqa: F811
    sc = slab_scene()
    whole = references(gpu, oracle_lib, sc, msaa)
    run, costs, runs = replayed(gpu, sc, msaa, whole, "without a slab")
    assert all(t == RING_SEGMENTS and RING_SEGMENTS < e <= 2 * RING_SEGMENTS + 1 and 0 < cells <= limits[3] for t, e, cells in costs[:N_RINGS]), costs
    assert all(c == (0, 2 * FOLLOWER_SIDES, 1) for c in costs[N_RINGS:]), costs[N_RINGS:]
    # (the costs give fill edges + hull vertices; the path's closing point may count as a fill edge of its own: the fewer slots of the two readings)
    ring_slots = [min(slots(t, fe, e - fe) for fe in (RING_SEGMENTS, RING_SEGMENTS + 1)) for t, e, _ in costs[:N_RINGS]]
    assert sum(ring_slots) >= KEY_RANGE, "every key of the items inside the slab is out of range behind the first ring's first slot"
    assert max(4 * t + 4 * e + 36 for t, e, _ in costs) + N_INSIDE * slots(0, FOLLOWER_SIDES, FOLLOWER_SIDES) < KEY_RANGE and all(min(b, N_RINGS) - a <= 1 for a, b in runs if a < N_RINGS), (ring_slots, runs)
    assert [p.fell_back for p in run] == [0] * PASSES, "cut by cost, no batch reaches from a ring to an octagon four rings on"
    print(f"msaa {msaa}: rings of {ring_slots} slots; without a slab the runs {runs}, fell back {[p.fell_back for p in run]}")

    masked = references(gpu, oracle_lib, sc, msaa, rows=SLAB_ROWS)
    assert masked[SLAB_ROWS[0]:].any() and not masked[:SLAB_ROWS[0]].any()
    run, costs, runs = replayed(gpu, sc, msaa, masked, "the slab pass", rows=SLAB_ROWS)
    assert all(c == (0, 0, 0) for c in costs[:N_RINGS]) and all(c == (0, 2 * FOLLOWER_SIDES, 1) for c in costs[N_RINGS:]), costs
    assert hits_bound(costs) <= HIT_REGION and runs == [(0, N_RINGS + N_INSIDE)], (costs, runs)
    print(f"msaa {msaa}: the slab pass: hits <= {hits_bound(costs)}, fell back per pass {[p.fell_back for p in run]}")
    assert all(p.fell_back >= 1 for p in run), [p.fell_back for p in run]


# ---------------------------------------------------------------------------------------------- 3. two turns of one workgroup
def two_turn_scenes(gpu, oracle_lib, limits):  # noqa: F811
    """Sixteen candidates whose edges fit a batch and whose tile cells do not: twelve six-row combs (heavy: at least (fill edges - 2) * 6 hits) and
    four rectangles of 12 x 16 tiles (light: eight edges each, and together exactly the pool). Combs first, the fourth rectangle waits for the
    second turn; rectangles first, they fill the pool and all the combs wait."""
    h, n_combs = 6, 12
    edges = comb_edges(gpu, oracle_lib, h)
    n = max(k for k, e in edges.items() if n_combs * e + 4 * 8 <= limits[2])
    combs = [comb(col, 0, h, n) for col in range(n_combs)]
    rects = [Item(rect(1.0, 1.0, TILE * 12 - 1.0, SIZE - 1.0), 0.0, 0.0, 1.0) for _ in range(4)]
    return n, {"combs-first": combs + rects, "combs-last": rects + combs}


def assert_two_turns(costs, limits, n):
    h, n_combs = 6, 12
    max_items, max_tris, max_edges, max_pool = limits
    combs = [c for c in costs if c[2] == h]
    rects = [c for c in costs if c[2] == 12 * 16]
    assert len(costs) == max_items and len(combs) == n_combs and len(rects) == 4 and all(c == (0, 8, 192) for c in rects), costs
    assert sum(e for _, e, _ in costs) <= max_edges and sum(c for _, _, c in rects) == max_pool, "all sixteen are set up; the pool decides the turns"
    assert sum(c for _, _, c in costs) > max_pool and sum(c for _, _, c in costs) <= 2 * max_pool
    # the turn with the combs cannot replay: every long edge of a comb enters a cell in each of its six tile rows
    comb_hits = n_combs * (2 * n - 2) * h
    room_at_most = HIT_REGION + EDGES_PER_RECORDS * (max_edges - sum(e for _, e, _ in combs))
    assert comb_hits > room_at_most, (comb_hits, room_at_most)
    assert slots_bound(costs) < KEY_RANGE
    return comb_hits, room_at_most


@pytest.mark.parametrize("order", ["combs-first", "combs-last"])
@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("flat", DEFAULT, indirect=True)
def test_one_turn_of_a_workgroup_walks_again_and_the_other_replays(flat, oracle_lib, msaa, order):
    """replay_off and the wavefronts' counts are the TURN's. Combs first: the first turn (combs and three rectangles) walks again, the second (one
    rectangle) replays; combs last: the first turn (the rectangles, the pool exactly) replays, the second (the combs) walks again. That the combs'
    turn cannot replay follows from the costs, so `fell back == 1` says that the other turn did.

    The kernel counts extra turns (overflow[76]) only for workgroups that took a run the HOST cut (r.bin_batches): a fresh frame's first pass has
    no such runs, its two turns follow from the costs (the sixteen candidates' cells exceed the pool), and the word stays 0. The counted case is
    drawn as well: the costs are taken in a slab of ONE tile row, where every item has a sliver of its cells and the host cuts one run of
    sixteen; the slab is then lifted, and the next pass — a verified one, through the pair stream — takes that stale run in two turns."""
    gpu, limits = flat  # noqa: F811
    n, scenes_ = two_turn_scenes(gpu, oracle_lib, limits)
    sc = as_scene(scenes_[order])
    expect = references(gpu, oracle_lib, sc, msaa)
    run, costs, runs = replayed(gpu, sc, msaa, expect, order)
    comb_hits, room = assert_two_turns(costs, limits, n)
    assert len(runs) == 2, runs  # (the host cuts where the kernel's own fitting did)
    print(f"msaa {msaa}, {order}: combs of {n} points, their turn has >= {comb_hits} hits for <= {room} records; runs {runs}; "
          f"fell back per pass {[p.fell_back for p in run]}, extra turns per pass {[p.extra_turns for p in run]}")
    assert [p.fell_back for p in run] == [1] * PASSES
    assert [p.extra_turns for p in run] == [0] * PASSES, "no run the host cut needs a second turn"

    # ... and a run the host cut for one turn that needs two (the extra turn is counted): the first pass in a slab of one tile row, the others without
    top_row = (0, TILE)
    sliver = oracle_image(oracle_lib, sc, msaa, rows=top_row)
    stale = {}
    for name, env in (("replay", {}), ("walk again", dict(CRH_BIN_REPLAY=0)), ("64 threads", dict(CRH_BIN_FLAT_THREADS=64))):
        stale[name], slab_costs, slab_runs = draw(gpu, sc, msaa, PASSES, rows=top_row, then_rows=(0, SIZE), **env)
        assert_frames(stale[name][:1], sliver, f"{order}, one tile row, {name}")
        assert_frames(stale[name][1:], expect, f"{order}, a stale run, {name}")
        if name == "replay":
            assert slab_runs == [(0, limits[0])] and sum(c for _, _, c in slab_costs) <= limits[3], (slab_costs, slab_runs)
    took = stale["replay"][1:]
    print(f"msaa {msaa}, {order}: a stale run of sixteen: extra turns per pass {[p.extra_turns for p in took]}, fell back {[p.fell_back for p in took]}, words {[hex(p.word) for p in took]}")
    assert not (took[0].word & DIRECT) and (took[0].word & REPLAYED)
    assert took[0].extra_turns >= 1
    assert [p.fell_back for p in took] == [1, 1, 1]
    assert all(p.fell_back == 0 and not (p.word & REPLAYED) for p in stale["walk again"] + stale["64 threads"])


# ---------------------------------------------------------------------------------------------- 4. other scene kinds under a cap
def largest_wave_hits(fell_back_at, upper=4096):
    """The most records a wavefront of the passes `fell_back_at(cap)` looks at wants to keep: the smallest CRH_BIN_REPLAY_CAP at which none of their
    batches walks again (a batch falls back when a wavefront finds MORE than the cap) — by bisection, a dozen short runs."""
    assert not fell_back_at(upper), "some batch walks again whatever the cap"
    lo, hi = 0, upper  # fell_back_at(hi) is False; below lo it is True
    while lo < hi:
        mid = (lo + hi) // 2
        if fell_back_at(mid):
            lo = mid + 1
        else:
            hi = mid
    return lo


def falls_back_at(gpu, sc, msaa, k, expect, **env):  # noqa: F811
    """cap -> does a batch of pass k fall back under that cap? (k + 1 passes, every frame `expect`)"""
    def at(cap):
        run, _, _ = draw(gpu, sc, msaa, k + 1, CRH_BIN_REPLAY_CAP=cap, **env)
        assert_frames(run, expect, f"cap {cap}")
        return run[k].fell_back > 0
    return at


def test_the_bisection_finds_the_cubic_scenes_largest_wavefront(gpu, oracle_lib):  # noqa: F811
    """test_gpu_bin_replay.py's figure for the steady passes of its scene (read there from an ablation build's workgroup records), found from outside."""
    sc = dict(cubic_scene(), winding_bits=4)
    found = largest_wave_hits(falls_back_at(gpu, sc, 1, 2, oracle_image(oracle_lib, sc, 1)))
    assert found == LARGEST_WAVE_HITS


def other_scenes():
    from contrast_renderer_amd import scenes
    return {
        "fills-and-strokes": lambda: scenes.scene_mixed(64, (SIZE, SIZE)),
        "glyphs": lambda: scenes.scene_glyphs(300, (SIZE, SIZE)),
    }


@pytest.mark.parametrize("msaa", MSAA)
@pytest.mark.parametrize("kind", list(other_scenes()))
def test_other_scene_kinds_under_a_cap_and_with_folded_hulls(gpu, oracle_lib, kind, msaa):  # noqa: F811
    """Fills with strokes, and glyphs (a small dashed-stroke scene has a thousand line triangles per Shape: every item is handed to the queue, k_bin_flat
    finds no hit of it and no batch of it falls back at cap 0 — measured, so it is not among these): with no cap, with every batch walking again, with a cap of half the largest wavefront (some
    batch of EITHER kind of pass walks again: the figure is found per kind), and the same with every hull strip folded (CRH_RASTER_DEBUG=4: the
    strips are binned as cover triangles behind pass 3, whichever way that ran), in both kinds of pass as well."""
    sc = other_scenes()[kind]()
    expect = references(gpu, oracle_lib, sc, msaa)
    run, _, _ = replayed(gpu, sc, msaa, expect, kind)
    assert all(p.fell_back == 0 for p in run), [p.fell_back for p in run]
    every, _, _ = replayed(gpu, sc, msaa, expect, f"{kind}, cap 0", CRH_BIN_REPLAY_CAP=0)
    assert all(p.fell_back > 0 for p in every), f"k_bin_flat bins no hit of this scene: {[p.fell_back for p in every]}"
    largest = [largest_wave_hits(falls_back_at(gpu, sc, msaa, k, expect)) for k in (0, 2)]
    print(f"msaa {msaa}, {kind}: batches {[p.fell_back for p in every]}; the largest wavefront keeps {largest[0]} hits in the first pass, {largest[1]} in a steady one")
    assert min(largest) >= 2
    half = min(largest) // 2
    capped, _, _ = replayed(gpu, sc, msaa, expect, f"{kind}, cap {half}", CRH_BIN_REPLAY_CAP=half)
    for p, q in zip(both_kinds(capped), both_kinds(every)):
        assert 0 < p.fell_back <= q.fell_back, (p.fell_back, q.fell_back)
    # ... folded: the hull edges are no hits any more, so the largest wavefront is found again (it is at most the one above)
    folded = references(gpu, oracle_lib, sc, msaa, CRH_RASTER_DEBUG=4)
    assert np.array_equal(folded, expect)
    run, _, _ = replayed(gpu, sc, msaa, folded, f"{kind}, folded hulls", CRH_RASTER_DEBUG=4)
    assert all(p.fell_back == 0 for p in run), [p.fell_back for p in run]
    largest = [largest_wave_hits(falls_back_at(gpu, sc, msaa, k, folded, CRH_RASTER_DEBUG=4), upper=largest[i]) for i, k in enumerate((0, 2))]
    print(f"msaa {msaa}, {kind}, folded hulls: the largest wavefront keeps {largest[0]} hits in the first pass, {largest[1]} in a steady one")
    assert min(largest) >= 2
    half = min(largest) // 2
    capped, _, _ = replayed(gpu, sc, msaa, folded, f"{kind}, folded hulls, cap {half}", CRH_RASTER_DEBUG=4, CRH_BIN_REPLAY_CAP=half)
    assert all(p.fell_back > 0 for p in both_kinds(capped)), [p.fell_back for p in capped]
